"""NumPy fp64 yardstick of the crowded-field fit of a cube with free positions (mpsfr_fit_cube_psf_free, include/mpsfr.h).

refine() restates the contract with dense algebra on top of frame_free_ref.Problem, one per layer at the start shifts
shift0 + layer_shift[l]: the valid pixels, accept[l][k] and Omega_l, once.  A layer with nothing to fit is dead.  Then
the outer rule of the header with exact solves (numpy.linalg.lstsq over the rows of the Omega_l of the live layers only,
scaled by sqrt(w)): the opening solve per layer; per Gauss-Newton step who carries (per layer, frame_free_ref's rule
with that layer's s2), who is free (carried by some live layer; nobody unless sum |Omega_l| >= sum (acc_l + [b]) + 2 A +
1), the joint design with the columns
    F_kl (the accepted stars of every live layer) | delta_y, delta_x (the free stars) | b_l (the live layers)
where the column of delta_k,y is, on the rows of layer l, F0_kl dP~_kl/ds_y if l carries k and zero otherwise; delta
with its clips (max_step, max_move, and the interval that keeps |s + layer_shift[l]| <= 8 after rounding in every
layer); the closing solve per layer at the final shifts.  converged() is the same rule run until the largest step is
below 1e-13 px: the joint minimiser, as far as fp64 resolves it.

The parity bound of a position (position_bounds()): frame_free_ref's, generalised.  With d_t the largest unclipped
|delta| of outer step t and rho the measured contraction of the converged run (contraction(): the largest
d_(t+1) / d_t over the steps whose d_(t+1) is above step_floor(), the rounding of the reference solve itself), exact
inner solves leave at most pos_tol rho / (1 - rho) after the step that passes the position test.  To this comes the
inexact inner solve of the last step.  The joint system is one weighted least-squares problem with the Jacobi preconditioner
diag(N) and the stop rule relative to g = A^T W D: frame_fit_ref.bounds applies to it as it stands -- convergence,
recurrence, right side, reference -- in the scaled unknowns y = Dg^(1/2) x.  Its term count is per layer: every row of
the design belongs to one layer, an entry of N p in a flux place is one render (at most L stars at a pixel of that
layer, three columns each) and one projection (3600 footprint pixels), NTERM = 3600 + 3 L + 40 as in frame_free_ref;
an entry in a delta place is the sum over the nl layers of F0_kl times such an entry, with a = F0_kl delta one more
product in the walk: NTERM + nl + 2 terms.  The larger count is taken for all places.  delta_k is itself an unknown
(not a / F as on a frame), and its diagonal term is Dg = sum_l F0_kl^2 N_aa,kl, so delta_k,y is within
bound_y / sqrt(sum_l F0_kl^2 N_aa,kl); the same for x.  The bound of a position is the sum of the two terms.  pos_tol
of the parity runs (parity_pos_tol()) is at least ten times the largest inner term, and no step of the yardstick falls
within a tenth of it, so that the two runs take the same decisions at the stop test.  None of this is fitted to what
the GPU gives.
"""
import numpy as np

import frame_fit_ref as F
import frame_free_ref as G

NS = F.NS
APRON = F.APRON
EPS = F.EPS
HELD, BOUND, CLIPPED = G.HELD, G.BOUND, G.CLIPPED


def shift_interval(layer_shift):
    """(lo, hi), each (2,): the shifts s with |s + layer_shift[l]| <= 8 after rounding in every layer, as k_cf_begin
    finds them -- max_l (-8 - t_l) and min_l (8 - t_l), moved inwards by an ulp while a rounded sum still passes."""
    lo, hi = np.full(2, -F.MAX_SHIFT), np.full(2, F.MAX_SHIFT)
    if layer_shift is None:
        return lo, hi
    t = np.asarray(layer_shift, dtype=np.float64)
    for ax in range(2):
        lo[ax] = max(lo[ax], np.max(-F.MAX_SHIFT - t[:, ax]))
        hi[ax] = min(hi[ax], np.min(F.MAX_SHIFT - t[:, ax]))
        for _ in range(4):
            if np.any(lo[ax] + t[:, ax] < -F.MAX_SHIFT):
                lo[ax] = np.nextafter(lo[ax], np.inf)
            if np.any(hi[ax] + t[:, ax] > F.MAX_SHIFT):
                hi[ax] = np.nextafter(hi[ax], -np.inf)
    return lo, hi


class CubeProblem:
    """What is decided once from the start: per layer a frame_free_ref.Problem at shift0 + layer_shift[l]."""

    def __init__(self, cube, var, psf, index, origin, shift0, layer_shift, radius, background):
        cube = np.asarray(cube, dtype=np.float64)
        self.nl, self.n = cube.shape[0], len(origin)
        self.shift0 = np.zeros((self.n, 2)) if shift0 is None else np.array(shift0, dtype=np.float64)
        self.ls = np.zeros((self.nl, 2)) if layer_shift is None else np.asarray(layer_shift, dtype=np.float64)
        self.background = bool(background)
        self.layers = [G.Problem(cube[l], None if var is None else var[l], np.ascontiguousarray(psf[:, l]), index, origin,
                                 self.shift0 + self.ls[l], radius, background) for l in range(self.nl)]
        self.live = [l for l in range(self.nl) if not self.layers[l].none]
        seen = np.zeros(self.n, dtype=bool)
        for l in self.live:
            seen[self.layers[l].acc] = True
        self.seen = seen
        self.lo8, self.hi8 = shift_interval(layer_shift)

    def of_layer(self, shift, l):
        return shift + self.ls[l]


def _block(w, AF, AY, AX, i):
    """The 3 x 3 block (F, a, c) of N of star i of a layer."""
    c = [AF[:, i], AY[:, i], AX[:, i]]
    return np.array([[float(np.sum(w * a * b)) for b in c] for a in c])


def refine(cube, var, psf, index, origin, shift0, layer_shift, radius, background, max_outer=8, pos_tol=1e-3,
           max_step=0.5, max_move=2.0, min_snr=3.0):
    """The call as the header states it, with exact inner solves.  Returns a dict: problem, shift (n, 2), err_shift
    (n, 2), flags, nfree (per star), steps, nouter, nfree_last, posok, carried (the (nl, n) mask of the last step that
    had free stars), closing (per layer Problem.held at the final shifts, None for a dead layer), last (the dense dict
    of the last Gauss-Newton step's joint system with free, the free stars, and ndelta, their number; None if there
    was no step), status (the call's)."""
    cp = CubeProblem(cube, var, psf, index, origin, shift0, layer_shift, radius, background)
    n, nl, back = cp.n, cp.nl, 1 if background else 0
    shift = cp.shift0.copy()
    out = dict(problem=cp, shift=shift, err_shift=np.zeros((n, 2)), flags=np.zeros(n, dtype=int),
               nfree=np.zeros(n, dtype=int), steps=[], nouter=0, nfree_last=0, posok=max_outer == 0,
               carried=np.zeros((nl, n), dtype=bool), closing=[None] * nl, last=None, status=2)
    if not cp.live:
        return out
    Fv, b = {}, {}
    for l in cp.live:
        o = cp.layers[l].held(cp.of_layer(shift, l))
        Fv[l], b[l] = o['F'].copy(), o['b']
    movable = sum(cp.layers[l].nomega for l in cp.live) >= \
        sum(cp.layers[l].nacc + back for l in cp.live) + 2 * int(cp.seen.sum()) + 1
    blocks = {}
    held_last = np.zeros(n, dtype=bool)
    sflag = np.zeros(n, dtype=int)
    for _ in range(max_outer):
        carried = np.zeros((nl, n), dtype=bool)
        design = {}
        for l in cp.live:
            pr = cp.layers[l]
            AF, AY, AX = pr.design(cp.of_layer(shift, l))
            res = pr.d - AF @ Fv[l] - b[l]
            s2 = float(np.sum(pr.w * res * res)) / (pr.nomega - pr.nacc - back)
            nff, naa, ncc = (np.sum(pr.w[:, None] * A * A, axis=0) for A in (AF, AY, AX))
            with np.errstate(invalid='ignore', divide='ignore'):
                cr = np.isfinite(Fv[l]) & (Fv[l] > 0) & (naa > 0) & np.isfinite(naa) & (ncc > 0) & np.isfinite(ncc) \
                    & (Fv[l] > min_snr * np.sqrt(s2 / nff))
            carried[l, pr.acc] = cr & movable
            design[l] = (AF, AY, AX)
        free = np.flatnonzero(carried.any(axis=0))
        held_last[:] = cp.seen
        held_last[free] = False
        out['nfree_last'] = len(free)
        if len(free) == 0:
            out['posok'] = True
            break
        out['carried'] = carried
        place = {k: j for j, k in enumerate(free)}
        nf = len(free)
        nflux = sum(cp.layers[l].nacc for l in cp.live)
        rows, col0 = [], 0
        for j, l in enumerate(cp.live):
            pr = cp.layers[l]
            AF, AY, AX = design[l]
            blk = np.zeros((pr.nomega, nflux + 2 * nf + back * len(cp.live)))
            blk[:, col0:col0 + pr.nacc] = AF
            for i, k in enumerate(pr.acc):
                if carried[l, k]:
                    blk[:, nflux + place[k]] = Fv[l][i] * AY[:, i]
                    blk[:, nflux + nf + place[k]] = Fv[l][i] * AX[:, i]
            if background:
                blk[:, nflux + 2 * nf + j] = 1.0
            rows.append(blk)
            col0 += pr.nacc
        A = np.concatenate(rows, axis=0)
        w = np.concatenate([cp.layers[l].w for l in cp.live])
        d = np.concatenate([cp.layers[l].d for l in cp.live])
        sw = np.sqrt(w)
        x = np.linalg.lstsq(A * sw[:, None], d * sw, rcond=None)[0]
        N = A.T @ (A * w[:, None])
        r = d - A @ x
        last = dict(A=A, w=w, d=d, x=x, N=N, Nabs=np.abs(A).T @ (np.abs(A) * w[:, None]), dg=np.diag(N).copy(), res=r,
                    chi2=float(np.sum(w * r * r)), nacc=nflux, background=background, free=free, ndelta=nf)
        out['last'] = last
        for k in free:                         # the blocks of this step, of the layers that carry the star
            blocks[k] = {}
        col0 = 0
        for j, l in enumerate(cp.live):
            pr = cp.layers[l]
            AF, AY, AX = design[l]
            for i, k in enumerate(pr.acc):
                if carried[l, k]:
                    blocks[k][l] = _block(pr.w, AF, AY, AX, i)
            Fv[l] = x[col0:col0 + pr.nacc].copy()
            if background:
                b[l] = float(x[nflux + 2 * nf + j])
            col0 += pr.nacc
        maxd = 0.0
        for j, k in enumerate(free):
            flag = 0
            for ax in range(2):
                dlt = float(x[nflux + ax * nf + j])
                if not np.isfinite(dlt):
                    dlt = 0.0
                maxd = max(maxd, abs(dlt))
                if abs(dlt) > max_step:
                    dlt = max_step if dlt > 0 else -max_step
                    flag |= CLIPPED
                lo = max(cp.shift0[k, ax] - max_move, cp.lo8[ax])
                hi = min(cp.shift0[k, ax] + max_move, cp.hi8[ax])
                s = shift[k, ax] + dlt
                if s <= lo:
                    s, flag = lo, flag | BOUND
                elif s >= hi:
                    s, flag = hi, flag | BOUND
                shift[k, ax] = s
            sflag[k] = flag
            out['nfree'][k] += 1
        out['steps'].append(maxd)
        out['nouter'] += 1
        if maxd <= pos_tol:
            out['posok'] = True
            break
    for l in cp.live:
        out['closing'][l] = cp.layers[l].held(cp.of_layer(shift, l))
    for k, per_layer in blocks.items():
        S = np.zeros((2, 2))
        for l, blk in per_layer.items():
            cl = out['closing'][l]
            i = int(np.flatnonzero(cp.layers[l].acc == k)[0])
            Fk = cl['F'][i]
            if not (np.isfinite(Fk) and Fk > 0):
                continue
            schur = blk[1:, 1:] - np.outer(blk[1:, 0], blk[0, 1:]) / blk[0, 0]
            with np.errstate(divide='ignore'):
                S = S + (Fk * Fk / cl['s2']) * schur
        with np.errstate(invalid='ignore', divide='ignore'):
            try:
                v = np.diag(np.linalg.inv(S))
            except np.linalg.LinAlgError:
                v = np.zeros(2)
            out['err_shift'][k] = np.where(np.isfinite(v) & (v > 0), np.sqrt(np.abs(v)), 0.0)
    out['flags'][cp.seen] = sflag[cp.seen] | np.where(held_last[cp.seen], HELD, 0)
    out['status'] = 0 if out['posok'] else 1
    return out


def converged(cube, var, psf, index, origin, shift0, layer_shift, radius, background, max_step=0.5, max_move=2.0,
              min_snr=3.0, max_outer=60):
    """refine() until the largest step is below 1e-13 px: the joint minimiser.  Adds rho, the measured contraction."""
    out = refine(cube, var, psf, index, origin, shift0, layer_shift, radius, background, max_outer=max_outer,
                 pos_tol=G.CONVERGED_TOL, max_step=max_step, max_move=max_move, min_snr=min_snr)
    out['floor'] = step_floor(out['last']) if out['last'] is not None else G.RHO_FLOOR
    out['rho'] = contraction(out['steps'], out['floor'])
    return out


def step_floor(dense):
    """Below this a step of the yardstick is the rounding of lstsq, not the iteration: at the fixed point the exact
    delta is zero and the computed one is the error of the reference solve, at most the `reference` term of
    frame_fit_ref.bounds over sqrt(Dg) of the delta place; the shifts it is computed at carry the error of the step
    before, which the iteration hands on shrunk by rho < 1: twice the term covers both.  At least frame_free_ref's
    RHO_FLOOR."""
    nflux, nf = dense['nacc'], dense['ndelta']
    lsq = F.bounds(dense, 1e-12, 1)['terms'][3]
    return max(G.RHO_FLOOR, 2.0 * lsq / float(np.sqrt(np.min(dense['dg'][nflux:nflux + 2 * nf]))))


def contraction(steps, floor):
    """The largest ratio of successive step norms above the rounding floor (0 if there is none)."""
    r = [b / a for a, b in zip(steps[:-1], steps[1:]) if b > floor and a > 0]
    return max(r) if r else 0.0


def inner_bounds(dense, tol, max_iter, nl):
    """frame_fit_ref.bounds on the joint system of a Gauss-Newton step with the term count of the docstring.  Returns
    (bound_y, per free star the bound of delta_y and of delta_x)."""
    A, nflux, nf = dense['A'], dense['nacc'], dense['ndelta']
    bb = F.bounds(dense, tol, max_iter)
    L = int(np.max(np.count_nonzero(A[:, :nflux], axis=1)))
    g1, g3 = (NS + 2 * APRON) ** 2 + L + 40, (NS + 2 * APRON) ** 2 + 3 * L + 40 + nl + 2
    conv, gap, rhs, lsq = bb['terms']
    by = conv + (gap + rhs) * g3 / g1 + lsq
    dg = dense['dg']
    return by, by / np.sqrt(dg[nflux:nflux + nf]), by / np.sqrt(dg[nflux + nf:nflux + 2 * nf])


def position_bounds(conv, pos_tol, tol, max_iter):
    """The parity bound of every free star's final shift against the converged run `conv`, (nfree, 2) in the order of
    conv['last']['free'], and the inner term alone."""
    rho = conv['rho']
    assert rho < 1.0
    _, by, bx = inner_bounds(conv['last'], tol, max_iter, conv['problem'].nl)
    inner = np.stack([by, bx], axis=1)
    return pos_tol * rho / (1.0 - rho) + inner, inner


def parity_pos_tol(conv, tol, max_iter):
    """pos_tol of a parity run against `conv`: ten times the largest inner term -- doubled until no step of the
    yardstick lies within a tenth of it, so that the inexact inner solves cannot decide the stop test."""
    inner = position_bounds(conv, 1.0, tol, max_iter)[1]
    p = 10.0 * float(inner.max())
    steps = np.array(conv['steps'])
    while np.any(np.abs(steps - p) <= 0.1 * p):
        p *= 2.0
    return p
