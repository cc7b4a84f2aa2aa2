"""NumPy fp64 yardstick of the crowded-field fit with free positions (mpsfr_fit_frame_psf_free, include/mpsfr.h).

refine() restates the contract with dense algebra.  From the start shifts s0, once: the valid pixels, the accepted stars
and Omega, by frame_fit_ref.solve.  Then the outer rule of the header with exact inner solves (numpy.linalg.lstsq on the
rows scaled by sqrt(w)): the opening solve at s0; per Gauss-Newton step the free stars (F finite and > 0, F > min_snr
err_F with err_F = sqrt((chi2 / dof) / N_kk) of the F and b before at the current shifts, positive derivative norms,
|Omega| >= 3 accepted + [b] + 1), the columns P~, dP~/ds_y, dP~/ds_x of a free star (columns(): the Keys kernel and its
derivative, psf_fit_ref.keys / dkeys, on the window of render_ref.window; d/ds = -d/dy), delta = (a, c) / F with its
clips; the closing solve at the final shifts.  converged() is the same rule run until the largest step is below 1e-13 px:
the minimiser itself, as far as fp64 resolves it.

The parity bound of a position (position_bounds()).  Let d_t be the largest unclipped |delta| of outer step t and rho the
measured contraction, the largest d_(t+1) / d_t over the steps of the converged run whose d_(t+1) is above 1e-10 px (below
that the steps are the rounding of lstsq, not the iteration).  With exact inner solves and rho < 1 the distance from the
iterate after a step d_T to the minimiser is at most d_(T+1) + d_(T+2) + ... <= d_T rho / (1 - rho); the loop ends at
d_T <= pos_tol, so at most pos_tol rho / (1 - rho) is left.  To this comes what the inexact inner solve of the last step
adds.  In the scaled unknowns y = Dg^(1/2) x of frame_fit_ref the solve ends within bounds(...)['y'] of the exact
solution in the 2-norm -- convergence: the stop rule is relative to g = A^T W D, |rs| <= tol |Dg^(-1/2) g| = tol |Ns y*| <=
tol lmax |y*|, so |y - y*| <= kappa tol |y*| as there; recurrence, right side and reference as there, with the term count
NTERM = 3600 + 3 L + 40 of three columns per star --, so a_k is within that over sqrt(N_aa,k), and delta = a / F within
bound_y / (F_k sqrt(N_aa,k)) to first order; the same for c.  The errors of earlier steps are not added: every step
starts from the shifts it is given, and the yardstick's own contraction covers where it starts.  The bound of a position
is the sum of the two.  pos_tol of the parity runs (parity_pos_tol()) is chosen so that the inner term is at most a tenth
of pos_tol and no step of the yardstick falls within that tenth of pos_tol: then the two runs take the same decisions
at the stop test.  None of this is fitted to what the GPU gives.
"""
import numpy as np

import frame_fit_ref as F
import render_ref as Y
from psf_fit_ref import dkeys, keys, tap_matrix  # noqa: F401  (tap_matrix: the same kernel on the 40 stamp rows)

NS = Y.NS
APRON = Y.APRON
EPS = F.EPS
HELD, BOUND, CLIPPED = 1, 2, 4
RHO_FLOOR = 1e-10
CONVERGED_TOL = 1e-13


def windows(psf, dp, dq):
    """(P~, dP~/ds_y, dP~/ds_x) on the window p, q = -10 .. 49: render_ref.window and its exact derivatives with respect
    to the shift (the sample position is p - dp: d/ds = -d/dy)."""
    p = np.arange(-APRON, NS + APRON)[:, None]
    j = np.arange(NS)[None, :]
    ky, dky = keys(p - dp - j), dkeys(p - dp - j)
    kx, dkx = keys(p - dq - j), dkeys(p - dq - j)
    return ky @ psf @ kx.T, -(dky @ psf @ kx.T), -(ky @ psf @ dkx.T)


def columns(shape, P, origin, shift):
    """The three columns of one star on the frame (zeros outside its footprint)."""
    y0, y1, x0, x1 = Y.footprint(shape, origin)
    wy, wx = y0 - (int(origin[0]) - APRON), x0 - (int(origin[1]) - APRON)
    out = []
    for w in windows(P, shift[0], shift[1]):
        c = np.zeros(shape)
        c[y0:y1, x0:x1] = w[wy:wy + y1 - y0, wx:wx + x1 - x0]
        out.append(c)
    return out


class Problem:
    """What is decided once from the start: the accepted stars, Omega, the weights and the data on it."""

    def __init__(self, image, var, psf, index, origin, shift0, radius, background):
        self.image = np.asarray(image, dtype=np.float64)
        self.psf, self.index, self.origin = psf, index, np.asarray(origin)
        n = len(origin)
        self.shift0 = np.zeros((n, 2)) if shift0 is None else np.array(shift0, dtype=np.float64)
        self.background = bool(background)
        self.base = F.solve(self.image, var, psf, index, origin, self.shift0, radius, background)
        self.acc = self.base['acc']
        self.omega = self.base['omega']
        self.nomega, self.nacc = self.base['nomega'], self.base['nacc']
        self.none = self.base['head_status'] == 2
        if not self.none:
            self.w, self.d = self.base['w'], self.base['d']

    def model(self, k):
        return self.psf[k if self.index is None else int(self.index[k])]

    def design(self, shift):
        """(A_F, A_y, A_x) over Omega at `shift`: one column per accepted star each."""
        cols = [columns(self.image.shape, self.model(k), self.origin[k], shift[k]) for k in self.acc]
        return [np.stack([c[j][self.omega] for c in cols], axis=1) for j in range(3)]

    def lstsq(self, A):
        sw = np.sqrt(self.w)
        return np.linalg.lstsq(A * sw[:, None], self.d * sw, rcond=None)[0]

    def dense(self, A, x):
        """The dict frame_fit_ref.bounds reads, for the design A and its solution x."""
        wo = self.w
        N = A.T @ (A * wo[:, None])
        res = self.d - A @ x
        return dict(A=A, w=wo, d=self.d, x=x, N=N, Nabs=np.abs(A).T @ (np.abs(A) * wo[:, None]), dg=np.diag(N).copy(),
                    res=res, chi2=float(np.sum(wo * res * res)), nacc=self.nacc, background=self.background)

    def held(self, shift, ever_free=0):
        """The solve with the positions held at `shift` over the fixed Omega: the dict of dense() with the columns of
        the result -- F, err, overlap, nkk, b, err_b per accepted star -- and dof = |Omega| - fluxes - 2 ever_free - [b]."""
        AF = self.design(shift)[0]
        A = np.concatenate([AF, np.ones((self.nomega, 1))], axis=1) if self.background else AF
        ref = self.dense(A, self.lstsq(A))
        nacc, dg = self.nacc, ref['dg']
        dof = self.nomega - nacc - 2 * ever_free - (1 if self.background else 0)
        s2 = ref['chi2'] / dof
        ref.update(F=ref['x'][:nacc], err=np.sqrt(s2 / dg[:nacc]), nkk=dg[:nacc],
                   overlap=(ref['N'][:nacc, :nacc].sum(axis=1) - dg[:nacc]) / dg[:nacc],
                   b=float(ref['x'][nacc]) if self.background else 0.0,
                   err_b=float(np.sqrt(s2 / dg[nacc])) if self.background else 0.0, dof=dof, s2=s2)
        return ref


def refine(image, var, psf, index, origin, shift0, radius, background, max_outer=8, pos_tol=1e-3, max_step=0.5,
           max_move=2.0, min_snr=3.0, scale0=None):
    """The call as the header states it, with exact inner solves.  Returns a dict: problem, status (per star, section
    24's), shift (n, 2), err_shift (n, 2), flags, nfree (per star), steps (the largest unclipped |delta| of every outer
    step), nouter, nfree_last, posok, closing (Problem.held at the final shifts; None if nothing is fitted), last (the
    dense() dict of the last Gauss-Newton step with free_idx, the places of its free stars among the accepted ones;
    None if there was none), head_status."""
    pr = Problem(image, var, psf, index, origin, shift0, radius, background)
    n = len(origin)
    shift = pr.shift0.copy()
    out = dict(problem=pr, status=pr.base['status'], shift=shift, err_shift=np.zeros((n, 2)), flags=np.zeros(n, dtype=int),
               nfree=np.zeros(n, dtype=int), steps=[], nouter=0, nfree_last=0, posok=max_outer == 0, closing=None,
               last=None, head_status=2)
    if pr.none:
        return out
    acc, nacc, back = pr.acc, pr.nacc, 1 if background else 0
    open_ = pr.held(shift)
    Fv, b = open_['F'].copy(), open_['b']
    blocks = {}
    held_last = np.zeros(n, dtype=bool)
    sflag = np.zeros(n, dtype=int)
    movable = pr.nomega >= 3 * nacc + back + 1
    for _ in range(max_outer):
        AF, AY, AX = pr.design(shift)
        res = pr.d - AF @ Fv - b
        s2 = float(np.sum(pr.w * res * res)) / (pr.nomega - nacc - back)
        nff, naa, ncc = (np.sum(pr.w[:, None] * A * A, axis=0) for A in (AF, AY, AX))
        with np.errstate(invalid='ignore', divide='ignore'):
            free = movable & np.isfinite(Fv) & (Fv > 0) & (naa > 0) & np.isfinite(naa) & (ncc > 0) & np.isfinite(ncc) \
                & (Fv > min_snr * np.sqrt(s2 / nff))
        held_last[:] = False
        held_last[acc] = ~free
        out['nfree_last'] = int(free.sum())
        if not free.any():
            out['posok'] = True
            break
        fi = np.flatnonzero(free)
        A = np.concatenate([AF, AY[:, fi], AX[:, fi]] + ([np.ones((pr.nomega, 1))] if background else []), axis=1)
        x = pr.lstsq(A)
        nf = len(fi)
        Fv, a, c = x[:nacc].copy(), x[nacc:nacc + nf], x[nacc + nf:nacc + 2 * nf]
        if background:
            b = float(x[-1])
        last = pr.dense(A, x)
        last['free_idx'] = fi
        out['last'] = last
        maxd = 0.0
        for j, i in enumerate(fi):
            k = acc[i]
            ok = np.isfinite(Fv[i]) and Fv[i] > 0
            flag = 0
            for ax, v in enumerate((a[j], c[j])):
                d = v / Fv[i] if ok else 0.0
                if not np.isfinite(d):
                    d = 0.0
                maxd = max(maxd, abs(d))
                if abs(d) > max_step:
                    d = max_step if d > 0 else -max_step
                    flag |= CLIPPED
                lo = max(pr.shift0[k, ax] - max_move, -F.MAX_SHIFT)
                hi = min(pr.shift0[k, ax] + max_move, F.MAX_SHIFT)
                s = shift[k, ax] + d
                if s <= lo:
                    s, flag = lo, flag | BOUND
                elif s >= hi:
                    s, flag = hi, flag | BOUND
                shift[k, ax] = s
            sflag[k] = flag
            out['nfree'][k] += 1
            idx = [i, nacc + j, nacc + nf + j]
            blocks[k] = last['N'][np.ix_(idx, idx)]
        out['steps'].append(maxd)
        out['nouter'] += 1
        if maxd <= pos_tol:
            out['posok'] = True
            break
    ever = int(np.sum(out['nfree'] > 0))
    closing = pr.held(shift, ever)
    out['closing'] = closing
    for i, k in enumerate(acc):
        if k in blocks and np.isfinite(closing['F'][i]) and closing['F'][i] > 0:
            cov = np.linalg.inv(blocks[k]) * closing['s2']
            out['err_shift'][k] = np.sqrt(np.diag(cov)[1:]) / closing['F'][i]
    out['flags'][acc] = sflag[acc] | np.where(held_last[acc], HELD, 0)
    out['head_status'] = 0 if out['posok'] else 1
    return out


def converged(image, var, psf, index, origin, shift0, radius, background, max_step=0.5, max_move=2.0, min_snr=3.0,
              max_outer=60):
    """refine() until the largest step is below 1e-13 px: the minimiser.  Adds rho, the measured contraction."""
    out = refine(image, var, psf, index, origin, shift0, radius, background, max_outer=max_outer, pos_tol=CONVERGED_TOL,
                 max_step=max_step, max_move=max_move, min_snr=min_snr)
    out['rho'] = contraction(out['steps'])
    return out


def contraction(steps):
    """rho of the docstring: the largest ratio of successive step norms above the rounding floor (0 if there is none)."""
    r = [b / a for a, b in zip(steps[:-1], steps[1:]) if b > RHO_FLOOR and a > 0]
    return max(r) if r else 0.0


def inner_bounds(dense, tol, max_iter):
    """frame_fit_ref.bounds on the three-column system of a Gauss-Newton step: the same four terms with NTERM = 3600 +
    3 L + 40.  Returns (bound_y, per free star the bound of delta_y and of delta_x)."""
    A, nacc = dense['A'], dense['nacc']
    b = F.bounds(dense, tol, max_iter)
    L = int(np.max(np.count_nonzero(A[:, :nacc], axis=1)))
    g1, g3 = (NS + 2 * APRON) ** 2 + L + 40, (NS + 2 * APRON) ** 2 + 3 * L + 40
    conv, gap, rhs, lsq = b['terms']
    by = conv + (gap + rhs) * g3 / g1 + lsq
    fi = dense['free_idx']
    nf = len(fi)
    Fv, dg = dense['x'][:nacc][fi], dense['dg']
    return by, by / (Fv * np.sqrt(dg[nacc:nacc + nf])), by / (Fv * np.sqrt(dg[nacc + nf:nacc + 2 * nf]))


def pcg_steps(dense, tol, max_iter):
    """The steps the header's iteration takes on the dense N of a system from a zero start, with the stop rule relative
    to the right-hand side: what a tolerance asks of max_iter (frame_fit_ref.pcg with this rule)."""
    N, dg = dense['N'], dense['dg']
    g = dense['A'].T @ (dense['w'] * dense['d'])
    x, r = np.zeros(len(dg)), g.copy()
    z = r / dg
    p, rho, rhog = z.copy(), float(r @ z), float(g @ (g / dg))
    for it in range(1, max_iter + 1):
        q = N @ p
        alpha = rho / float(p @ q)
        x, r = x + alpha * p, r - alpha * q
        z = r / dg
        rho1 = float(r @ z)
        if rho1 <= tol * tol * rhog:
            return it
        p, rho = z + (rho1 / rho) * p, rho1
    return max_iter + 1


def position_bounds(conv, pos_tol, tol, max_iter):
    """The parity bound of every free star's final shift against the converged run `conv`, (nfree, 2) in the order of
    conv['last']['free_idx'], and the inner term alone."""
    rho = conv['rho']
    assert rho < 1.0
    _, by, bx = inner_bounds(conv['last'], tol, max_iter)
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


_DRAW = {}


def displaced_scene(noise, amplitude=0.3, seed=17):
    """frame_fit_ref.scene(noise) with the starts displaced by a fixed pseudo-random draw of up to +-amplitude px per
    axis (default_rng(seed); the seed is picked so that the contraction of the noiseless scene stays below 1/2 in all
    eight cases of the parity tests, which test_frame_free_host.py asserts); the true shifts stay in 'truth'.  A start is kept inside the +-8 px domain."""
    key = (noise, amplitude, seed)
    if key not in _DRAW:
        s = dict(F.scene(noise))
        rng = np.random.default_rng(seed)
        s['truth'] = s['shift']
        s['shift'] = np.clip(s['shift'] + rng.uniform(-amplitude, amplitude, s['shift'].shape), -8.0, 8.0)
        _DRAW[key] = s
    return _DRAW[key]


_CONV = {}


def scene_converged(with_var, background, radius, noise, **kw):
    """converged() of the displaced scene, once per case."""
    key = (with_var, background, radius, noise, tuple(sorted(kw.items())))
    if key not in _CONV:
        s = displaced_scene(noise)
        _CONV[key] = converged(s['image'], s['var'] if with_var else None, s['psf'], s['index'], s['origin'],
                               s['shift'], radius, background, **kw)
    return _CONV[key]
