"""NumPy fp64 yardstick of the crowded-field fit (mpsfr_fit_frame_psf, include/mpsfr.h) and the scene the CPU and GPU
tests share.

solve() restates the contract with dense algebra: the accepted stars, the fit domain Omega by the disc rule (each
product rounded, then the sum), the design matrix A out of render_ref.window (one column per accepted star, one of ones
with the background), numpy.linalg.lstsq on the rows scaled by sqrt(w), and from N = A^T W A the diagonal, the overlap,
chi2, the conditional and the marginal errors.

The parity bounds (bounds()).  Notation: Dg = diag(N), y = Dg^(1/2) x, Ns = Dg^(-1/2) N Dg^(-1/2) with the eigenvalues
lmin .. lmax and kappa = lmax / lmin; |N|s the same out of |A|; u the unit roundoff, EPS = 2 u.
  convergence   The solver stops when |rs_k| <= tol |rs_0| for the scaled recurrence residual rs = Dg^(-1/2) r.  From a
                zero start rs_0 = Ns y*, and y_k - y* = Ns^-1 (Ns y_k - Ns y*), so |y_k - y*| <= kappa tol |y*|.
  recurrence    The true residual differs from the recurrence by the rounding of every product N p the loop forms.  One
                product is a render (at most L stars summed at a pixel, every P~ a 16-term FIR) and a projection (3600
                footprint pixels, every P~ the same FIR, a fixed tree): each entry a sum of at most NTERM = 3600 + L + 40
                terms, so between exact and computed |d(N p)| <= NTERM EPS |N| |p| entry by entry, as find_ref counts
                its sums.  Over k products (Greenbaum's estimate, first order) the gap is at most
                (k + 1) NTERM EPS ||N|s| max_j |y_j|; the norms of conjugate-gradient iterates from a zero start grow
                monotonically to |y*|, and 2 |y*| is taken for the computed ones.  Through Ns^-1: / lmin.  k = max_iter.
  right side    rs_0 itself: |d(A^T W D)| <= NTERM EPS |A|^T W |D|, scaled and through Ns^-1.
  reference     lstsq is backward stable: its own error is of the order n EPS (kappa_A + kappa_A^2 |res| / (smax |x|));
                in the scaled variables that is at most 8 n EPS (sqrt(kappa) |y*| + kappa |sqrt(w) res| / sqrt(lmax)).
The bound of y is the sum of the four, in the 2-norm over all unknowns.  F_k alone is within bound / sqrt(N_kk).
  N_kk          a sum of at most NTERM terms that are not negative: relative NTERM EPS.
  overlap       (q_k - N_kk) / N_kk with q = N 1 by one render and one projection: |dq_k| <= NTERM EPS (|N| 1)_k, so the
                absolute bound is 2 NTERM EPS ((|N| 1)_k / N_kk + 1 + |overlap_k|) (the 2 for the second order).
  chi2          chi2(y) - chi2(y*) = |y - y*|^2 in the Ns norm (the gradient vanishes at y*): at most lmax bound_y^2;
                the residual frame carries |dR| <= (L + 20) EPS S per pixel, S = |D| + sum |F| |P~| + |b|, and the sum over
                Omega (|Omega| + 4) EPS chi2: 2 sqrt(chi2 sum w dR^2) + sum w dR^2 + (|Omega| + 4) EPS chi2.
None of these is fitted to what the GPU gives.

solve_sparse() is solve() with a sparse design matrix, for thousands of stars or millions of pixels; it solves the normal
equations with refinement, and bounds() then takes its a-posteriori 'ref_err' for the reference term (its docstring).
"""
import numpy as np

import render_ref as Y

NS = Y.NS
APRON = Y.APRON
EPS = float(np.finfo(np.float64).eps)
MAX_SHIFT = 8.0
MAX_ORIGIN = 1 << 30
FRAME = (97, 150)
SKY = 7.0


def centre(origin, shift):
    """c = (double)(origin + 20) + shift per axis: one rounding."""
    o = np.asarray(origin, dtype=np.int64)
    s = np.zeros(2) if shift is None else np.asarray(shift, dtype=np.float64)
    return float(o[0] + NS // 2) + float(s[0]), float(o[1] + NS // 2) + float(s[1])


def valid_pixels(image, var):
    """The observed fits' rule: the datum finite, var finite and > 0 (None: every finite datum)."""
    ok = np.isfinite(image)
    if var is not None:
        with np.errstate(invalid='ignore'):
            ok = ok & np.isfinite(var) & (var > 0)
    return ok


def disc(shape, c, radius):
    """The boolean frame of dy dy + dx dx <= radius radius, each product rounded, then the sum (NumPy does not fuse)."""
    ny, nx = shape
    dy = (np.arange(ny, dtype=np.float64) - c[0])[:, None]
    dx = (np.arange(nx, dtype=np.float64) - c[1])[None, :]
    a, b = dy * dy, dx * dx
    return a + b <= np.float64(radius) * np.float64(radius)


def column(shape, P, origin, shift):
    """P~ of one star on the frame (zeros outside its footprint), or None if the footprint misses the frame."""
    y0, y1, x0, x1 = Y.footprint(shape, origin)
    if y0 >= y1 or x0 >= x1:
        return None
    dp, dq = (0.0, 0.0) if shift is None else shift
    w = Y.window(P, dp, dq)
    wy, wx = y0 - (int(origin[0]) - APRON), x0 - (int(origin[1]) - APRON)
    out = np.zeros(shape)
    out[y0:y1, x0:x1] = w[wy:wy + y1 - y0, wx:wx + x1 - x0]
    return out


def solve(image, var, psf, index, origin, shift, radius, background):
    """The fit as the header states it.  Returns a dict: status, F, err, flux, err_flux, overlap, ndisc, nkk (per star,
    zeros for the stars left out), sigma (the marginal error sqrt(N^-1_kk), var taken as the true variance), b, err_b,
    chi2, nomega, nacc, head_status, resid (image - sum F P~), omega, and the matrices the bounds need."""
    image = np.asarray(image, dtype=np.float64)
    shape = image.shape
    n = len(origin)
    ok = valid_pixels(image, var)
    w = np.where(ok, 1.0 / np.where(ok, 1.0 if var is None else var, 1.0), 0.0)
    status = np.zeros(n, dtype=int)
    ndisc = np.zeros(n)
    cols, discs = {}, {}
    for k in range(n):
        ix = k if index is None else int(index[k])
        sh = None if shift is None else shift[k]
        fine = 0 <= ix < len(psf) and np.all(np.abs(origin[k]) <= MAX_ORIGIN) and \
            (sh is None or bool(np.all(np.abs(sh) <= MAX_SHIFT)))
        if not fine:
            status[k] = 2
            continue
        col = column(shape, psf[ix], origin[k], sh)
        if col is None:
            status[k] = 1
            continue
        dk = disc(shape, centre(origin[k], sh), radius) & ok
        own = float(np.sum(w[dk] * col[dk] ** 2))
        if dk.sum() == 0 or not (own > 0 and np.isfinite(own)):
            status[k] = 2
            continue
        ndisc[k] = dk.sum()
        cols[k], discs[k] = col, dk
    acc = sorted(cols)
    omega = np.zeros(shape, dtype=bool)
    for k in acc:
        omega |= discs[k]
    nomega, nacc = int(omega.sum()), len(acc)
    nunk = nacc + (1 if background else 0)
    out = dict(status=status, F=np.zeros(n), err=np.zeros(n), flux=np.zeros(n), err_flux=np.zeros(n),
               overlap=np.zeros(n), ndisc=np.zeros(n), nkk=np.zeros(n), sigma=np.zeros(n), b=0.0, err_b=0.0, chi2=0.0,
               nomega=nomega, nacc=nacc, omega=omega, acc=np.array(acc, dtype=int), resid=image.copy(), head_status=0)
    if nacc == 0 or nomega < nunk + 1:
        out['status'] = np.where(status == 1, 1, 2)
        out['head_status'] = 2
        return out
    A = np.stack([cols[k][omega] for k in acc] + ([np.ones(nomega)] if background else []), axis=1)
    wo, d = w[omega], image[omega]
    sw = np.sqrt(wo)
    x = np.linalg.lstsq(A * sw[:, None], d * sw, rcond=None)[0]
    N = A.T @ (A * wo[:, None])
    Nabs = np.abs(A).T @ (np.abs(A) * wo[:, None])
    dg = np.diag(N).copy()
    res = d - A @ x
    chi2 = float(np.sum(wo * res * res))
    s2 = chi2 / (nomega - nunk)
    cov = np.linalg.inv(N)
    sump = np.array([psf[k if index is None else int(index[k])].sum() for k in acc])
    F = x[:nacc]
    out['F'][acc] = F
    out['err'][acc] = np.sqrt(s2 / dg[:nacc])
    out['flux'][acc] = F * sump
    out['err_flux'][acc] = out['err'][acc] * np.abs(sump)
    out['overlap'][acc] = (N[:nacc, :nacc].sum(axis=1) - dg[:nacc]) / dg[:nacc]
    out['ndisc'][acc] = ndisc[acc]
    out['nkk'][acc] = dg[:nacc]
    out['sigma'][acc] = np.sqrt(np.diag(cov)[:nacc])
    if background:
        out['b'], out['err_b'] = float(x[nacc]), float(np.sqrt(s2 / dg[nacc]))
    out['chi2'] = chi2
    resid = image.copy()
    for i, k in enumerate(acc):
        resid = resid - F[i] * cols[k]
    out['resid'] = resid
    out.update(A=A, w=wo, d=d, x=x, N=N, Nabs=Nabs, dg=dg, res=res, background=background)
    return out


REFINE = 3


def solve_sparse(image, var, psf, index, origin, shift, radius, background):
    """solve() for thousands of stars or millions of pixels: the same contract and the same dict keys, with the design
    matrix A a scipy.sparse CSR matrix over Omega whose columns come from render_ref.window on each star's footprint
    (no per-star frame is kept; the disc lies inside the footprint, so the disc rule is evaluated there with the same
    operations).  N, Nabs and dg are dense, (nstar + 1)^2.

    x is not lstsq's: the scaled normal equations Ns y = Dg^(-1/2) A^T W D by numpy.linalg.solve, then REFINE rounds of
    refinement on the gradient g(x) = A^T W (D - A x).  Its error is accounted for a posteriori.  The gradient is
    linear, g(x) = N (x* - x), so Dg^(1/2) (x - x*) = Ns^-1 Dg^(-1/2) g(x) and |y - y*| <= |Dg^(-1/2) g(x)| / lmin for
    the exact gradient at the x returned.  The computed gradient differs from the exact one by rounding: the residual
    of a pixel, a sum of at most L + 1 products, by (L + 3) EPS (|D| + |A| |x|) =: dres, and entry k of the projection,
    a sum of at most m terms (m the longest column), by (m + 3) EPS (|A|^T W |res|)_k + (|A|^T W dres)_k.  'ref_err' is
    (|Dg^(-1/2) g| + |Dg^(-1/2) dg|) / lmin in the 2-norm: the term bounds() takes in place of lstsq's."""
    import scipy.sparse as sp
    image = np.asarray(image, dtype=np.float64)
    shape = image.shape
    ny, nx = shape
    n = len(origin)
    ok = valid_pixels(image, var)
    w = np.where(ok, 1.0 / np.where(ok, 1.0 if var is None else var, 1.0), 0.0)
    status = np.zeros(n, dtype=int)
    ndisc = np.zeros(n)
    wins, omega = {}, np.zeros(shape, dtype=bool)
    r2 = np.float64(radius) * np.float64(radius)
    for k in range(n):
        ix = k if index is None else int(index[k])
        sh = None if shift is None else shift[k]
        fine = 0 <= ix < len(psf) and np.all(np.abs(origin[k]) <= MAX_ORIGIN) and \
            (sh is None or bool(np.all(np.abs(sh) <= MAX_SHIFT)))
        if not fine:
            status[k] = 2
            continue
        y0, y1, x0, x1 = Y.footprint(shape, origin[k])
        if y0 >= y1 or x0 >= x1:
            status[k] = 1
            continue
        dp, dq = (0.0, 0.0) if sh is None else sh
        win = Y.window(psf[ix], dp, dq)
        wy, wx = y0 - (int(origin[k][0]) - APRON), x0 - (int(origin[k][1]) - APRON)
        col = win[wy:wy + y1 - y0, wx:wx + x1 - x0]
        c = centre(origin[k], sh)
        dy = (np.arange(y0, y1, dtype=np.float64) - c[0])[:, None]
        dx = (np.arange(x0, x1, dtype=np.float64) - c[1])[None, :]
        a, b = dy * dy, dx * dx
        dk = (a + b <= r2) & ok[y0:y1, x0:x1]
        own = float(np.sum(w[y0:y1, x0:x1][dk] * col[dk] ** 2))
        if dk.sum() == 0 or not (own > 0 and np.isfinite(own)):
            status[k] = 2
            continue
        ndisc[k] = dk.sum()
        wins[k] = (y0, y1, x0, x1, col)
        omega[y0:y1, x0:x1] |= dk
    acc = sorted(wins)
    nomega, nacc = int(omega.sum()), len(acc)
    nunk = nacc + (1 if background else 0)
    out = dict(status=status, F=np.zeros(n), err=np.zeros(n), flux=np.zeros(n), err_flux=np.zeros(n),
               overlap=np.zeros(n), ndisc=np.zeros(n), nkk=np.zeros(n), sigma=np.zeros(n), b=0.0, err_b=0.0, chi2=0.0,
               nomega=nomega, nacc=nacc, omega=omega, acc=np.array(acc, dtype=int), resid=image.copy(), head_status=0)
    if nacc == 0 or nomega < nunk + 1:
        out['status'] = np.where(status == 1, 1, 2)
        out['head_status'] = 2
        return out
    place = np.full(shape, -1, dtype=np.int64)
    place[omega] = np.arange(nomega)                       # (boolean indexing runs in pixel order, as A[omega] does)
    ri, ci, vals = [], [], []
    for j, k in enumerate(acc):
        y0, y1, x0, x1, col = wins[k]
        p = place[y0:y1, x0:x1]
        on = (p >= 0) & (col != 0.0)
        ri.append(p[on])
        ci.append(np.full(int(on.sum()), j, dtype=np.int64))
        vals.append(col[on])
    if background:
        ri.append(np.arange(nomega))
        ci.append(np.full(nomega, nacc, dtype=np.int64))
        vals.append(np.ones(nomega))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(ri), np.concatenate(ci))), shape=(nomega, nunk))
    Aabs = abs(A)
    wo, d = w[omega], image[omega]
    W = sp.diags(wo)
    N = np.asarray((A.T @ W @ A).todense())
    Nabs = np.asarray((Aabs.T @ W @ Aabs).todense())
    dg = np.diag(N).copy()
    s = 1.0 / np.sqrt(dg)
    Ns = N * s[:, None] * s[None, :]
    x = np.zeros(nunk)
    for _ in range(1 + REFINE):
        g = A.T @ (wo * (d - A @ x))
        x = x + s * np.linalg.solve(Ns, s * g)
    res = d - A @ x
    g = A.T @ (wo * res)
    L = int(np.max(np.diff(A[:, :nacc].tocsr().indptr)))
    m = int(np.max(np.diff(A.tocsc().indptr)))
    dres = (L + 3) * EPS * (np.abs(d) + Aabs @ np.abs(x))
    dgrad = (m + 3) * EPS * (Aabs.T @ (wo * np.abs(res))) + Aabs.T @ (wo * dres)
    lmin = float(np.linalg.eigvalsh(Ns)[0])
    ref_err = (float(np.linalg.norm(s * g)) + float(np.linalg.norm(s * dgrad))) / lmin
    chi2 = float(np.sum(wo * res * res))
    s2 = chi2 / (nomega - nunk)
    cov = np.linalg.inv(N)
    sump = np.array([psf[k if index is None else int(index[k])].sum() for k in acc])
    F = x[:nacc]
    out['F'][acc] = F
    out['err'][acc] = np.sqrt(s2 / dg[:nacc])
    out['flux'][acc] = F * sump
    out['err_flux'][acc] = out['err'][acc] * np.abs(sump)
    out['overlap'][acc] = (N[:nacc, :nacc].sum(axis=1) - dg[:nacc]) / dg[:nacc]
    out['ndisc'][acc] = ndisc[acc]
    out['nkk'][acc] = dg[:nacc]
    out['sigma'][acc] = np.sqrt(np.diag(cov)[:nacc])
    if background:
        out['b'], out['err_b'] = float(x[nacc]), float(np.sqrt(s2 / dg[nacc]))
    out['chi2'] = chi2
    resid = image.copy()
    for i, k in enumerate(acc):
        y0, y1, x0, x1, col = wins[k]
        resid[y0:y1, x0:x1] = resid[y0:y1, x0:x1] - F[i] * col
    out['resid'] = resid
    out.update(A=A, w=wo, d=d, x=x, N=N, Nabs=Nabs, dg=dg, res=res, background=background, sparse=True, L=L,
               ref_err=ref_err)
    return out


def scaled(ref):
    """(Ns, |N|s, y*) of the docstring."""
    s = 1.0 / np.sqrt(ref['dg'])
    return ref['N'] * s[:, None] * s[None, :], ref['Nabs'] * s[:, None] * s[None, :], ref['x'] * np.sqrt(ref['dg'])


def bounds(ref, tol, max_iter):
    """The a-priori bounds of the docstring for a solve from a zero start: dict(y, kappa, nkk_rel, overlap (per accepted
    star), chi2, terms (the four parts of y)).  Of a solve_sparse() result the `reference` term is not lstsq's but the
    a-posteriori 'ref_err' derived in its docstring; the three other terms and every other bound are the same
    expressions on the sparse A."""
    A, wo, d = ref['A'], ref['w'], ref['d']
    nacc = ref['nacc']
    sparse = bool(ref.get('sparse'))
    Aabs = abs(A) if sparse else np.abs(A)
    Ns, Nsabs, ys = scaled(ref)
    ev = np.linalg.eigvalsh(Ns)
    lmin, lmax = float(ev[0]), float(ev[-1])
    kappa = lmax / lmin
    mu = float(np.linalg.norm(Nsabs, 2))
    ynorm = float(np.linalg.norm(ys))
    L = ref['L'] if sparse else int(np.max(np.count_nonzero(A[:, :nacc], axis=1)))
    g = (NS + 2 * APRON) ** 2 + L + 40
    conv = kappa * tol * ynorm
    gap = (max_iter + 1) * g * EPS * mu * 2.0 * ynorm / lmin
    rhs = g * EPS * float(np.linalg.norm((Aabs.T @ (wo * np.abs(d))) / np.sqrt(ref['dg']))) / lmin
    if sparse:
        lsq = ref['ref_err']
    else:
        wres = float(np.sqrt(np.sum(wo * ref['res'] ** 2)))
        lsq = 8 * len(ys) * EPS * (np.sqrt(kappa) * ynorm + kappa * wres / np.sqrt(lmax))
    by = conv + gap + rhs + lsq
    dg = ref['dg'][:nacc]
    ovl = (ref['N'][:nacc, :nacc].sum(axis=1) - dg) / dg
    b_ovl = 2 * g * EPS * (ref['Nabs'][:nacc, :nacc].sum(axis=1) / dg + 1.0 + np.abs(ovl))
    S = np.abs(d) + Aabs @ np.abs(ref['x'])
    dR = (L + 20) * EPS * S
    sdr = float(np.sum(wo * dR * dR))
    b_chi2 = lmax * by * by + 2.0 * np.sqrt(ref['chi2'] * sdr) + sdr + (len(d) + 4) * EPS * ref['chi2']
    return dict(y=by, kappa=kappa, nkk_rel=g * EPS, overlap=b_ovl, chi2=b_chi2, terms=(conv, gap, rhs, lsq), lmax=lmax,
                lmin=lmin)


def pcg(ref, tol, max_iter, x0=None):
    """The textbook iteration the header describes, on the dense N: (x, iterations, relative residual).  Only used to
    know how many steps a tolerance asks for."""
    N, dg = ref['N'], ref['dg']
    rhs = ref['A'].T @ (ref['w'] * ref['d'])
    x = np.zeros(len(dg)) if x0 is None else np.array(x0, dtype=float)
    r = rhs - N @ x
    z = r / dg
    p = z.copy()
    rho0 = rho = float(r @ z)
    if rho0 == 0:
        return x, 0, 0.0
    for it in range(1, max_iter + 1):
        q = N @ p
        alpha = rho / float(p @ q)
        x = x + alpha * p
        r = r - alpha * q
        z = r / dg
        rho1 = float(r @ z)
        if rho1 <= tol * tol * rho0:
            return x, it, np.sqrt(rho1 / rho0)
        p = z + (rho1 / rho) * p
        rho = rho1
    return x, max_iter, np.sqrt(rho / rho0)


CHAIN = 7
_SCENE = {}


def scene(noise=True):
    """The shared scene on the 97 x 150 frame (no multiple of the 32-pixel tile), the four models of render_ref by
    k % 4: a chain of 7 stars at a pitch of (0.3, 3.0) px, three stars within 2 px of each other, 20 at random, one
    centred 3 px above the top edge, one in the bottom-right corner, one wholly off the frame (status 1) and one whose
    disc is all NaN (status 2; the frame holds no light of it).  Fluxes 200 .. 5000, sky 7, var = 4 + model / 2,
    Gaussian noise of that variance, 1 % NaN pixels; default_rng(5).  noise=False: the same scene without noise and
    without sky.  Returns a dict."""
    if noise in _SCENE:
        return _SCENE[noise]
    rng = np.random.default_rng(5)
    ny, nx = FRAME
    pos = [(30.0 + 0.3 * i, 20.0 + 3.0 * i) for i in range(CHAIN)]
    pos += [(60.2, 40.1), (61.3, 41.0), (60.0, 41.7)]
    pos += [(float(a), float(b)) for a, b in zip(rng.uniform(4, ny - 4, 20), rng.uniform(4, nx - 4, 20))]
    pos += [(-3.0, 75.3), (95.6, 148.7), (-80.0, 30.0), (14.2, 131.4)]
    pos = np.array(pos)
    n = len(pos)
    top, corner, off, dark = n - 4, n - 3, n - 2, n - 1
    flux = rng.uniform(200, 5000, n)
    flux[dark] = 200.0
    origin = (np.rint(pos) - NS // 2).astype(np.int32)
    shift = pos - (origin + NS // 2)
    index = (np.arange(n) % 4).astype(np.int32)
    psf = Y.models()
    lit = np.arange(n) != dark               # (the masked star's light is left out: the truth stays exact)
    model, _, _ = Y.render(None, psf, index[lit], origin[lit], shift[lit], flux[lit], shape=FRAME)
    var = 4.0 + model / 2.0
    gauss = rng.normal(size=FRAME)
    image = model + (SKY + gauss * np.sqrt(var) if noise else 0.0)
    image[rng.uniform(size=FRAME) < 0.01] = np.nan
    cy, cx = int(round(pos[dark][0])), int(round(pos[dark][1]))
    image[max(cy - 10, 0):cy + 11, max(cx - 10, 0):cx + 11] = np.nan
    s = dict(image=image, var=var, psf=psf, index=index, origin=origin, shift=shift, pos=pos, flux=flux, n=n,
             chain=np.arange(CHAIN), triple=np.arange(CHAIN, CHAIN + 3), top=top, corner=corner, off=off, dark=dark)
    _SCENE[noise] = s
    return s


_REF = {}


def scene_reference(with_var, background, radius, noise=True):
    """solve() of the scene, computed once per case."""
    key = (with_var, background, radius, noise)
    if key not in _REF:
        s = scene(noise)
        _REF[key] = solve(s['image'], s['var'] if with_var else None, s['psf'], s['index'], s['origin'], s['shift'],
                          radius, background)
    return _REF[key]


LOOP_FRAME = (160, 200)
LOOP_CRIT = 6.0
LOOP_CHAIN = 6
LOOP_FIND = dict(half=2, sep=2, threshold=5.0)       # a 5 x 5 core resolves stars 4 pixels apart at FWHM 3.5 (group_ref)


def loop_field():
    """The field of the chain find -> fit -> subtract -> find: 38 stars of find_ref's model on 160 x 200 -- a chain of 6
    at a pitch of 5 px (one group at crit 6: oversize), 4 pairs 5 px apart and 24 singles, one to a cell of a 30-pixel
    grid --, for a background of 5 with unit-variance noise.  Returns (positions (38, 2), fluxes (38,), the chain's
    indices)."""
    rng = np.random.default_rng(11)
    cells = [(15 + 30 * i, 15 + 30 * j) for i in range(5) for j in range(6)]
    pos = [(cells[0][0] + 0.3 * k + rng.uniform(-0.2, 0.2), cells[0][1] - 5.0 + 5.0 * k + rng.uniform(-0.2, 0.2))
           for k in range(LOOP_CHAIN)]
    for n, c in enumerate(cells[2:]):           # (the chain runs through the first two cells of the first row)
        y, x = c[0] + rng.uniform(-3, 3), c[1] + rng.uniform(-3, 3)
        pos.append((y, x))
        if n % 7 == 3:
            pos.append((y + 3.0, x + 4.0))
    pos = np.array(pos)
    flux = rng.uniform(600.0, 1500.0, len(pos))
    return pos, flux, np.arange(LOOP_CHAIN)


def loop_background():
    return 5.0 + np.random.default_rng(12).normal(size=LOOP_FRAME)
