"""NumPy / SciPy yardstick of the PSF-model fit of blended stars (mpsfr_fit_groups_psf, include/mpsfr.h), and the noisy,
masked groups the CPU and GPU tests share.  The resampling, the weights and the single-star yardstick are those of
tests/psf_fit_ref.py.

Model: m(p, q) = sum_k F_k P~(p - dp_k, q - dq_k) + b over the K sources of a stamp, one model stamp P.  Variables x:
    'free'    (F_0, dp_0, dq_0, F_1, dp_1, dq_1, ..., [b])
    'common'  (F_0 .. F_{K-1}, Dp, Dq, [b]),  dp_k = s_k,p + Dp, dq_k = s_k,q + Dq with s the given positions
    'fixed'   (F_0 .. F_{K-1}, [b]) at the given positions: linear
The fit starts from the closed-form weighted linear solve for (F_k, b) at the given positions, runs scipy's
least_squares ('lm') with the analytic Jacobian and then Gauss-Newton steps in fp64 until the step is below 1e-10 of
the formal error.  Errors and the correlation coefficients of the F_k: (J^T W J)^-1 chi2 / dof, dof = n_used - npar.
"""
import numpy as np

from psf_fit_ref import NS, _weights, golden_stamps, keys, moffat, resample, tap_matrix  # noqa: F401

MODES = ('free', 'common', 'fixed')
SIZES = (2, 3, 4)
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))       # fit_out[40 .. 45]
NGROUP = 12


def n_par(K, back, mode):
    return {'free': 3 * K, 'common': K + 2, 'fixed': K}[mode] + int(back)


def i_flux(K, mode):
    """Indices of the F_k in x."""
    return [3 * k if mode == 'free' else k for k in range(K)]


def unpack(x, pos0, back, mode):
    """(F (K), positions (K, 2), b) of the variables x."""
    pos0 = np.asarray(pos0, dtype=float)
    K = len(pos0)
    x = np.asarray(x, dtype=float)
    F = x[i_flux(K, mode)]
    if mode == 'free':
        pos = np.stack([x[1:3 * K:3], x[2:3 * K:3]], axis=1)
    elif mode == 'common':
        pos = pos0 + x[K:K + 2]
    else:
        pos = pos0.copy()
    return F, pos, (x[-1] if back else 0.0)


def model(psf, x, pos0, back, mode, jac=False):
    """m on the stamp; with jac also dm/dx, shape (40, 40, npar)."""
    F, pos, b = unpack(x, pos0, back, mode)
    K = len(F)
    m = np.full((NS, NS), float(b))
    J = np.zeros((NS, NS, n_par(K, back, mode)))
    for k in range(K):
        wy, dwy = tap_matrix(pos[k, 0])
        wx, dwx = tap_matrix(pos[k, 1])
        s = wy @ psf @ wx.T
        m += F[k] * s
        if not jac:
            continue
        gy, gx = -F[k] * (dwy @ psf @ wx.T), -F[k] * (wy @ psf @ dwx.T)
        if mode == 'free':
            J[..., 3 * k], J[..., 3 * k + 1], J[..., 3 * k + 2] = s, gy, gx
        else:
            J[..., k] = s
            if mode == 'common':
                J[..., K] += gy
                J[..., K + 1] += gx
    if back:
        J[..., -1] = 1.0
    return (m, J) if jac else m


def linear_solve(data, var, psf, pos, back):
    """Closed-form weighted least squares for (F_0 .. F_{K-1}, [b]) at the positions pos (K, 2): NumPy's lstsq and one
    step of refinement against its own rounding (the columns of the design matrix differ by two orders of magnitude in
    norm: unrefined, a background of 1e-3 of the peak carries a relative error of 4e-11)."""
    ok, sw, dd = _weights(np.asarray(data, dtype=float), var)
    cols = [resample(psf, p[0], p[1]).ravel() for p in pos] + ([np.ones(NS * NS)] if back else [])
    A = np.stack(cols, axis=1) * sw.ravel()[:, None]
    rhs = (dd * sw).ravel()
    sol = np.linalg.lstsq(A, rhs, rcond=None)[0]
    return sol + np.linalg.lstsq(A, rhs - A @ sol, rcond=None)[0]


def start(data, var, psf, pos0, back, mode):
    """The start values of the definition: the given positions (a common offset of 0), F_k and b from the linear
    solve there."""
    pos0 = np.asarray(pos0, dtype=float)
    K = len(pos0)
    sol = linear_solve(data, var, psf, pos0, back)
    x = np.zeros(n_par(K, back, mode))
    x[i_flux(K, mode)] = sol[:K]
    if mode == 'free':
        x[1:3 * K:3], x[2:3 * K:3] = pos0[:, 0], pos0[:, 1]
    if back:
        x[-1] = sol[K]
    return x


def fit(data, var, psf, pos0, back, mode, x0=None):
    """Weighted least-squares fit of one group.  Returns a dict: x, err (formal errors of x), F, pos, b, err_F,
    err_pos (K, 2; the error of the common offset for every source in 'common', 0 in 'fixed'), err_b, corr (K, K
    correlation coefficients of the F_k), chi2, npix, nfev, status (scipy's; 0 for the linear problem), cond (of the
    Marquardt-scaled normal matrix)."""
    from scipy.optimize import least_squares
    data = np.asarray(data, dtype=float).reshape(NS, NS)
    psf = np.asarray(psf, dtype=float).reshape(NS, NS)
    pos0 = np.asarray(pos0, dtype=float).reshape(-1, 2)
    K = len(pos0)
    ok, sw, dd = _weights(data, var)
    npar = n_par(K, back, mode)

    def res(x):
        return ((model(psf, x, pos0, back, mode) - dd) * sw).ravel()

    def jac(x):
        return (model(psf, x, pos0, back, mode, True)[1] * sw[..., None]).reshape(-1, npar)

    x = np.array(start(data, var, psf, pos0, back, mode) if x0 is None else x0, dtype=float)
    nfev, status = 0, 0
    if mode != 'fixed':
        r = least_squares(res, x, jac=jac, method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
        x, nfev, status = r.x, r.nfev, r.status
    npix = int(ok.sum())
    dof = npix - npar
    for _ in range(40):                         # Gauss-Newton to the bottom (the linear problem: exact after one)
        J, rr = jac(x), res(x)
        dx = -np.linalg.lstsq(J, rr, rcond=None)[0]
        x = x + dx
        cov = np.linalg.inv(J.T @ J) * float(rr @ rr) / dof
        if np.all(np.abs(dx) <= 1e-10 * np.sqrt(np.diag(cov))) or float(rr @ rr) == 0.0:
            break
    J = jac(x)
    chi2 = float((res(x) ** 2).sum())
    A = J.T @ J
    cov = np.linalg.inv(A) * chi2 / dof
    err = np.sqrt(np.diag(cov))
    d = np.sqrt(np.diag(A))
    F, pos, b = unpack(x, pos0, back, mode)
    iF = i_flux(K, mode)
    err_pos = np.zeros((K, 2))
    if mode == 'free':
        err_pos = np.stack([err[1:3 * K:3], err[2:3 * K:3]], axis=1)
    elif mode == 'common':
        err_pos[:] = err[K:K + 2]
    corr = cov[np.ix_(iF, iF)] / np.outer(err[iF], err[iF])
    return dict(x=x, err=err, F=F, pos=pos, b=b, err_F=err[iF], err_pos=err_pos, err_b=err[-1] if back else 0.0,
                corr=corr, chi2=chi2, npix=npix, nfev=nfev, status=status, cond=float(np.linalg.cond(A / np.outer(d, d))))


def gpu_values(row, K, back, mode):
    """(x, err) in the yardstick's layout from a library row (NFIT_GROUP)."""
    row = np.asarray(row)
    src = row[8:8 + 8 * K].reshape(K, 8)
    if mode == 'free':
        x, e = src[:, 0:3].ravel(), src[:, 3:6].ravel()
    elif mode == 'common':
        x, e = np.concatenate([src[:, 0], [np.nan, np.nan]]), np.concatenate([src[:, 3], src[0, 4:6]])
    else:
        x, e = src[:, 0].copy(), src[:, 3].copy()
    if back:
        x, e = np.append(x, row[0]), np.append(e, row[1])
    return x, e


def gpu_corr(row, K):
    c = np.eye(K)
    for n, (i, j) in enumerate(PAIRS):
        if j < K:
            c[i, j] = c[j, i] = row[40 + n]
    return c


def _fwhm_px(psf):
    """FWHM of a stamp from the number of pixels above half its maximum."""
    return 2.0 * np.sqrt((psf > 0.5 * psf.max()).sum() / np.pi)


_GROUPS = {}


def groups(K, back):
    """12 blended groups of K sources with their model stamps: Moffat PSFs (FWHM 2.2 / 3 / 5 px in turn, n 1.8 - 4, sum
    1, centred on a pixel or between four) whose stars are the analytic Moffats at the shifted centres -- the model is
    then only nearly right --; every fourth group a g9_profile golden stamp whose blend is the resampled stamp itself.
    Positions within +-6 px per axis, the smallest pair separation >= 0.8 FWHM; F_0 500 - 5000, the others F_0 x (0.1 ..
    1); a background of -1 ... 5 % of the blend's peak when `back`; noise (0.02 peak)^2 (0.05 + |star| / peak); 3 % of
    the pixels NaN and one 3 x 3 block of var = 0.  Returns (data, var, psf, F, pos, b): (12, 40, 40) three times,
    (12, K), (12, K, 2), (12,)."""
    if (K, back) in _GROUPS:
        return _GROUPS[K, back]
    rng = np.random.default_rng([5, K, int(back)])
    gold = golden_stamps()
    data, var, psfs, Fs, poss, bs = [], [], [], [], [], []
    for g in range(NGROUP):
        exact = g % 4 == 3
        if exact:
            psf = gold[rng.integers(len(gold))]
            fw = _fwhm_px(psf)
        else:
            fw, n = (2.2, 3.0, 5.0)[g % 3], rng.uniform(1.8, 4)
            c0 = 20.0 - 0.5 * (g % 2)
            norm = moffat(c0, c0, fw, n).sum()
            psf = moffat(c0, c0, fw, n) / norm
        while True:
            pos = rng.uniform(-6, 6, (K, 2))
            sep = [np.hypot(*(pos[i] - pos[j])) for i in range(K) for j in range(i)]
            if min(sep) >= 0.8 * fw:
                break
        F = rng.uniform(500, 5000) * np.concatenate([[1.0], rng.uniform(0.1, 1.0, K - 1)])
        if exact:
            star = sum(f * resample(psf, p[0], p[1]) for f, p in zip(F, pos))
        else:
            star = sum(f * moffat(c0 + p[0], c0 + p[1], fw, n) / norm for f, p in zip(F, pos))
        peak = star.max()
        b = rng.uniform(-0.01, 0.05) * peak if back else 0.0
        va = (0.02 * peak) ** 2 * (0.05 + np.abs(star) / peak)
        d = star + b + rng.normal(size=star.shape) * np.sqrt(va)
        d[rng.uniform(size=star.shape) < 0.03] = np.nan
        i, j = rng.integers(3, 34, 2)
        va[i:i + 3, j:j + 3] = 0.0
        for a, v in zip((data, var, psfs, Fs, poss, bs), (d, va, psf, F, pos, b)):
            a.append(v)
    _GROUPS[K, back] = tuple(np.array(a) for a in (data, var, psfs, Fs, poss, bs))
    return _GROUPS[K, back]


def given_positions(pos, mode):
    """The positions handed to the fit: 'free' the true ones rounded to 1/2 px (start values), 'common' rounded to 1/8
    px plus (0.25, -0.25) (a catalogue with an offset), 'fixed' rounded to 1/8 px."""
    if mode == 'free':
        return np.round(pos * 2) / 2
    return np.round(pos * 8) / 8 + (np.array([0.25, -0.25]) if mode == 'common' else 0.0)


_YARD = {}


def yardstick(K, back, mode):
    """(data, var, psf, F, pos, b, given, fits) of one (K, back, mode) on the shared groups, computed once."""
    if (K, back, mode) not in _YARD:
        data, var, psf, F, pos, b = groups(K, back)
        given = given_positions(pos, mode)
        fits = [fit(d, va, p, s, back, mode) for d, va, p, s in zip(data, var, psf, given)]
        _YARD[K, back, mode] = (data, var, psf, F, pos, b, given, fits)
    return _YARD[K, back, mode]
