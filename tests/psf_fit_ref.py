"""NumPy / SciPy yardstick of the PSF-model fit of observed stars (mpsfr_fit_stamps_psf, include/mpsfr.h), and the
noisy, masked stars the CPU and GPU tests share.

Model: m(p, q) = F P~(p - dp, q - dq) + b with P~(y, x) = sum_kl c(y - k) c(x - l) P[k][l], c the Keys cubic-convolution
kernel (a = -1/2) and P zero outside its 40 x 40 pixels; v = (F, dp, dq, b).  The fit minimises
sum_used (m - d)^2 / var over the free variables (no background: b = 0 fixed; fixed shift: dp, dq fixed, a linear
problem solved in closed form) with scipy's least_squares ('lm') and the analytic Jacobian, followed by Gauss-Newton
steps in fp64 until the step is below 1e-10 of the formal error; residuals carry the weight 1 / sqrt(var), excluded
pixels the weight 0.  Errors: sqrt(diag((J^T W J)^-1) chi2 / dof), dof = n_used - npar.
"""
import os

import numpy as np

NS = 40
MAX_SHIFT = 8.0
VARIANTS = ((False, False), (True, False), (False, True), (True, True))     # (background, fixed shift)
KEYS = ('F', 'dp', 'dq', 'back')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def keys(t):
    """The Keys kernel c(t), a = -1/2."""
    a = np.abs(t)
    return np.where(a <= 1, (1.5 * a - 2.5) * a * a + 1, np.where(a < 2, ((-0.5 * a + 2.5) * a - 4) * a + 2, 0.0))


def dkeys(t):
    """c'(t)."""
    a = np.abs(t)
    return np.sign(t) * np.where(a <= 1, (4.5 * a - 5) * a, np.where(a < 2, (-1.5 * a + 5) * a - 4, 0.0))


def tap_matrix(d):
    """W[p, k] = c(p - d - k) and its derivative with respect to the sample position y = p - d:
    P~(p - d) = sum_k W[p, k] P[k]."""
    t = np.arange(NS)[:, None] - d - np.arange(NS)[None, :]
    return keys(t), dkeys(t)


def resample(psf, dp, dq):
    """P~(p - dp, q - dq) on the 40 x 40 pixels."""
    return tap_matrix(dp)[0] @ psf @ tap_matrix(dq)[0].T


def model(psf, v, jac=False):
    """m on the stamp; with jac also dm/d(F, dp, dq, b), shape (40, 40, 4)."""
    F, dp, dq, b = v
    wy, dwy = tap_matrix(dp)
    wx, dwx = tap_matrix(dq)
    s = wy @ psf @ wx.T
    m = F * s + b
    if not jac:
        return m
    return m, np.stack([s, -F * (dwy @ psf @ wx.T), -F * (wy @ psf @ dwx.T), np.ones_like(s)], axis=-1)


def used_pixels(data, var=None):
    d = np.asarray(data, dtype=float)
    ok = np.isfinite(d)
    if var is not None:
        va = np.asarray(var, dtype=float)
        with np.errstate(invalid='ignore'):
            ok &= np.isfinite(va) & (va > 0)
    return ok


def free_indices(back, fixed):
    return [0] + ([] if fixed else [1, 2]) + ([3] if back else [])


def _weights(data, var):
    ok = used_pixels(data, var)
    va = np.ones((NS, NS)) if var is None else np.asarray(var, dtype=float)
    sw = np.where(ok, 1.0 / np.sqrt(np.where(ok, va, 1.0)), 0.0)
    return ok, sw, np.where(ok, data, 0.0)


def linear_solve(data, var, psf, dp, dq, back):
    """Closed-form weighted least squares for (F, b) at the shift (dp, dq): (F, b), b = 0 without a background."""
    ok, sw, dd = _weights(np.asarray(data, dtype=float), var)
    cols = [resample(psf, dp, dq).ravel()] + ([np.ones(NS * NS)] if back else [])
    A = np.stack(cols, axis=1) * sw.ravel()[:, None]
    sol = np.linalg.lstsq(A, (dd * sw).ravel(), rcond=None)[0]
    return float(sol[0]), float(sol[1]) if back else 0.0


def start(data, var, psf, back, shift=None):
    """The start values of the definition: the given shift, or argmax over the used pixels of the star minus argmax of
    the model stamp (first maxima in C order) brought into the domain; F and b from the linear solve there."""
    data = np.asarray(data, dtype=float)
    if shift is None:
        ok = used_pixels(data, var)
        ks = int(np.argmax(np.where(ok, np.where(ok, data, 0.0), -np.inf)))
        kp = int(np.argmax(psf))
        dp = float(np.clip(ks // NS - kp // NS, -MAX_SHIFT, MAX_SHIFT))
        dq = float(np.clip(ks % NS - kp % NS, -MAX_SHIFT, MAX_SHIFT))
    else:
        dp, dq = float(shift[0]), float(shift[1])
    F, b = linear_solve(data, var, psf, dp, dq, back)
    return np.array([F, dp, dq, b])


def fit(data, var, psf, back, fixed=False, shift=None, v0=None):
    """Weighted least-squares fit of one star.  Returns a dict: x (4 variables), err (formal errors of the free
    variables, 0 for fixed ones), chi2, npix, nfev, status (scipy's; 0 for the linear problem)."""
    from scipy.optimize import least_squares
    data = np.asarray(data, dtype=float).reshape(NS, NS)
    psf = np.asarray(psf, dtype=float).reshape(NS, NS)
    ok, sw, dd = _weights(data, var)
    free = free_indices(back, fixed)
    full = np.array(start(data, var, psf, back, shift) if v0 is None else v0, dtype=float)
    if not back:
        full[3] = 0.0

    def ex(x):
        v = full.copy()
        v[free] = x
        return v

    def res(x):
        return ((model(psf, ex(x)) - dd) * sw).ravel()

    def jac(x):
        return (model(psf, ex(x), True)[1] * sw[..., None]).reshape(-1, 4)[:, free]

    x, nfev, status = full[free], 0, 0
    if not fixed:
        r = least_squares(res, x, jac=jac, method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
        x, nfev, status = r.x, r.nfev, r.status
    npix = int(ok.sum())
    dof = npix - len(free)
    for _ in range(40):                         # Gauss-Newton to the bottom (the linear problem: exact after one)
        J, rr = jac(x), res(x)
        dx = -np.linalg.lstsq(J, rr, rcond=None)[0]
        x = x + dx
        cov = np.linalg.inv(J.T @ J) * float(rr @ rr) / dof
        if np.all(np.abs(dx) <= 1e-10 * np.sqrt(np.diag(cov))) or float(rr @ rr) == 0.0:
            break
    J = jac(x)
    chi2 = float((res(x) ** 2).sum())
    cov = np.linalg.inv(J.T @ J) * chi2 / dof
    err = np.zeros(4)
    err[free] = np.sqrt(np.diag(cov))
    return dict(x=ex(x), err=err, chi2=chi2, npix=npix, nfev=nfev, status=status, free=free)


def gpu_values(row):
    """(F, dp, dq, back) and their errors from a library row (NFIT_PSF)."""
    return np.array(row[0:4]), np.array(row[6:10])


def moffat(p0, q0, fwhm, n, peak=1.0):
    a = fwhm / (2 * np.sqrt(2 ** (1 / n) - 1))
    p, q = np.mgrid[:NS, :NS]
    return peak * (1 + ((p - p0) ** 2 + (q - q0) ** 2) / a ** 2) ** -n


def golden_stamps():
    g = np.load(os.path.join(GOLDEN, 'g9_profile.npz'))
    return np.concatenate([g['a_fin'], g['b_fin'], g['c_fin']]).reshape(-1, NS, NS)


_STARS = {}


def noisy_stars(back, count=24, seed=11):
    """`count` observed stars with their model stamps: two of three are Moffat PSFs (FWHM 2.2 / 3 / 5 / 8 px in turn,
    n 1.8 - 4, sum 1, centred on a pixel or between four) whose star is the analytic Moffat at the shifted centre -- the
    model is then only nearly right, as for a real star --, every third a g9_profile golden stamp whose star is the
    resampled stamp itself.  True shifts within +-3 px, F 50 - 5000, a background of -1 ... 5 % of the peak when
    `back`, noise of 2 % of the peak with a signal term, 3 % of the pixels NaN, one 3 x 3 block of var = 0 and two
    pixels of var < 0.  Returns (data, var, psf, truth): (count, 40, 40) three times and (count, 4)."""
    if (back, count, seed) in _STARS:
        return _STARS[back, count, seed]
    rng = np.random.default_rng([seed, int(back)])
    gold = golden_stamps()
    data, var, psfs, truth = [], [], [], []
    for k in range(count):
        dp, dq = rng.uniform(-3, 3, 2)
        F = rng.uniform(50, 5000)
        if k % 3 == 2:
            psf = gold[rng.integers(len(gold))]
            star = F * resample(psf, dp, dq)
        else:
            fw, n = (2.2, 3.0, 5.0, 8.0)[(k // 3) % 4], rng.uniform(1.8, 4)
            c0 = 20.0 - 0.5 * (k % 2)
            norm = moffat(c0, c0, fw, n).sum()
            psf = moffat(c0, c0, fw, n) / norm
            star = F * moffat(c0 + dp, c0 + dq, fw, n) / norm
        peak = star.max()
        b = rng.uniform(-0.01, 0.05) * peak if back else 0.0
        va = (0.02 * peak) ** 2 * (0.05 + np.abs(star) / peak)
        d = star + b + rng.normal(size=star.shape) * np.sqrt(va)
        d[rng.uniform(size=star.shape) < 0.03] = np.nan
        i, j = rng.integers(3, 34, 2)
        va[i:i + 3, j:j + 3] = 0.0
        va[rng.integers(0, NS, 2), rng.integers(0, NS, 2)] = -1.0
        data.append(d)
        var.append(va)
        psfs.append(psf)
        truth.append([F, dp, dq, b])
    _STARS[back, count, seed] = tuple(np.array(a) for a in (data, var, psfs, truth))
    return _STARS[back, count, seed]


_YARD = {}


def yardstick(back, fixed):
    """(data, var, psf, truth, shift, fits) of one variant on the shared stars, computed once.  The fixed-shift
    variants hold the true shift rounded to 1/8 px."""
    if (back, fixed) not in _YARD:
        data, var, psf, truth = noisy_stars(back)
        shift = np.round(truth[:, 1:3] * 8) / 8 if fixed else None
        fits = [fit(d, va, p, back, fixed, None if shift is None else shift[k])
                for k, (d, va, p) in enumerate(zip(data, var, psf))]
        _YARD[back, fixed] = (data, var, psf, truth, shift, fits)
    return _YARD[back, fixed]
