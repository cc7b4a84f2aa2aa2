"""NumPy / SciPy yardstick of the weighted Moffat fit of observed stars (mpsfr_fit_stamps_observed, include/mpsfr.h),
and the noisy, masked stamps the CPU and GPU tests share.

Model: moffat_ell_ref.model plus a constant background, v = (I, p0, q0, w, e1, e2, eta, b).  The fit minimises
sum_used (model - data)^2 / var over a subset of free variables (circular: e1 = e2 = 0 fixed; no background: b = 0
fixed) with scipy's least_squares and the analytic Jacobian; residuals carry the weight 1 / sqrt(var), excluded pixels
the weight 0.  Errors: sqrt(diag((J^T W J)^-1) chi2 / dof), dof = n_used - npar; those of derived values (FWHM axes,
n, rot) by first-order propagation through central differences of derived().
"""
import numpy as np

import moffat_ell_ref as M

NS = M.NS
VARIANTS = ((False, False), (False, True), (True, False), (True, True))     # (elliptical, background)


def free_indices(ell, back):
    return [0, 1, 2, 3] + ([4, 5] if ell else []) + [6] + ([7] if back else [])


def model8(v, jac=False):
    if not jac:
        return M.model(v[:7]) + v[7]
    m, J = M.model(v[:7], jac=True)
    return m + v[7], np.hstack([J, np.ones((m.size, 1))])


def used_pixels(data, var=None):
    d = np.asarray(data, dtype=float)
    ok = np.isfinite(d)
    if var is not None:
        va = np.asarray(var, dtype=float)
        with np.errstate(invalid='ignore'):
            ok &= np.isfinite(va) & (va > 0)
    return ok


def start(data, var, back):
    """Data-driven start values (8 entries) from the used pixels: brightest pixel, median background, the width of
    the disc of the pixels above half maximum."""
    ok = used_pixels(data, var)
    dz = np.where(ok, np.where(ok, data, 0.0), -np.inf)
    k = int(np.argmax(dz))
    p, q = divmod(k, NS)
    bg = float(np.median(np.asarray(data)[ok])) if back else 0.0
    fw = 2.0 * np.sqrt(np.count_nonzero(dz - bg > 0.5 * (dz.max() - bg)) / np.pi)
    return np.array([dz.max() - bg, p, q, max(fw, 1.5), 0.0, 0.0, 0.4, bg])


def derived(v):
    """peak, p0, q0, fwhm_major, fwhm_minor, n, rot (degrees), back of the 8 variables."""
    d = M.derived(v[:7])
    return np.array([d['peak'], d['p0'], d['q0'], d['fwhm_major'], d['fwhm_minor'], d['n'], d['rot'], v[7]])


KEYS = ('peak', 'p0', 'q0', 'fwhm_major', 'fwhm_minor', 'n', 'rot', 'back')


def fit(data, var, ell, back, v0=None, method='lm'):
    """Weighted least-squares fit of one stamp.  Returns a dict: x (8 variables), err (formal errors of the free
    variables, 0 for fixed ones), val / verr (KEYS: derived values and their errors, rot in degrees), chi2, npix,
    ba, status (scipy's)."""
    from scipy.optimize import least_squares
    d = np.asarray(data, dtype=float).ravel()
    ok = used_pixels(d, None if var is None else np.ravel(var))
    va = np.ones_like(d) if var is None else np.asarray(var, dtype=float).ravel()
    sw = np.where(ok, 1.0 / np.sqrt(np.where(ok, va, 1.0)), 0.0)
    dd = np.where(ok, d, 0.0)
    free = free_indices(ell, back)
    full = np.array(start(np.asarray(data).reshape(NS, NS), None if var is None else np.reshape(var, (NS, NS)), back)
                    if v0 is None else v0, dtype=float)
    if not ell:
        full[4:6] = 0.0
    if not back:
        full[7] = 0.0

    def ex(x):
        v = full.copy()
        v[free] = x
        return v

    def res(x):
        return (model8(ex(x)) - dd) * sw

    def jac(x):
        return model8(ex(x), True)[1][:, free] * sw[:, None]

    r = least_squares(res, full[free], jac=jac, method=method, xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
    J = jac(r.x)
    npix = int(ok.sum())
    chi2 = float((res(r.x) ** 2).sum())
    cov = np.linalg.inv(J.T @ J) * chi2 / (npix - len(free))
    x = ex(r.x)
    err = np.zeros(8)
    err[free] = np.sqrt(np.diag(cov))
    # first-order errors of the derived values: G cov G^T with G by central differences
    G = np.zeros((len(KEYS), len(free)))
    for c, k in enumerate(free):
        h = 1e-6 * max(abs(x[k]), 1e-2)
        xp, xm = x.copy(), x.copy()
        xp[k] += h
        xm[k] -= h
        dv = derived(xp) - derived(xm)
        dv[6] = (dv[6] + 90.0) % 180.0 - 90.0
        G[:, c] = dv / (2 * h)
    verr = np.sqrt(np.maximum(np.einsum('ij,jk,ik->i', G, cov, G), 0.0))
    e = np.hypot(x[4], x[5])
    return dict(x=x, err=err, val=derived(x), verr=verr, chi2=chi2, npix=npix, ba=np.sqrt((1 - e) / (1 + e)),
                status=r.status, redchi2=chi2 / (npix - len(free)))


def gpu_values(row):
    """The KEYS values and their errors from a library row (NFIT_ELL, observed layout)."""
    val = np.array([row[0], row[1], row[2], row[7], row[8], row[5], row[6], row[21]])
    err = np.array([row[11], row[12], row[13], row[14], row[15], row[17], row[16], row[22]])
    return val, err


def noisy_stamps(ell, back, count=40, seed=3):
    """`count` observed stars of one variant: FWHM 3-8 px, n 1.8-4, b/a 0.6-1 (elliptical), peak SNR 30-1000 with a
    variance of a read-noise term plus a signal term, 2 % random NaN pixels, one 3 x 3 block of var = 0, background
    in -2 ... 5 % of the peak.  Returns (data, var, truth): (count, 40, 40) twice and (count, 8)."""
    rng = np.random.default_rng([seed, int(ell), int(back)])
    data, var, truth = [], [], []
    for _ in range(count):
        peak = rng.uniform(0.5, 2)
        p0, q0 = 19.5 + rng.uniform(-2, 2, 2)
        fw = rng.uniform(3, 8)
        n = rng.uniform(1.8, 4)
        ba = rng.uniform(0.6, 1) if ell else 1.0
        rot = rng.uniform(0, 180)
        b = rng.uniform(-0.02, 0.05) * peak if back else 0.0
        snr = 10 ** rng.uniform(np.log10(30), np.log10(1000))
        e1, e2 = M.e_from_ratio(ba, rot)
        t = np.array([peak, p0, q0, fw, e1, e2, 1 / n, b])
        m = model8(t).reshape(NS, NS)
        va = (peak / snr) ** 2 * (0.2 + 0.8 * np.clip(m, 0, None) / peak)
        d = m + rng.normal(size=m.shape) * np.sqrt(va)
        d[rng.uniform(size=m.shape) < 0.02] = np.nan
        i, j = rng.integers(3, 34, 2)
        va[i:i + 3, j:j + 3] = 0.0
        data.append(d)
        var.append(va)
        truth.append(t)
    return np.array(data), np.array(var), np.array(truth)
