"""NumPy / SciPy yardstick of the elliptical Moffat fit (mpsfr_fit_stamps_elliptical, include/mpsfr.h).

Model on a 40 x 40 stamp (rows p, columns q; x = q - q0, y = p - p0):
    I (1 + Q)^-n,  Q = (g / alpha^2) [(1 - e1) x^2 - 2 e2 x y + (1 + e1) y^2],  g = 1 / sqrt(1 - e1^2 - e2^2)
fitted in (I, p0, q0, w, e1, e2, eta = 1/n), w = 2 alpha sqrt(2^eta - 1), by scipy's Levenberg-Marquardt with the
analytic Jacobian.

fit_full adds every derived column of MPSFR_NFIT_ELL by the recipe of the header: chi2, flux, and the error columns
from inv(J^T J) chi2 / (1600 - 7), carried to the FWHMs, rot, n and flux through gradients taken numerically (central
differences of plain functions of the seven variables), so that no algebra of the kernel's epilogue is repeated here.
"""
import numpy as np

NS = 40


def e_from_ratio(ba, rot_deg):
    """(e1, e2) of axis ratio b/a with the major axis at rot (degrees from +q towards +p)."""
    e = (1.0 - ba * ba) / (1.0 + ba * ba)
    t = np.deg2rad(2.0 * rot_deg)
    return e * np.cos(t), e * np.sin(t)


def model(v, ns=NS, jac=False):
    I, p0, q0, w, e1, e2, eta = v
    n = 1.0 / eta
    s = 2.0 ** eta - 1.0
    K = 4.0 * s / (w * w)
    q = 1.0 - e1 * e1 - e2 * e2
    g = 1.0 / np.sqrt(q)
    p, qq = np.mgrid[0:ns, 0:ns].astype(float)
    y, x = (p - p0).ravel(), (qq - q0).ravel()
    gK = g * K
    A, B, C = gK * (1 - e1), gK * e2, gK * (1 + e1)
    Q = A * x * x - 2 * B * x * y + C * y * y
    lg = np.log1p(Q)
    e = np.exp(-n * lg)
    m = I * e
    if not jac:
        return m
    c = n * m / (1.0 + Q)
    dKn = (s + 1.0) * np.log(2.0) / s
    J = np.empty((m.size, 7))
    J[:, 0] = e
    J[:, 1] = 2 * c * (C * y - B * x)
    J[:, 2] = 2 * c * (A * x - B * y)
    J[:, 3] = 2 * c * Q / w
    J[:, 4] = c * (gK * (x * x - y * y) - e1 / q * Q)
    J[:, 5] = c * (2 * gK * x * y - e2 / q * Q)
    J[:, 6] = m * n * n * lg - c * Q * dKn
    return m, J


def stamp(peak, p0, q0, fwhm, ba, rot_deg, n):
    """Exact model stamp; fwhm is the geometric-mean FWHM (px)."""
    e1, e2 = e_from_ratio(ba, rot_deg)
    return model((peak, p0, q0, fwhm, e1, e2, 1.0 / n)).reshape(NS, NS)


def derived(v):
    """(peak, p0, q0, fwhm_major, fwhm_minor, n, rot_deg, b/a) of LM variables v."""
    I, p0, q0, w, e1, e2, eta = v
    e = np.hypot(e1, e2)
    f = ((1 + e) / (1 - e)) ** 0.25
    rot = np.rad2deg(0.5 * np.arctan2(e2, e1)) % 180.0
    return dict(peak=I, p0=p0, q0=q0, fwhm_major=w * f, fwhm_minor=w / f, n=1.0 / eta, rot=rot, ba=1.0 / (f * f))


def fit(data, v0=None):
    """Least-squares fit of a stamp (fp64): the LM variables at the minimum."""
    from scipy.optimize import least_squares
    d = np.asarray(data, dtype=float).ravel()
    if v0 is None:
        k = int(np.argmax(d))
        p0, q0 = divmod(k, NS)
        fw = 2.0 * np.sqrt(np.count_nonzero(d > 0.5 * d[k]) / np.pi)
        v0 = (d[k], p0, q0, fw, 0.0, 0.0, 0.4)

    def res(v):
        return model(v) - d

    def jac(v):
        return model(v, jac=True)[1]

    r = least_squares(res, np.asarray(v0, dtype=float), jac=jac, method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15,
                      max_nfev=2000)
    return r.x


def gpu_derived(row):
    """The same quantities from a library fit row (NFIT_ELL)."""
    return dict(peak=row[0], p0=row[1], q0=row[2], fwhm_major=row[7], fwhm_minor=row[8], n=row[5], rot=row[6],
                ba=row[8] / row[7])


def rot_diff(a, b):
    """|a - b| in radians, modulo 180 degrees."""
    d = (np.asarray(a) - np.asarray(b)) % 180.0
    return np.deg2rad(np.minimum(d, 180.0 - d))


# ---- every column of MPSFR_NFIT_ELL in fp64
NPAR = 7
DOF = NS * NS - NPAR


def _axis_factor(v):
    e = np.hypot(v[4], v[5])
    return ((1 + e) / (1 - e)) ** 0.25


def _alpha(v):
    return v[3] / (2.0 * np.sqrt(2.0 ** v[6] - 1.0))


# the derived quantities of a row as plain functions of the LM variables v
QUANTITIES = {
    'fwhm_major': lambda v: v[3] * _axis_factor(v),
    'fwhm_minor': lambda v: v[3] / _axis_factor(v),
    'rot': lambda v: np.rad2deg(0.5 * np.arctan2(v[5], v[4])),            # degrees, not wrapped
    'n': lambda v: 1.0 / v[6],
    'flux': lambda v: v[0] * np.pi * _alpha(v) ** 2 / (1.0 / v[6] - 1.0),     # alpha_major alpha_minor = alpha^2
}


def num_gradient(name, v, h=1e-4):
    """d QUANTITIES[name] / d v by the five-point central difference with step h max(1, |v_k|): the truncation
    error is h^4 f^(5) / 30 (about 1e-11 relative at |e| >= 0.02, where the fifth derivative of |e| is 1 / e^4) and
    the rounding error eps |f| / h about 1e-11.  rot is differenced modulo 180 degrees."""
    f = QUANTITIES[name]
    v = np.asarray(v, dtype=float)
    g = np.zeros(NPAR)
    for k in range(NPAR):
        hk = h * max(1.0, abs(v[k]))
        val = []
        for m in (-2, -1, 1, 2):
            u = v.copy()
            u[k] += m * hk
            val.append(f(u))
        if name == 'rot':
            f0 = f(v)
            val = [(x - f0 + 90.0) % 180.0 - 90.0 for x in val]
        g[k] = (val[0] - 8 * val[1] + 8 * val[2] - val[3]) / (12 * hk)
    return g


def normal_inverse(v):
    """inv(J^T J) of the analytic Jacobian at v, and cond(J^T J)."""
    _, J = model(v, jac=True)
    A = J.T @ J
    return np.linalg.inv(A), float(np.linalg.cond(A))


def columns_at(v, chi2):
    """The error columns of the header's recipe at the point v with the given chi2: the covariance
    inv(J^T J) chi2 / (1600 - 7), first-order propagation.  err_rot is in degrees, capped at 180 (180 at e = 0)."""
    v = np.asarray(v, dtype=float)
    C, cond = normal_inverse(v)
    C = C * (chi2 / DOF)
    out = dict(err_peak=np.sqrt(C[0, 0]), err_p0=np.sqrt(C[1, 1]), err_q0=np.sqrt(C[2, 2]), cond=cond)
    for name in ('fwhm_major', 'fwhm_minor', 'n', 'flux'):
        g = num_gradient(name, v)
        out['err_' + name] = float(np.sqrt(max(g @ C @ g, 0.0)))
    if v[4] == 0.0 and v[5] == 0.0:
        out['err_rot'] = 180.0
    else:
        g = num_gradient('rot', v, h=min(1e-4, 0.05 * np.hypot(v[4], v[5])))
        er = float(np.sqrt(max(g @ C @ g, 0.0)))
        out['err_rot'] = min(er, 180.0) if er == er else 180.0
    return out


def kappa(v):
    """The ill-conditioning number of include/mpsfr.h with the 7-column Jacobian: n^2 sqrt(inv(J^T J)[eta, eta]) |I|."""
    C, _ = normal_inverse(v)
    return float(np.sqrt(C[6, 6]) * abs(v[0]) / (v[6] * v[6]))


def fit_full(data, v0=None):
    """fit(data, v0) and every derived column of MPSFR_NFIT_ELL at the minimum, in fp64.  Keys: v (the LM variables),
    those of derived(v), alpha_major, alpha_minor, chi2, flux, err_peak, err_p0, err_q0, err_fwhm_major,
    err_fwhm_minor, err_rot, err_n, err_flux, cond (of J^T J), kappa."""
    d = np.asarray(data, dtype=float).ravel()
    v = fit(d, v0)
    r = model(v) - d
    chi2 = float(r @ r)
    out = dict(v=v, chi2=chi2, kappa=kappa(v))
    out.update(derived(v))
    f = _axis_factor(v)
    out['alpha_major'], out['alpha_minor'] = _alpha(v) * f, _alpha(v) / f
    out['flux'] = QUANTITIES['flux'](v)
    out.update(columns_at(v, chi2))
    return out


def v_from_row(row):
    """The LM variables of a library fit row (NFIT_ELL)."""
    R = (row[7] / row[8]) ** 2
    e = (R - 1.0) / (R + 1.0)
    t = np.deg2rad(2.0 * row[6])
    return np.array([row[0], row[1], row[2], np.sqrt(row[7] * row[8]), e * np.cos(t), e * np.sin(t), 1.0 / row[5]])


# fit_out index of the columns fit_full names
COLUMN = dict(peak=0, p0=1, q0=2, alpha_major=3, alpha_minor=4, n=5, rot=6, fwhm_major=7, fwhm_minor=8, chi2=9,
              iterations=10, err_peak=11, err_p0=12, err_q0=13, err_fwhm_major=14, err_fwhm_minor=15, err_rot=16,
              err_n=17, status=18, flux=19, err_flux=20)


def perturbed_cases():
    """Stamps with a known minimum that is not the truth, as tail_ref.perturbed_cases but elliptical: a Moffat of peak
    1 and n 2.5, geometric-mean FWHM 3 and 8 px, (b/a, rot) = (0.7, 30) and (0.98, 120), centred at (19.7, 20.2) or at
    (4.3, 20.4) with the brightest pixel four pixels from the top edge, plus one of two fixed perturbations of 1e-3 of
    the peak: a round Moffat (peak 1e-3, FWHM 2.5 x the base, n 1.8) offset by (+0.8, -0.6) px, or the seeded noise
    field of tail_ref.perturbed_cases.  Returns 16 of [(name, truth as LM variables, stamp)]."""
    rng = np.random.default_rng(77)
    noise = rng.standard_normal((NS, NS))
    noise *= 1e-3 / np.abs(noise).max()
    cases = []
    for fw in (3.0, 8.0):
        for ba, rot in ((0.7, 30.0), (0.98, 120.0)):
            for where, (p0, q0) in (('centre', (19.7, 20.2)), ('rm4', (4.3, 20.4))):
                e1, e2 = e_from_ratio(ba, rot)
                truth = np.array([1.0, p0, q0, fw, e1, e2, 1.0 / 2.5])
                base = stamp(1.0, p0, q0, fw, ba, rot, 2.5)
                wide = stamp(1e-3, p0 + 0.8, q0 - 0.6, 2.5 * fw, 1.0, 0.0, 1.8)
                tag = 'fwhm%g_ba%g_%s' % (fw, ba, where)
                cases.append(('wide_' + tag, truth, base + wide))
                cases.append(('noise_' + tag, truth, base + noise))
    return cases


def three_starts(truth):
    """The truth, the truth x 1.05 with e + 0.02, and None (the default start of fit)."""
    off = np.asarray(truth, dtype=float) * 1.05
    off[4:6] = np.asarray(truth[4:6]) + 0.02
    return [np.asarray(truth, dtype=float), off, None]


_PERTURBED = []


def perturbed_references():
    """[(name, stamp, fit_full from the truth, worst relative difference of the minimum over three_starts)] of
    perturbed_cases, computed once per process."""
    if not _PERTURBED:
        for name, truth, st in perturbed_cases():
            full = fit_full(st, truth)
            spread = 0.0
            for v0 in three_starts(truth)[1:]:
                v = fit(st, v0)
                spread = max(spread, float(np.max(np.abs(v - full['v']) / np.maximum(np.abs(full['v']), 1.0))))
            _PERTURBED.append((name, st, full, spread))
    return _PERTURBED
