"""NumPy / SciPy yardstick of the elliptical Moffat fit (mpsfr_fit_stamps_elliptical, include/mpsfr.h).

Model on a 40 x 40 stamp (rows p, columns q; x = q - q0, y = p - p0):
    I (1 + Q)^-n,  Q = (g / alpha^2) [(1 - e1) x^2 - 2 e2 x y + (1 + e1) y^2],  g = 1 / sqrt(1 - e1^2 - e2^2)
fitted in (I, p0, q0, w, e1, e2, eta = 1/n), w = 2 alpha sqrt(2^eta - 1), by scipy's Levenberg-Marquardt with the
analytic Jacobian.
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
