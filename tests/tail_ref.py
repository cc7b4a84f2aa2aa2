"""fp64 references of the tail of a call -- the two 'same' convolutions and the circular Moffat fit -- in plain
NumPy / SciPy, for tests/test_gpu_conv.py and tests/test_gpu_fit_circular.py.  Nothing here runs on a GPU and
nothing is read from the reference tree; tests/test_tail_ref.py checks this module on the CPU.

Convolutions: scipy.signal.fftconvolve(mode='same') in float64, the call the reference itself makes
(psfrec.py:917, 928), with the oracle's kernels (pinned to the reference at 4e-14 by oracle/make_golden.py).

Fit: the model of K_FIT, I (1 + u K)^(-1/eta), u = (p - p0)^2 + (q - q0)^2, K = 4 (2^eta - 1) / w^2, in the
variables (I, p0, q0, w = FWHM [px], eta = 1 / n), with its Jacobian in closed form.
"""
import numpy as np
from scipy.optimize import leastsq
from scipy.signal import fftconvolve

import psfr_oracle as O

NS = 40
KS = 41
LN2 = np.log(2.0)


def kernels(lbda, seeing, gl, l0, pixscale=0.2):
    """(tip-tilt kernel (41, 41), instrument kernels (nl, 41, 41)) of one task, as convolve_final_psf builds them."""
    lbda = np.atleast_1d(np.asarray(lbda, dtype=float))
    ktt = O.moffat_kernel(O.tiptilt_alpha(seeing, gl, l0, pixscale), 2, KS)
    fwhm, beta = O.muse_intrinsic_psf(lbda)
    alpha = fwhm / pixscale / (2 * np.sqrt(2 ** (1. / beta) - 1))
    return ktt, np.array([O.moffat_kernel(alpha[k], beta[k], KS) for k in range(lbda.size)])


def final_stamps(lbda, seeing, gl, l0, pre, pixscale=0.2, tiptilt=True):
    """convolve_final_psf (psfrec.py:874-930) of `pre` (nl, 40, 40) for one task, or (ntask, nl, 40, 40) with
    per-task seeing, gl, l0.  tiptilt=False leaves the tip-tilt convolution out (the limit GL -> 1, where the
    kernel is the identity and the reference's own Moffat2DKernel(0, 2) is NaN)."""
    lbda = np.atleast_1d(np.asarray(lbda, dtype=float))
    pre = np.asarray(pre, dtype=np.float64)
    if pre.ndim == 4:
        seeing, gl, l0 = (np.broadcast_to(np.atleast_1d(x), pre.shape[:1]) for x in (seeing, gl, l0))
        return np.array([final_stamps(lbda, seeing[t], gl[t], l0[t], pre[t], pixscale, tiptilt)
                         for t in range(pre.shape[0])])
    assert pre.shape == (lbda.size, NS, NS)
    ktt, kmuse = kernels(lbda, seeing, 0.5 if not tiptilt else gl, l0, pixscale)
    out = np.empty_like(pre)
    for k in range(lbda.size):
        tmp = fftconvolve(pre[k], ktt, mode='same') if tiptilt else pre[k]
        out[k] = fftconvolve(tmp, kmuse[k], mode='same')
    return out


_P, _Q = (a.astype(float) for a in np.indices((NS, NS)))


def _terms(v):
    I, p0, q0, w, eta = (float(x) for x in v)
    n = 1.0 / eta
    s = 2.0 ** eta - 1.0
    K = 4.0 * s / (w * w)
    dp, dq = _P - p0, _Q - q0
    u = dp * dp + dq * dq
    g = 1.0 + u * K
    return I, w, n, s, K, dp, dq, u, g


def moffat_vw(v):
    """The model at v = (I, p0, q0, w, eta) on the 40 x 40 stamp."""
    I, w, n, s, K, dp, dq, u, g = _terms(v)
    return I * g ** (-n)


def moffat_stamp(peak, p0, q0, fwhm, n):
    """Exact circular Moffat of FWHM `fwhm` [px] and index n, centred at row p0, column q0."""
    return moffat_vw((peak, p0, q0, fwhm, 1.0 / n))


def moffat_jacobian(v):
    """d model / d (I, p0, q0, w, eta) at v, shape (1600, 5), in closed form:
         d/dI = g^-n,  d/dp0 = 2 n K (p - p0) m / g,  d/dq0 likewise,  d/dw = 2 n K u m / (g w),
         d/deta = n^2 m ln g - n K (s'/s) u m / g,   s = 2^eta - 1, s' = 2^eta ln 2."""
    I, w, n, s, K, dp, dq, u, g = _terms(v)
    e = g ** (-n)
    m = I * e
    t = m / g
    J = np.empty((NS * NS, 5))
    J[:, 0] = e.ravel()
    J[:, 1] = (2 * n * K * t * dp).ravel()
    J[:, 2] = (2 * n * K * t * dq).ravel()
    J[:, 3] = (2 * n * K * t * u / w).ravel()
    J[:, 4] = (n * n * m * np.log(g) - n * K * ((s + 1.0) * LN2 / s) * t * u).ravel()
    return J


def kappa(peak, p0, q0, fwhm, n):
    """The ill-conditioning number of include/mpsfr.h (MPSFR_FIT_ILL_CONDITIONED): n^2 sqrt((J^T J)^-1[eta, eta])
    peak, the standard deviation of the fitted n per unit of relative pixel noise, from the fp64 Jacobian at
    the given parameters."""
    J = moffat_jacobian((peak, p0, q0, fwhm, 1.0 / n))
    cov = np.linalg.inv(J.T @ J)
    return n * n * np.sqrt(cov[4, 4]) * abs(peak)


def fit(stamp, start):
    """Least-squares circular Moffat fit of `stamp` with MINPACK (xtol = ftol = 1e-14) from start = (peak, p0,
    q0, fwhm, n).  Returns a dict: peak, p0, q0, fwhm [px], n, alpha, chi2, flux, and the error columns by the
    recipe of oracle.moffat_fit(errors=True) -- the inverse of J^T J at the solution times chi2 / dof, carried
    to (alpha, n, fwhm) by first-order propagation, which for a covariance under a change of variables is exact
    (J_y = J_x G^-1, so cov_y = G cov_x G^T): the same numbers whichever variables the fit ran in."""
    d = np.asarray(stamp, dtype=np.float64).ravel()
    v0 = [start[0], start[1], start[2], start[3], 1.0 / start[4]]
    v, cov, info, _, ier = leastsq(lambda v: moffat_vw(v).ravel() - d, v0, Dfun=moffat_jacobian, full_output=True,
                                   xtol=1e-14, ftol=1e-14, gtol=0.0)
    I, p0, q0, w, eta = v
    w = abs(w)
    n = 1.0 / eta
    p2 = 2.0 ** eta
    s2 = p2 - 1.0
    al = w / (2 * np.sqrt(s2))
    chi2 = float(np.sum(info['fvec'] ** 2))
    J = moffat_jacobian(v)
    c = np.linalg.inv(J.T @ J)
    sc = chi2 / (d.size - 5)
    aw = 1.0 / (2 * np.sqrt(s2))
    an = -al * p2 * LN2 / (2 * s2)
    return dict(peak=I, p0=p0, q0=q0, fwhm=w, n=n, alpha=al, chi2=chi2, flux=I * np.pi * al * al / (n - 1),
                err_peak=np.sqrt(c[0, 0] * sc), err_p0=np.sqrt(c[1, 1] * sc), err_q0=np.sqrt(c[2, 2] * sc),
                err_alpha=np.sqrt((aw * aw * c[3, 3] + 2 * aw * an * c[3, 4] + an * an * c[4, 4]) * sc),
                err_n=n * n * np.sqrt(c[4, 4] * sc), err_fwhm=np.sqrt(c[3, 3] * sc), ier=ier)


def perturbed_cases():
    """Stamps with a known minimum that is not the truth: a Moffat (peak 1, n 2.5, FWHM 3 and 8 px; centred and with
    the brightest pixel four pixels from the top edge, where K_FIT takes its fallback start) plus a fixed
    perturbation of 1e-3 of the peak -- a second, wider Moffat off to one side, or a seeded noise field.
    Returns [(name, truth (peak, p0, q0, fwhm, n), stamp)]; tests/test_tail_ref.py holds that MINPACK reaches the
    same minimum from two starts on every one of them."""
    rng = np.random.default_rng(77)
    noise = rng.standard_normal((NS, NS))
    noise *= 1e-3 / np.abs(noise).max()
    cases = []
    for fw in (3.0, 8.0):
        for where, (p0, q0) in (('centre', (19.7, 20.2)), ('rm4', (4.3, 20.4))):
            truth = (1.0, p0, q0, fw, 2.5)
            base = moffat_stamp(*truth)
            wide = moffat_stamp(1e-3, p0 + 0.8, q0 - 0.6, 2.5 * fw, 1.8)
            cases.append(('wide_fwhm%g_%s' % (fw, where), truth, base + wide))
            cases.append(('noise_fwhm%g_%s' % (fw, where), truth, base + noise))
    return cases
