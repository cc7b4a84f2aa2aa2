"""NumPy / SciPy yardstick of the PSF-model fit of star cubes (mpsfr_fit_spectra_psf, include/mpsfr.h), and the noisy,
masked star cubes the CPU and GPU tests share.

Model, per star: m_l(p, q) = F_l P~_l(p - dp - sp x_l, q - dq - sq x_l) + b_l over the layers l, P~ the Keys resampling
of psf_fit_ref.  The yardstick is the joint problem, independent of any elimination: all variables (theta = (dp, dq[,
sp, sq]), then (F_l[, b_l]) of every fitted layer) go to scipy's least_squares ('lm') with the analytic Jacobian,
followed by joint Newton steps in fp64 (Gauss-Newton steps diverge on the faint stars, see joint_fit) until the step is
below 1e-10 of the formal error.  Errors: sqrt(diag((J^T J)^-1) chi2 / dof) of the weighted joint Jacobian,
dof = N_used - nvar.

`eliminated` is the other route, the one the kernel takes (variable projection: the layers' linear solves inside, a
descent in theta on the Schur complements); tests/test_psf_spec_host.py holds it against the joint solution.
"""
import numpy as np

import psf_fit_ref as R

NS = R.NS
MAX_SHIFT = R.MAX_SHIFT
VARIANTS = ((False, False), (True, False), (False, True), (True, True))      # (background, drift)
WAVES = 4                          # waves of a workgroup of k_fit_spec (kSpecWaves, fit_spec.hip)
SNR = (20, 20, 3, 3, 1, 1)
NLAYERS = (5, 5, 5, 5, 12, 12)
NAN_LAYER = (1, 2)                 # (star, layer): wholly NaN


def layer_fitted(d, va, psf, back):
    """A layer takes part in the fit: enough used pixels, no infinite pixel under a valid variance, a finite model
    stamp whose largest modulus lies in [2^-40, 2^40].  Returns (fitted, n_used)."""
    d = np.asarray(d, dtype=float)
    ok = R.used_pixels(d, va)
    vok = np.ones_like(ok) if va is None else R.used_pixels(np.zeros_like(d), va)
    bad = vok & np.isinf(d)
    pmax = np.abs(psf).max() if np.all(np.isfinite(psf)) else np.nan
    fitted = (ok.sum() >= (2 if back else 1) + 1 and not bad.any() and np.isfinite(pmax)
              and 2.0 ** -40 <= pmax <= 2.0 ** 40)
    return bool(fitted), int(ok.sum())


def layers_of(cube, var, psfs, back):
    info = [layer_fitted(cube[l], None if var is None else var[l], psfs[l], back) for l in range(len(cube))]
    return np.array([f for f, _ in info]), np.array([n for _, n in info])


def default_start(cube, var, psfs, back):
    """The start of the definition without a given shift: the first maximum of sum_l d_l / var_l over the used pixels
    of the fitted layers minus the first maximum of sum_l P_l (fitted layers), brought into the domain."""
    fitted, _ = layers_of(cube, var, psfs, back)
    c = np.zeros((NS, NS))
    p = np.zeros((NS, NS))
    for l in np.flatnonzero(fitted):
        va = None if var is None else var[l]
        ok = R.used_pixels(cube[l], va)
        w = np.ones((NS, NS)) if va is None else np.where(ok, 1.0 / np.where(ok, va, 1.0), 0.0)
        c += np.where(ok, np.where(ok, cube[l], 0.0) * w, 0.0)
        p += psfs[l]
    ks, kp = int(np.argmax(c)), int(np.argmax(p))
    return np.array([np.clip(ks // NS - kp // NS, -MAX_SHIFT, MAX_SHIFT),
                     np.clip(ks % NS - kp % NS, -MAX_SHIFT, MAX_SHIFT)], dtype=float)


class Problem:
    """The joint problem of one star: variables theta (2 or 4), then (F_l[, b_l]) of every fitted layer in order."""

    def __init__(self, cube, var, psfs, back, drift, x=None):
        self.cube = np.asarray(cube, dtype=float)
        self.var = None if var is None else np.asarray(var, dtype=float)
        self.psfs = np.asarray(psfs, dtype=float)
        self.back, self.drift = bool(back), bool(drift)
        self.nl = len(self.cube)
        self.x = np.zeros(self.nl) if x is None else np.asarray(x, dtype=float)
        self.fitted, self.n_used = layers_of(self.cube, self.var, self.psfs, back)
        self.layers = np.flatnonzero(self.fitted)
        self.nt = 4 if drift else 2
        self.nlin = 2 if back else 1
        self.nvar = self.nt + self.nlin * len(self.layers)
        self.npix = int(self.n_used[self.layers].sum())
        self.dof = self.npix - self.nvar
        self.w = {}
        for l in self.layers:
            ok, sw, dd = R._weights(self.cube[l], None if self.var is None else self.var[l])
            self.w[l] = (ok.ravel(), sw.ravel(), dd.ravel())

    def shift(self, theta, l):
        dp, dq = theta[0], theta[1]
        if self.drift:
            dp, dq = dp + theta[2] * self.x[l], dq + theta[3] * self.x[l]
        return dp, dq

    def inside(self, theta):
        return all(abs(s) <= MAX_SHIFT for l in self.layers for s in self.shift(theta, l))

    def linear(self, theta):
        """(F_l, b_l) of every fitted layer at theta: the closed-form solves."""
        return np.array([R.linear_solve(self.cube[l], None if self.var is None else self.var[l], self.psfs[l],
                                        *self.shift(theta, l), self.back) for l in self.layers])

    def pack(self, theta, lin):
        return np.concatenate([np.asarray(theta, dtype=float)[:self.nt], np.asarray(lin)[:, :self.nlin].ravel()])

    def unpack(self, v):
        lin = np.zeros((len(self.layers), 2))
        lin[:, :self.nlin] = v[self.nt:].reshape(-1, self.nlin)
        return v[:self.nt], lin

    def residual(self, v, jac=False):
        """Weighted residuals over the used pixels of the fitted layers (and the Jacobian)."""
        theta, lin = self.unpack(v)
        res, rows = [], []
        for k, l in enumerate(self.layers):
            ok, sw, dd = self.w[l]
            dp, dq = self.shift(theta, l)
            out = R.model(self.psfs[l], (lin[k, 0], dp, dq, lin[k, 1]), jac)
            m = out[0] if jac else out
            res.append(((m.ravel() - dd) * sw)[ok])
            if jac:
                jl = (out[1].reshape(-1, 4) * sw[:, None])[ok]
                J = np.zeros((jl.shape[0], self.nvar))
                J[:, 0:2] = jl[:, 1:3]
                if self.drift:
                    J[:, 2:4] = jl[:, 1:3] * self.x[l]
                c = self.nt + self.nlin * k
                J[:, c] = jl[:, 0]
                if self.back:
                    J[:, c + 1] = jl[:, 3]
                rows.append(J)
        r = np.concatenate(res)
        return (r, np.concatenate(rows)) if jac else r

    def layer_chi2(self, v):
        theta, lin = self.unpack(v)
        out = np.zeros(self.nl)
        for k, l in enumerate(self.layers):
            ok, sw, dd = self.w[l]
            dp, dq = self.shift(theta, l)
            m = R.model(self.psfs[l], (lin[k, 0], dp, dq, lin[k, 1]))
            out[l] = float(((((m.ravel() - dd) * sw)[ok]) ** 2).sum())
        return out


def joint_fit(prob, theta0):
    """The yardstick.  Returns a dict: theta (4, zeros where not fitted), err_theta (4), F, b, err_F, err_b, chi2_l (nl,
    zeros on left-out layers), chi2, npix, nlayers, dof, v (the joint vector), cov (its covariance)."""
    from scipy.optimize import least_squares
    t0 = np.zeros(prob.nt)
    t0[:2] = theta0[:2]
    v = prob.pack(t0, prob.linear(t0))
    r = least_squares(prob.residual, v, jac=lambda y: prob.residual(y, True)[1], method='lm', xtol=1e-15, ftol=1e-15,
                      gtol=1e-15, max_nfev=4000)
    v = r.x

    def gradient(y):
        rr, J = prob.residual(y, True)
        return J.T @ rr

    # Newton steps to the bottom.  (Gauss-Newton steps do not get there on the faint stars: with a peak pixel at the
    # noise level the residuals are as large as the model, the term of the second derivatives in the Hessian is as
    # large as J^T J, and the undamped Gauss-Newton iteration diverges from a point 1e-6 px from the minimum.)  The
    # Hessian is the central difference of the analytic gradient.
    for _ in range(40):
        rr, J = prob.residual(v, True)
        g = J.T @ rr
        hs = 1e-5 * np.maximum(1.0, np.abs(v))
        H = np.empty((prob.nvar, prob.nvar))
        for k in range(prob.nvar):
            e = np.zeros(prob.nvar)
            e[k] = hs[k]
            H[:, k] = (gradient(v + e) - gradient(v - e)) / (2 * hs[k])
        H = 0.5 * (H + H.T)
        dx = -np.linalg.solve(H, g)
        v = v + dx
        cov = np.linalg.inv(J.T @ J) * float(rr @ rr) / prob.dof
        if np.all(np.abs(dx) <= 1e-10 * np.sqrt(np.diag(cov))) or float(rr @ rr) == 0.0:
            break
    else:
        raise RuntimeError('the yardstick did not converge')
    rr, J = prob.residual(v, True)
    chi2 = float(rr @ rr)
    cov = np.linalg.inv(J.T @ J) * chi2 / prob.dof
    err = np.sqrt(np.diag(cov))
    theta, lin = prob.unpack(v)
    _, elin = prob.unpack(err)
    out = dict(theta=np.zeros(4), err_theta=np.zeros(4), F=np.zeros(prob.nl), b=np.zeros(prob.nl),
               err_F=np.zeros(prob.nl), err_b=np.zeros(prob.nl), chi2_l=prob.layer_chi2(v), chi2=chi2, npix=prob.npix,
               nlayers=len(prob.layers), dof=prob.dof, v=v, cov=cov)
    out['theta'][:prob.nt] = theta
    out['err_theta'][:prob.nt] = err[:prob.nt]
    out['F'][prob.layers], out['b'][prob.layers] = lin[:, 0], lin[:, 1]
    out['err_F'][prob.layers], out['err_b'][prob.layers] = elin[:, 0], elin[:, 1]
    return out


# ---- the elimination (variable projection), as the kernel does it

def reduced(prob, theta):
    """At theta, with every layer at its linear optimum: (S, g, chi2, parts); S = sum X_l^T S_l X_l with
    S_l = A_tt - A_tl A_ll^-1 A_lt, g = sum X_l^T J_t^T W r.  parts: per fitted layer (F, b, A_ll^-1, B = A_ll^-1 A_lt
    X_l, chi2_l)."""
    nt, nlin = prob.nt, prob.nlin
    S, g, chi2, parts = np.zeros((nt, nt)), np.zeros(nt), 0.0, []
    lin = prob.linear(theta)
    for k, l in enumerate(prob.layers):
        ok, sw, dd = prob.w[l]
        dp, dq = prob.shift(theta, l)
        m, jac = R.model(prob.psfs[l], (lin[k, 0], dp, dq, lin[k, 1]), True)
        r = ((m.ravel() - dd) * sw)[ok]
        J = (jac.reshape(-1, 4) * sw[:, None])[ok]
        Jl, Jt = J[:, [0, 3][:nlin]], J[:, 1:3]
        All, Alt, Att = Jl.T @ Jl, Jl.T @ Jt, Jt.T @ Jt
        Ainv = np.linalg.inv(All)
        Sl = Att - Alt.T @ Ainv @ Alt
        X = np.hstack([np.eye(2), prob.x[l] * np.eye(2)]) if prob.drift else np.eye(2)
        S += X.T @ Sl @ X
        g += X.T @ (Jt.T @ r)
        c2 = float(r @ r)
        chi2 += c2
        parts.append((lin[k, 0], lin[k, 1], Ainv, Ainv @ Alt @ X, c2))
    return S, g, chi2, parts


def eliminated(prob, theta0, maxit=200):
    """Gauss-Newton with step halving in theta on the reduced normal equations, then the error formulas of the
    elimination.  The dict of joint_fit (without v and cov)."""
    theta = np.zeros(prob.nt)
    theta[:2] = theta0[:2]
    S, g, chi2, parts = reduced(prob, theta)
    for _ in range(maxit):
        dx = -np.linalg.solve(S, g)
        f = 1.0
        while True:
            tn = theta + f * dx
            if prob.inside(tn):
                Sn, gn, cn, pn = reduced(prob, tn)
                if cn <= chi2 or np.abs(f * dx).max() < 1e-13:
                    break
            f *= 0.5
            if f < 1e-6:
                break
        theta, S, g, chi2, parts = tn, Sn, gn, cn, pn
        if np.abs(f * dx).max() < 1e-13:
            break
    s = chi2 / prob.dof
    ct = np.linalg.inv(S) * s
    out = dict(theta=np.zeros(4), err_theta=np.zeros(4), F=np.zeros(prob.nl), b=np.zeros(prob.nl),
               err_F=np.zeros(prob.nl), err_b=np.zeros(prob.nl), chi2_l=np.zeros(prob.nl), chi2=chi2, npix=prob.npix,
               nlayers=len(prob.layers), dof=prob.dof)
    out['theta'][:prob.nt] = theta
    out['err_theta'][:prob.nt] = np.sqrt(np.diag(ct))
    for l, (F, b, Ainv, B, c2) in zip(prob.layers, parts):
        cl = Ainv * s + B @ ct @ B.T
        out['F'][l], out['b'][l], out['chi2_l'][l] = F, b, c2
        out['err_F'][l] = np.sqrt(cl[0, 0])
        if prob.back:
            out['err_b'][l] = np.sqrt(cl[1, 1])
    return out


# ---- the shared stars

def model_cube(nl, golden=False):
    """Model stamps of a star: Moffat PSFs (sum 1) whose FWHM runs 4.5 -> 2.6 px over the layers, or g9_profile golden
    stamps."""
    if golden:
        return R.golden_stamps()[:nl].copy()
    fw = np.linspace(4.5, 2.6, nl) if nl > 1 else np.array([3.0])
    return np.array([R.moffat(20.0, 20.0, f, 2.5) / R.moffat(20.0, 20.0, f, 2.5).sum() for f in fw])


def make_star(rng, nl, snr, back, drift, golden=False, nan_layer=None):
    """One star cube: (cube, var, psfs, x, truth) with truth = dict(theta (4), F (nl), b (nl))."""
    psfs = model_cube(nl, golden)
    x = np.linspace(-1.0, 1.0, nl) if nl > 1 else np.zeros(1)
    theta = np.zeros(4)
    theta[:2] = rng.uniform(-3, 3, 2)
    if drift:
        theta[2:] = rng.uniform(-0.4, 0.4, 2)
    F = 1000.0 * rng.uniform(0.5, 1.5, nl)
    cube, var, bs = [], [], []
    for l in range(nl):
        dp, dq = theta[0] + theta[2] * x[l], theta[1] + theta[3] * x[l]
        if golden:
            star = F[l] * R.resample(psfs[l], dp, dq)
        else:
            fw = np.linspace(4.5, 2.6, nl)[l] if nl > 1 else 3.0
            star = F[l] * R.moffat(20.0 + dp, 20.0 + dq, fw, 2.5) / R.moffat(20.0, 20.0, fw, 2.5).sum()
        peak = star.max()
        b = rng.uniform(-0.01, 0.05) * peak if back else 0.0
        sig = peak / snr
        d = star + b + rng.normal(size=star.shape) * sig
        va = np.full((NS, NS), sig ** 2)
        d[rng.uniform(size=star.shape) < 0.03] = np.nan
        i, j = rng.integers(3, 34, 2)
        va[i:i + 3, j:j + 3] = 0.0
        if nan_layer == l:
            d[:] = np.nan
        cube.append(d)
        var.append(va)
        bs.append(b)
    return np.array(cube), np.array(var), psfs, x, dict(theta=theta, F=F, b=np.array(bs))


_STARS = {}


def stars(back, drift):
    """The six shared stars of a variant: a list of dicts with cube, var, psfs, x, truth, snr and shift (the start: None
    for the SNR-20 stars, which use the default start; the truth rounded to 1/2 px for the faint ones)."""
    key = (bool(back), bool(drift))
    if key not in _STARS:
        rng = np.random.default_rng([13, int(back), int(drift)])
        out = []
        for k, (snr, nl) in enumerate(zip(SNR, NLAYERS)):
            cube, var, psfs, x, truth = make_star(rng, nl, snr, back, drift, golden=(k == 3),
                                                  nan_layer=NAN_LAYER[1] if k == NAN_LAYER[0] else None)
            shift = None if snr >= 20 else np.round(truth['theta'][:2] * 2) / 2
            out.append(dict(cube=cube, var=var, psfs=psfs, x=x, truth=truth, snr=snr, shift=shift))
        _STARS[key] = out
    return _STARS[key]


_UNEVEN = {}


def uneven_stars(back, drift):
    """Two SNR-20 stars of 2 W + 3 layers: the waves of a workgroup carry unequal shares (default start)."""
    key = (bool(back), bool(drift))
    if key not in _UNEVEN:
        rng = np.random.default_rng([14, int(back), int(drift)])
        out = []
        for k in range(2):
            cube, var, psfs, x, truth = make_star(rng, 2 * WAVES + 3, 20, back, drift, nan_layer=4 if k == 1 else None)
            out.append(dict(cube=cube, var=var, psfs=psfs, x=x, truth=truth, snr=20, shift=None))
        _UNEVEN[key] = out
    return _UNEVEN[key]


def problem(star, back, drift):
    return Problem(star['cube'], star['var'], star['psfs'], back, drift, star['x'] if drift else None)


def start_of(star, back):
    if star['shift'] is not None:
        return np.asarray(star['shift'], dtype=float)
    return default_start(star['cube'], star['var'], star['psfs'], back)


_YARD = {}


def yardstick(back, drift, uneven=False):
    """(stars, fits) of a variant, computed once: the joint fit of every shared star from its start."""
    key = (bool(back), bool(drift), bool(uneven))
    if key not in _YARD:
        ss = uneven_stars(back, drift) if uneven else stars(back, drift)
        _YARD[key] = (ss, [joint_fit(problem(s, back, drift), start_of(s, back)) for s in ss])
    return _YARD[key]


def batch(ss):
    """Stars of equal nl as the arrays of one call: (cubes, var, psf, shift or None)."""
    cubes = np.array([s['cube'] for s in ss])
    var = np.array([s['var'] for s in ss])
    psf = np.array([s['psfs'] for s in ss])
    sh = None if ss[0]['shift'] is None else np.array([s['shift'] for s in ss])
    return cubes, var, psf, sh


def row_values(head, layers):
    """theta (4), its errors (4), F, b, err_F, err_b (nl each) of a library row."""
    return head[0:4], head[4:8], layers[:, 0], layers[:, 1], layers[:, 2], layers[:, 3]
