"""CPU: the yardstick of the PSF-model fit (tests/psf_fit_ref.py) against its own definition, and the argument
validation of the Python layer.

* the Keys weights of any sample position sum to 1; an integer shift reproduces the stamp exactly (rolled, zero
  extended);
* the analytic Jacobian equals central differences to 1e-6 (relative to the largest entry of its column);
* the yardstick's floor on the shared stars: a restart 0.3 px off reaches the same minimum to <= 1e-6 formal sigma
  (the GPU test allows the f64 kernel ten times that), SciPy reports convergence, and the pulls against the truth
  of the stars whose model is exact have an rms of order 1;
* the closed-form linear solve is the minimum of the fixed-shift problem;
* psf_fit_arguments / psf_fit_flags refuse what mpsfr_fit_stamps_psf refuses.
"""
import numpy as np
import pytest

import psf_fit_ref as R


def test_keys_weights_sum_to_one_and_interpolate():
    for d in np.linspace(-7.9, 7.9, 80):
        w, dw = R.tap_matrix(d)
        inner = slice(12, 28)                       # rows whose four taps lie on the stamp
        assert np.max(np.abs(w[inner].sum(axis=1) - 1.0)) <= 1e-14
        assert np.max(np.abs(dw[inner].sum(axis=1))) <= 1e-13
    assert R.keys(0.0) == 1.0 and np.all(R.keys(np.array([-2.0, -1.0, 1.0, 2.0, 2.5])) == 0.0)
    # C1: the derivative is continuous across the knots
    for k in (-2.0, -1.0, 0.0, 1.0, 2.0):
        assert abs(R.dkeys(k - 1e-9) - R.dkeys(k + 1e-9)) <= 1e-8


def test_integer_shift_reproduces_the_stamp():
    rng = np.random.default_rng(1)
    P = rng.normal(size=(40, 40))
    for k, l in ((0, 0), (2, -3), (-8, 8), (5, 0)):
        want = np.zeros_like(P)
        src = P[max(0, -k):40 - max(0, k), max(0, -l):40 - max(0, l)]
        want[max(0, k):max(0, k) + src.shape[0], max(0, l):max(0, l) + src.shape[1]] = src
        assert np.array_equal(R.resample(P, float(k), float(l)), want), (k, l)


def test_jacobian_against_central_differences():
    data, var, psf, truth = R.noisy_stars(True)
    worst = 0.0
    for k in (0, 2, 5, 11):
        v = truth[k] + np.array([0.0, 0.137, -0.291, 0.0])
        _, J = R.model(psf[k], v, jac=True)
        for c in range(4):
            h = 1e-5 * max(abs(v[c]), 1.0) if c in (0, 3) else 1e-5
            vp, vm = v.copy(), v.copy()
            vp[c] += h
            vm[c] -= h
            num = (R.model(psf[k], vp) - R.model(psf[k], vm)) / (2 * h)
            worst = max(worst, float(np.max(np.abs(num - J[..., c])) / np.max(np.abs(J[..., c]))))
    print('Jacobian against central differences: %.2e' % worst)
    assert worst <= 1e-6


@pytest.mark.parametrize('back', [False, True])
def test_floor_of_the_yardstick_on_the_shared_stars(back):
    data, var, psf, truth, _, fits = R.yardstick(back, False)
    assert len(data) == 24
    ok = R.used_pixels(data, var)
    assert np.isnan(data).mean() > 0.02 and np.any(var == 0) and np.any(var < 0)
    worst, pulls, nfev = 0.0, [], []
    for k, f in enumerate(fits):
        assert f['status'] > 0 and f['npix'] == ok[k].sum()
        free = f['free']
        off = f['x'] + np.array([0.01 * f['x'][0], 0.3, -0.3, 0.001 * f['x'][0] if back else 0.0])
        g = R.fit(data[k], var[k], psf[k], back, v0=off)
        worst = max(worst, float(np.max(np.abs(g['x'] - f['x'])[free] / f['err'][free])))
        assert abs(g['chi2'] - f['chi2']) <= 1e-9 * f['chi2']
        nfev.append(f['nfev'])
        assert np.max(np.abs(f['x'][1:3] - truth[k, 1:3])) < 0.5
        if k % 3 == 2:                              # the model is exact for these stars
            pulls.extend(((f['x'] - truth[k])[free] / f['err'][free]).tolist())
    rms = float(np.sqrt(np.mean(np.square(pulls))))
    print('back=%d: restart 0.3 px off agrees to %.2e sigma; SciPy evaluations %d - %d; rms pull of the exact-model '
          'stars %.2f' % (back, worst, min(nfev), max(nfev), rms))
    assert worst <= 1e-6
    assert 0.5 < rms < 2.0


@pytest.mark.parametrize('back', [False, True])
def test_fixed_shift_is_the_linear_solve(back):
    data, var, psf, truth, shift, fits = R.yardstick(back, True)
    for k, f in enumerate(fits):
        F, b = R.linear_solve(data[k], var[k], psf[k], shift[k, 0], shift[k, 1], back)
        assert abs(f['x'][0] - F) <= 1e-12 * abs(F)
        assert abs(f['x'][3] - b) <= 1e-12 * abs(F)
        assert np.array_equal(f['x'][1:3], shift[k]) and np.all(f['err'][1:3] == 0)


def test_argument_validation():
    from muse_psfr_amd import _lib
    psf = np.ones((3, 40, 40))
    ps, ix, sh, flags = _lib.psf_fit_arguments(3, psf, None, None, True, False)
    assert ps.shape == (3, 40, 40) and ix is None and sh is None and flags == _lib.FIT_BACKGROUND
    ps, ix, sh, flags = _lib.psf_fit_arguments(5, psf, [0, 2, 1, 1, 0], np.zeros((5, 2)), False, True)
    assert ix.dtype == np.int32 and ix.tolist() == [0, 2, 1, 1, 0] and sh.shape == (5, 2)
    assert flags == _lib.FIT_FIXED_SHIFT == 4 and _lib.NFIT_PSF == 16
    bad = (dict(nstamp=2, psf_index=None),                                  # npsf != nstamp
           dict(psf_index=[0, 1, 3]), dict(psf_index=[0, -1, 1]), dict(psf_index=[0, 1]),
           dict(psf_index=[0.0, 1.0, 2.0]),
           dict(shift=np.full((3, 2), np.nan)), dict(shift=np.full((3, 2), 8.5)), dict(shift=np.zeros((2, 2))),
           dict(shift=np.zeros(6)), dict(fixed_shift=True), dict(background=1), dict(fixed_shift=0),
           dict(psf=np.ones((3, 40, 39))), dict(psf=np.ones((0, 40, 40))))
    for kw in bad:
        args = dict(nstamp=3, psf=psf, psf_index=None, shift=None, background=True, fixed_shift=False)
        args.update(kw)
        with pytest.raises(ValueError):
            _lib.psf_fit_arguments(**args)
    assert 'mpsfr_fit_stamps_psf' in _lib.EXPORTS
    import muse_psfr_amd
    assert muse_psfr_amd.NFIT_PSF == 16 and muse_psfr_amd.FIT_FIXED_SHIFT == 4
    assert callable(muse_psfr_amd.fit_stars_with_psf)
