"""CPU: the weighted Moffat fit of observed stars (mpsfr_fit_stamps_observed, Context.fit_stamps_observed,
fit_psf_cube(var=..., fit_back=...)): the header and the binding agree, the argument checks and column names hold
before any GPU context exists, and the SciPy yardstick of the GPU tests (moffat_obs_ref) is sound on the very stamps
the GPU test uses: it reaches the same minimum from the data-driven start and from the true parameters, with
method='lm' and method='trf', and its formal errors describe the scatter about the truth."""
import os
import re

import numpy as np
import pytest

import moffat_obs_ref as R
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec


@pytest.fixture
def no_context(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('a GPU context was requested before the arguments were checked')
    monkeypatch.setattr(psfrec, 'get_context', refuse)


def test_header_constants_and_symbol():
    src = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    assert int(re.search(r'#define MPSFR_FIT_BACKGROUND\s+(\d+)', src).group(1)) == _lib.FIT_BACKGROUND == 1
    assert int(re.search(r'#define MPSFR_FIT_ELLIPTICAL\s+(\d+)', src).group(1)) == _lib.FIT_ELLIPTICAL == 2
    body = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'int mpsfr_fit_stamps_observed\(mpsfr_ctx\* ctx, int nstamp, const double\* stamps, '
                     r'const double\* var, int flags,\s+double\* fit_out, int on_device\);', body)
    assert 'mpsfr_fit_stamps_observed' in _lib.EXPORTS
    import muse_psfr_amd
    assert muse_psfr_amd.FIT_BACKGROUND == 1 and muse_psfr_amd.FIT_ELLIPTICAL == 2
    assert hasattr(muse_psfr_amd.Context, 'fit_stamps_observed')
    assert hasattr(muse_psfr_amd.Context, 'fit_stamps_observed_device')


def test_flags_from_booleans():
    assert _lib.observed_flags(False, True) == 0
    assert _lib.observed_flags(True, True) == 1
    assert _lib.observed_flags(False, False) == 2
    assert _lib.observed_flags(True, False) == 3
    for bad in (1, 'yes', None):
        with pytest.raises(ValueError):
            _lib.observed_flags(bad, True)
        with pytest.raises(ValueError):
            _lib.observed_flags(True, bad)


def test_observed_stamps_in_the_binding():
    d = np.ones((2, 3, 40, 40), dtype=np.float32)
    st, va = _lib.observed_stamps(d)
    assert va is None and st.shape == (6, 40, 40) and st.dtype == np.float64 and st.flags.c_contiguous
    d2 = np.ones((3, 40, 40))
    d2[1, 4, 5] = np.nan
    d2[2, 0, 0] = np.inf
    st, va = _lib.observed_stamps(d2, np.full((3, 40, 40), -1.0))          # non-finite data and bad variances pass
    assert np.isnan(st[1, 4, 5]) and np.isinf(st[2, 0, 0]) and va.shape == (3, 40, 40)
    ma = np.ma.MaskedArray(np.ones((1, 40, 40)), mask=np.eye(40, dtype=bool)[None])
    st, _ = _lib.observed_stamps(ma)
    assert np.isnan(st[0][np.eye(40, dtype=bool)]).all() and np.isfinite(st).sum() == 1600 - 40
    for bad in (np.ones((3, 40, 39)), np.ones(40), np.ones((0, 40, 40)), 'stamps'):
        with pytest.raises(ValueError):
            _lib.observed_stamps(bad)
    for badvar in (np.ones((2, 40, 40)), np.ones((3, 40, 39)), 'var'):
        with pytest.raises(ValueError):
            _lib.observed_stamps(np.ones((3, 40, 40)), badvar)


def test_observed_columns_from_fit_rows():
    rng = np.random.default_rng(4)
    n, ps = 3, 0.2
    f = rng.uniform(0.5, 3.0, (n, _lib.NFIT_ELL))
    f[:, 23] = [1600, 1571, 9]
    lb = np.linspace(500.0, 900.0, n)
    ce = psfrec._fit_columns_obs(lb, f, ps, circular=False)
    assert tuple(ce) == psfrec._FIT_COLS_ELL + ('back', 'err_back', 'npix')
    cc = psfrec._fit_columns_obs(lb, f, ps, circular=True)
    assert tuple(cc) == psfrec._FIT_COLS + ('back', 'err_back', 'npix')
    for c in (ce, cc):
        np.testing.assert_array_equal(c['back'], f[:, 21])
        np.testing.assert_array_equal(c['err_back'], f[:, 22])
        np.testing.assert_array_equal(c['npix'], [1600, 1571, 9])
        assert c['npix'].dtype.kind == 'i'
        np.testing.assert_array_equal(c['fwhm'], f[:, 7:9] * ps)
        np.testing.assert_array_equal(c['err_fwhm'], f[:, 14:16] * ps)
        np.testing.assert_array_equal(c['n'], f[:, 5])
        np.testing.assert_array_equal(c['peak'], f[:, 0])
        np.testing.assert_array_equal(c['flux'], f[:, 19])
    np.testing.assert_array_equal(ce['rot'], f[:, 6])


GOOD = np.ones((2, 40, 40))


class _Cube:
    def __init__(self, data, var=None):
        self.data, self.var = data, var


@pytest.mark.parametrize('kw', [dict(psfcube=np.ones((2, 30, 30))), dict(psfcube=np.ones((0, 40, 40))),
                                dict(var=np.ones((2, 40, 39))), dict(var=np.ones((3, 40, 40))),
                                dict(var=True), dict(var=True, psfcube=_Cube(GOOD)),
                                dict(fit_back=1), dict(fit_back='yes'), dict(circular=0),
                                dict(lbda=[600.0])])
def test_fit_psf_cube_observed_refuses_before_any_context(no_context, kw):
    args = dict(lbda=[600.0, 700.0], psfcube=GOOD, var=np.ones((2, 40, 40)), fit_back=True)
    args.update(kw)
    with pytest.raises(ValueError):
        psfrec.fit_psf_cube(args.pop('lbda'), args.pop('psfcube'), **args)


def test_observed_cube_takes_mpdaf_style_objects():
    mask = np.zeros((2, 40, 40), dtype=bool)
    mask[0, 3, 4] = True
    cube = _Cube(np.ma.MaskedArray(GOOD.copy(), mask=mask), var=np.full((2, 40, 40), 0.5))
    st, va = psfrec._observed_cube(cube, True)
    assert np.isnan(st[0, 3, 4]) and np.isfinite(st).sum() == 3199 and np.all(va == 0.5)
    st, va = psfrec._observed_cube(cube, None)
    assert va is None and np.isnan(st[0, 3, 4])
    st, va = psfrec._observed_cube(np.ma.MaskedArray(GOOD.copy(), mask=mask), np.ones((2, 40, 40)))
    assert np.isnan(st[0, 3, 4]) and np.all(va == 1.0)


# ---- the yardstick on the inputs of the GPU test.  Bounds: the minimum found from the data-driven start, from the
# true parameters and by the trust-region method agree to 1e-5 of the formal error, and |fit - truth| / err has an rms
# in [0.8, 1.2].  Measured on these 4 x 40 stamps (the figures DESIGN.md section 17 quotes): start to start
# <= 1.5e-6, lm against trf <= 8.1e-7, reduced chi2 0.91 ... 1.10, rms pull 0.97 ... 1.06.
@pytest.mark.parametrize('ell,back', R.VARIANTS)
def test_yardstick_on_the_noisy_stamps(ell, back):
    data, var, truth = R.noisy_stamps(ell, back)
    free = R.free_indices(ell, back)
    spread = lmtrf = 0.0
    pulls, red = [], []
    for d, va, t in zip(data, var, truth):
        a = R.fit(d, va, ell, back)
        b = R.fit(d, va, ell, back, v0=t)
        c = R.fit(d, va, ell, back, method='trf')
        assert a['status'] > 0 and b['status'] > 0 and c['status'] > 0
        assert a['npix'] == np.count_nonzero(np.isfinite(d) & (va > 0)) and 1500 < a['npix'] < 1600
        spread = max(spread, np.max(np.abs(a['x'] - b['x'])[free] / a['err'][free]))
        lmtrf = max(lmtrf, np.max(np.abs(a['x'] - c['x'])[free] / a['err'][free]))
        pulls.append((a['x'] - t)[free] / a['err'][free])
        red.append(a['redchi2'])
    rms = float(np.sqrt(np.mean(np.square(pulls))))
    print('ell %d back %d: start spread %.2e sigma, lm vs trf %.2e sigma, reduced chi2 %.3f ... %.3f, rms pull %.3f'
          % (ell, back, spread, lmtrf, min(red), max(red), rms))
    assert spread <= 1e-5, spread
    assert lmtrf <= 1e-5, lmtrf
    assert 0.8 <= rms <= 1.2, rms


def test_yardstick_errors_do_not_depend_on_the_scale_of_var():
    data, var, _ = R.noisy_stamps(True, True, count=2)
    for d, va in zip(data, var):
        a, b = R.fit(d, va, True, True), R.fit(d, 4.0 * va, True, True)
        np.testing.assert_allclose(a['x'], b['x'], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(a['verr'], b['verr'], rtol=1e-6)
        assert abs(a['chi2'] / b['chi2'] - 4.0) < 1e-9


def test_yardstick_derived_errors_against_the_closed_forms():
    """n = 1 / eta and the background are single variables: their propagated errors are known in closed form."""
    data, var, _ = R.noisy_stamps(True, True, count=1)
    a = R.fit(data[0], var[0], True, True)
    k = {key: i for i, key in enumerate(R.KEYS)}
    assert abs(a['verr'][k['n']] - a['err'][6] / a['x'][6] ** 2) <= 1e-6 * a['verr'][k['n']]
    assert abs(a['verr'][k['back']] - a['err'][7]) <= 1e-6 * a['err'][7]
    assert abs(a['verr'][k['p0']] - a['err'][1]) <= 1e-6 * a['err'][1]
