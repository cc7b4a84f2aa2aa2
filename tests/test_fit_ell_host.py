"""CPU: the elliptical Moffat fit (mpsfr_fit_stamps_elliptical, fit_psf_cube(circular=False), circular=False of
compute_field_psf / compute_profile_psf): the header and the binding agree, the column builder, refusals before any
GPU context exists, and the SciPy yardstick of the GPU tests recovers exact model parameters."""
import os
import re

import numpy as np
import pytest

import moffat_ell_ref as M
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec


@pytest.fixture
def no_context(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('a GPU context was requested before the arguments were checked')
    monkeypatch.setattr(psfrec, 'get_context', refuse)


def test_header_constant_and_symbol():
    src = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    assert int(re.search(r'#define MPSFR_NFIT_ELL\s+(\d+)', src).group(1)) == _lib.NFIT_ELL == 24
    body = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'int mpsfr_fit_stamps_elliptical\(mpsfr_ctx\* ctx, int nstamp, const double\* stamps, '
                     r'double\* fit_out, int on_device\);', body)
    assert 'mpsfr_fit_stamps_elliptical' in _lib.EXPORTS
    import muse_psfr_amd
    assert muse_psfr_amd.NFIT_ELL == 24


def test_elliptical_columns_from_fit_rows():
    rng = np.random.default_rng(3)
    n, ps = 4, 0.025
    f = rng.uniform(0.5, 3.0, (n, _lib.NFIT_ELL))
    lb = np.linspace(490.0, 930.0, n)
    cols = psfrec._fit_columns_ell(lb, f, ps)
    assert tuple(cols) == psfrec._FIT_COLS_ELL == ('lbda', 'center', 'flux', 'fwhm', 'n', 'rot', 'peak', 'err_center',
                                                   'err_flux', 'err_fwhm', 'err_n', 'err_rot', 'err_peak')
    np.testing.assert_array_equal(cols['lbda'], lb)
    np.testing.assert_array_equal(cols['center'], f[:, 1:3])
    np.testing.assert_array_equal(cols['flux'], f[:, 19])
    np.testing.assert_array_equal(cols['fwhm'], f[:, 7:9] * ps)
    np.testing.assert_array_equal(cols['n'], f[:, 5])
    np.testing.assert_array_equal(cols['rot'], f[:, 6])
    np.testing.assert_array_equal(cols['peak'], f[:, 0])
    np.testing.assert_array_equal(cols['err_center'], f[:, 12:14])
    np.testing.assert_array_equal(cols['err_flux'], f[:, 20])
    np.testing.assert_array_equal(cols['err_fwhm'], f[:, 14:16] * ps)
    np.testing.assert_array_equal(cols['err_n'], f[:, 17])
    np.testing.assert_array_equal(cols['err_rot'], f[:, 16])
    np.testing.assert_array_equal(cols['err_peak'], f[:, 11])
    assert cols['fwhm'].shape == cols['err_fwhm'].shape == (n, 2)
    # the field form: dir_idx, x, y, then these columns
    pos = np.array([[0.0, 0.0], [30.0, -10.0]])
    fc = psfrec._field_columns(lb[:2], pos, f.reshape(2, 2, -1), ps, psfrec._fit_columns_ell)
    assert tuple(fc) == ('dir_idx', 'x', 'y') + psfrec._FIT_COLS_ELL
    np.testing.assert_array_equal(fc['rot'], f[:, 6])
    # the circular table is unchanged
    assert psfrec._FIT_COLS == ('lbda', 'center', 'flux', 'fwhm', 'n', 'peak', 'err_center', 'err_flux', 'err_fwhm',
                                'err_n', 'err_peak')


GOOD = np.ones((2, 40, 40))


@pytest.mark.parametrize('kw', [dict(psfcube=np.ones((2, 30, 30))), dict(psfcube=np.ones((2, 40, 41))),
                                dict(psfcube=np.ones(40)), dict(psfcube=np.ones((0, 40, 40))),
                                dict(psfcube=np.where(np.eye(40, dtype=bool)[None], np.nan, GOOD)),
                                dict(psfcube=np.where(np.eye(40, dtype=bool)[None], np.inf, GOOD)),
                                dict(circular='no'), dict(circular=0), dict(circular=None),
                                dict(lbda=[600.0])])
def test_fit_psf_cube_refuses_before_any_context(no_context, kw):
    args = dict(lbda=[600.0, 700.0], psfcube=GOOD, circular=False)
    args.update(kw)
    with pytest.raises(ValueError):
        psfrec.fit_psf_cube(args.pop('lbda'), args.pop('psfcube'), **args)


@pytest.mark.parametrize('circular', ['false', 1, None, np.array([True, False])])
def test_field_and_profile_refuse_a_non_bool_circular(no_context, circular):
    with pytest.raises(ValueError):
        psfrec.compute_field_psf([600.0], 1.0, 0.7, 25.0, verbose=False, circular=circular)
    with pytest.raises(ValueError):
        psfrec.compute_profile_psf([600.0], 1.0, 25.0, [0.7, 0.3], [100.0, 10000.0], verbose=False,
                                   circular=circular)


def test_elliptical_stamps_refusals_in_the_binding():
    with pytest.raises(ValueError):
        _lib.elliptical_stamps(np.ones((3, 40, 39)))
    with pytest.raises(ValueError):
        _lib.elliptical_stamps(np.full((1, 40, 40), np.nan))
    with pytest.raises(ValueError):
        _lib.elliptical_stamps('stamps')
    st = _lib.elliptical_stamps(np.ones((2, 3, 40, 40), dtype=np.float32))
    assert st.shape == (6, 40, 40) and st.dtype == np.float64 and st.flags.c_contiguous


@pytest.mark.parametrize('par', [(1.0, 19.3, 20.6, 6.0, 0.7, 30.0, 2.5), (2.0, 20.0, 19.0, 4.0, 0.95, 135.0, 4.0),
                                 (0.5, 21.2, 18.4, 9.0, 0.5, 170.0, 1.6), (1.0, 20.0, 20.0, 5.0, 1.0, 0.0, 8.0)])
def test_reference_fit_recovers_exact_parameters(par):
    peak, p0, q0, fw, ba, rot, n = par
    d = M.stamp(peak, p0, q0, fw, ba, rot, n)
    v = M.fit(d)
    got = M.derived(v)
    e1, e2 = M.e_from_ratio(ba, rot)
    f = ((1 + np.hypot(e1, e2)) / (1 - np.hypot(e1, e2))) ** 0.25
    want = dict(peak=peak, p0=p0, q0=q0, fwhm_major=fw * f, fwhm_minor=fw / f, n=n)
    for k, w in want.items():
        assert abs(got[k] - w) <= 1e-9 * abs(w), (k, got[k], w)
    if ba < 1:
        assert (1 - ba) * M.rot_diff(got['rot'], rot) <= 1e-9
    else:
        assert abs(1 - got['ba']) <= 1e-9


def test_reference_jacobian_matches_finite_differences():
    v = np.array([1.3, 19.6, 20.2, 5.5, 0.12, -0.07, 0.35])
    _, J = M.model(v, jac=True)
    for k in range(7):
        h = 1e-6 * max(1.0, abs(v[k]))
        vp, vm = v.copy(), v.copy()
        vp[k] += h
        vm[k] -= h
        fd = (M.model(vp) - M.model(vm)) / (2 * h)
        assert np.abs(fd - J[:, k]).max() <= 1e-6 * np.abs(J[:, k]).max(), k
