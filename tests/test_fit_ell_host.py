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


# ---- the fp64 yardstick of tests/test_gpu_fit_ell_columns.py
def test_fit_full_on_an_exact_stamp_returns_the_truth():
    e1, e2 = M.e_from_ratio(0.7, 30.0)
    truth = np.array([1.3, 19.3, 20.6, 6.0, e1, e2, 1.0 / 2.5])
    full = M.fit_full(M.stamp(1.3, 19.3, 20.6, 6.0, 0.7, 30.0, 2.5))
    assert np.abs(full['v'] - truth).max() <= 1e-9
    assert full['chi2'] < 1e-24
    al = 6.0 / (2 * np.sqrt(2 ** 0.4 - 1))
    assert abs(full['flux'] - 1.3 * np.pi * al * al / 1.5) <= 1e-9 * full['flux']
    assert abs(full['alpha_major'] * full['alpha_minor'] - al * al) <= 1e-9 * al * al
    assert abs(full['alpha_minor'] / full['alpha_major'] - 0.7) <= 1e-9
    np.testing.assert_allclose(M.v_from_row(_row_of(full)), full['v'], rtol=0, atol=1e-12)


def _row_of(full):
    row = np.zeros(_lib.NFIT_ELL)
    for k, j in M.COLUMN.items():
        if k in full:
            row[j] = full[k]
    return row


@pytest.mark.parametrize('ba,rot', [(0.7, 30.0), (0.98, 120.0), (0.3, 100.0)])
def test_numerical_gradient_against_the_analytic_one_of_fwhm_major(ba, rot):
    """fwhm_major = w f, f = ((1 + e)/(1 - e))^(1/4): d/dw = f, d/de_k = w f e_k / (2 e (1 - e^2))."""
    e1, e2 = M.e_from_ratio(ba, rot)
    v = np.array([1.0, 19.7, 20.2, 5.0, e1, e2, 0.4])
    e = np.hypot(e1, e2)
    f = ((1 + e) / (1 - e)) ** 0.25
    want = np.array([0, 0, 0, f, 5.0 * f * e1 / (2 * e * (1 - e * e)), 5.0 * f * e2 / (2 * e * (1 - e * e)), 0])
    got = M.num_gradient('fwhm_major', v)
    assert np.abs(got - want).max() <= 1e-7 * np.abs(want).max(), (got, want)
    # rot across its branch cut (e2 = 0, e1 < 0): the differences are taken modulo 180 degrees
    vc = np.array([1.0, 19.7, 20.2, 5.0, -0.3, 0.0, 0.4])
    g = M.num_gradient('rot', vc)
    assert abs(g[5] - np.rad2deg(0.5 / -0.3)) <= 1e-7 * abs(g[5]) and abs(g[4]) <= 1e-7 * abs(g[5])


def _symmetric_cases():
    """Round Moffats (peak 1, n 2.5, FWHM 3 and 8) at the stamp's centre of symmetry (19.5, 19.5) plus a perturbation
    of 1e-3 of the peak with the eight symmetries of the square: a concentric wide Moffat, or the seeded noise field of
    tail_ref.perturbed_cases averaged over its flips and transposes.  e = 0 is then a stationary point of the
    7-variable fit, and J^T J is block diagonal between (e1, e2) and the five circular variables."""
    import tail_ref as T
    rng = np.random.default_rng(77)
    noise = rng.standard_normal((40, 40))
    noise = sum(a for t in (noise, noise.T) for a in (t, t[::-1], t[:, ::-1], t[::-1, ::-1])) / 8.0
    noise *= 1e-3 / np.abs(noise).max()
    out = []
    for fw in (3.0, 8.0):
        base = T.moffat_stamp(1.0, 19.5, 19.5, fw, 2.5)
        out.append(('wide_fwhm%g' % fw, fw, base + T.moffat_stamp(1e-3, 19.5, 19.5, 2.5 * fw, 1.8)))
        out.append(('noise_fwhm%g' % fw, fw, base + noise))
    return out


def test_circular_columns_agree_with_the_circular_reference_at_e_0():
    """A 5-variable MINPACK fit (tail_ref.fit) against the 7-variable fit_full of the same stamp.  The perturbed
    stamps of tail_ref are not symmetric, so a free (e1, e2) leaves e = 0 on them and the two fits have different
    minima; the stamps here are theirs made symmetric (_symmetric_cases), where e stays 0 by construction.  The shared
    columns then differ by the degrees of freedom alone (1600 - 5 against 1600 - 7 under the square root)."""
    import tail_ref as T
    dof = np.sqrt((1600.0 - 5) / (1600.0 - 7))
    for name, fw, st in _symmetric_cases():
        c = T.fit(st, (1.0, 19.5, 19.5, fw, 2.5))
        full = M.fit_full(st, (1.0, 19.5, 19.5, fw, 0.0, 0.0, 0.4))
        assert np.hypot(full['v'][4], full['v'][5]) <= 1e-12, name
        for k in ('peak', 'p0', 'q0', 'n', 'flux', 'chi2'):
            assert abs(full[k] - c[k]) <= 1e-6 * abs(c[k]), (name, k, full[k], c[k])
        for k in ('err_peak', 'err_p0', 'err_q0', 'err_n'):
            assert abs(full[k] - c[k] * dof) <= 1e-6 * c[k], (name, k, full[k], c[k] * dof)
        assert abs(full['err_fwhm_major'] - c['err_fwhm'] * dof) <= 1e-6 * c['err_fwhm']
        assert abs(full['err_fwhm_minor'] - c['err_fwhm'] * dof) <= 1e-6 * c['err_fwhm']


@pytest.mark.parametrize('fw,n', [(2.0, 8.0), (5.0, 2.5), (8.0, 20.0), (20.0, 8.0), (3.0, 1.5)])
def test_kappa_is_the_circular_one_at_b_over_a_1(fw, n):
    import tail_ref as T
    for c in ((19.5, 19.5), (19.7, 20.4)):
        k7 = M.kappa((1.0, c[0], c[1], fw, 0.0, 0.0, 1.0 / n))
        k5 = T.kappa(1.0, c[0], c[1], fw, n)
        assert abs(k7 - k5) <= 0.01 * k5, (c, k7, k5)


def test_every_perturbed_case_has_one_minimum():
    """16 cases; three starts reach the same minimum; the minimum is well conditioned (kappa below the flag's
    threshold) and err_rot is far from its cap, so the error columns are those of a plain first-order propagation."""
    refs = M.perturbed_references()
    assert len(refs) == 16 and len({n for n, _, _, _ in refs}) == 16
    for name, st, full, spread in refs:
        a, b = np.unravel_index(st.argmax(), st.shape)
        assert min(a, 39 - a, b, 39 - b) == (4 if name.endswith('rm4') else 19), name
        assert spread <= 1e-8, (name, spread)
        assert full['kappa'] < 100 and full['cond'] < 1e4, (name, full['kappa'], full['cond'])
        assert 0.0 < full['err_rot'] < 18.0, (name, full['err_rot'])
        assert full['chi2'] > 1e-8, name
    print('perturbed: kappa %.3g .. %.3g, cond <= %.3g, err_rot %.3g .. %.3g deg, spread <= %.3g' % (
        min(f['kappa'] for _, _, f, _ in refs), max(f['kappa'] for _, _, f, _ in refs),
        max(f['cond'] for _, _, f, _ in refs), min(f['err_rot'] for _, _, f, _ in refs),
        max(f['err_rot'] for _, _, f, _ in refs), max(s for _, _, _, s in refs)))
