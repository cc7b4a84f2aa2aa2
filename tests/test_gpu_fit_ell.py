"""GPU: the elliptical Moffat fit (mpsfr_fit_stamps_elliptical), both precisions.

1. exact model stamps over axis ratio, orientation, n, FWHM and centre: the parameters come back;
2. the reference's own stamps (tests/golden/g9_profile*.npz) against an fp64 SciPy fit of the same model;
3. round stamps (exact circular Moffats, reconstructed stamps made 4-fold symmetric) give the circular fit;
4. symmetry: a transposed stamp / a stamp with its rows reversed maps (p0, q0, rot) as it should;
5. plumbing: batches, device pointers, a device-output reconstruct chained into the fit, a few thousand stamps,
   compute_field_psf / compute_profile_psf(circular=False), an all-zero stamp.
Margins go to record_margin('fit_ell', ...) as error / tolerance.
"""
import numpy as np
import pytest

import moffat_ell_ref as M
from conftest import H, record_margin

pytestmark = pytest.mark.gpu

TOL = {'f64': 1e-8, 'mixed': 1e-4}
PARITY = {'f64': 1e-6, 'mixed': 1e-4}
PRECS = ['mixed', 'f64']


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


_CTX = {}


@pytest.fixture
def ctx(api, prec):
    if prec not in _CTX:
        _CTX[prec] = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision=prec)
    return _CTX[prec]


def _synthetic_grid(seed=11):
    rng = np.random.default_rng(seed)
    pars = []
    for ba in (1.0, 0.99, 0.9, 0.7, 0.5):
        for rot in (0.0, 30.0, 75.0, 90.0, 135.0, 170.0):
            if ba == 1.0 and rot != 0.0:
                continue
            for n in (1.6, 2.5, 4.0, 8.0):
                for fw in (3.0, 6.0, 12.0):
                    p0, q0 = 19.5 + rng.uniform(-2, 2, 2)
                    pars.append((rng.uniform(0.5, 2.0), p0, q0, fw, ba, rot, n))
    return pars


def _want(par):
    peak, p0, q0, fw, ba, rot, n = par
    return dict(peak=peak, p0=p0, q0=q0, fwhm_major=fw / np.sqrt(ba), fwhm_minor=fw * np.sqrt(ba), n=n, rot=rot,
                ba=ba)


def _compare(got, want, tol, keys=('fwhm_major', 'fwhm_minor', 'n', 'p0', 'q0')):
    """Worst error / tol over keys (relative) and over rot ((1 - b/a) |d rot| in radians, skipped when b/a = 1)."""
    worst = {}
    for k in keys:
        worst[k] = abs(got[k] - want[k]) / abs(want[k]) / tol
    if want['ba'] < 1.0:
        worst['rot'] = (1.0 - want['ba']) * M.rot_diff(got['rot'], want['rot']) / tol
    return worst


# ---- 1. synthetic recovery
@pytest.mark.parametrize('prec', PRECS)
def test_synthetic_recovery(ctx, prec):
    pars = _synthetic_grid()
    st = np.array([M.stamp(*p) for p in pars])
    fit = ctx.fit_stamps_elliptical(st)
    assert fit.shape == (len(pars), 24)
    assert np.all(fit[:, 18].astype(int) & 3 == 0), fit[:, 18]
    worst = {}
    for p, row in zip(pars, fit):
        w = _compare(M.gpu_derived(row), _want(p), TOL[prec])
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    record_margin('fit_ell', **{'synthetic_%s_%s' % (prec, k): v for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    assert np.all(fit[:, 21:] == 0.0)


# ---- 2. the reference's stamps against an fp64 SciPy fit
def _reference_stamps(golden):
    g, gd = golden('g9_profile'), golden('g9_profile_field')
    return {'a': g['a_fin'], 'b': g['b_fin'], 'c': g['c_fin'], 'd': gd['d_fin'].reshape(-1, 40, 40)}


_SCIPY = {}


def _scipy_fits(golden):
    if not _SCIPY:
        for case, st in _reference_stamps(golden).items():
            _SCIPY[case] = [M.derived(M.fit(s)) for s in st]
    return _SCIPY


@pytest.mark.parametrize('prec', PRECS)
def test_reference_stamps_against_scipy(ctx, prec, golden):
    refs = _scipy_fits(golden)
    worst = {}
    for case, st in _reference_stamps(golden).items():
        fit = ctx.fit_stamps_elliptical(st)
        assert np.all(fit[:, 18].astype(int) & 3 == 0), (case, fit[:, 18])
        for row, want in zip(fit, refs[case]):
            w = _compare(M.gpu_derived(row), want, PARITY[prec], keys=('fwhm_major', 'fwhm_minor', 'n'))
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0.0), v)
        if case == 'd':
            rows = fit.reshape(5, 5, 24)                 # (position, wavelength)
            for p in range(5):
                ba = rows[p, :, 8] / rows[p, :, 7]
                assert np.all((ba >= 0.97) & (ba < 1.0)), (p, ba)
                rot = rows[p, :, 6]
                spread = max(np.rad2deg(M.rot_diff(a, b)) for a in rot for b in rot)
                assert spread <= 6.0, (p, rot)
    record_margin('fit_ell', **{'scipy_%s_%s' % (prec, k): v for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


# ---- 3. round stamps give the circular answer
def _symmetrise(s):
    """Mean of the eight flips / transposes of a stamp about pixel (20, 20) (i -> 40 - i, row 0 fixed)."""
    r = lambda a, ax: np.roll(np.flip(a, ax), 1, ax)      # noqa: E731
    out = []
    for t in (s, s.T):
        for a in (t, r(t, 0)):
            out += [a, r(a, 1)]
    return np.mean(out, axis=0)


def _against_circular(fe, fc, tol, tol_ba, axes=('fwhm_major', 'fwhm_minor')):
    """Worst error / tol of the elliptical rows fe against the circular rows fc, and (1 - b/a) / tol_ba."""
    worst = {}
    for re_, rc in zip(fe, fc):
        got = {'peak': re_[0], 'p0': re_[1], 'q0': re_[2], 'n': re_[5], 'fwhm_major': re_[7], 'fwhm_minor': re_[8],
               'fwhm_geo': np.sqrt(re_[7] * re_[8])}
        want = {'peak': rc[0], 'p0': rc[1], 'q0': rc[2], 'n': rc[4], 'fwhm_major': rc[5], 'fwhm_minor': rc[5],
                'fwhm_geo': rc[5]}
        for k in ('peak', 'p0', 'q0', 'n') + axes:
            worst[k] = max(worst.get(k, 0.0), abs(got[k] - want[k]) / abs(want[k]) / tol)
        worst['1-b/a'] = max(worst.get('1-b/a', 0.0), (1.0 - re_[8] / re_[7]) / tol_ba)
    return worst


@pytest.mark.parametrize('prec', PRECS)
def test_round_stamps_give_the_circular_fit(ctx, prec, golden):
    rng = np.random.default_rng(5)
    circ = np.array([M.stamp(rng.uniform(0.5, 2), *(19.5 + rng.uniform(-2, 2, 2)), fw, 1.0, 0.0, n)
                     for n in (1.6, 2.5, 4.0, 8.0) for fw in (3.0, 6.0, 12.0)])
    refs = _reference_stamps(golden)
    sym = np.array([_symmetrise(s) for s in np.concatenate([refs['a'], refs['d'][:10]])])
    tol_ba = 1e-6 if prec == 'f64' else 1e-4
    # exact circular Moffats: the circular fit's answer to the tolerance of the synthetic recovery
    w = _against_circular(ctx.fit_stamps_elliptical(circ), ctx.fit_stamps(circ), TOL[prec], tol_ba)
    record_margin('fit_ell', **{'round_exact_%s_%s' % (prec, k): v for k, v in w.items()})
    assert max(w.values()) <= 1.0, w
    # 4-fold symmetric reconstructed stamps.  The symmetry makes e = 0 a stationary point, not necessarily the
    # minimum: a square-ish stamp can be fitted marginally better by four equivalent diagonal ellipses (SciPy finds
    # b/a = 1 - 2.7e-7 at 135 degrees on the first one).  So: b/a within tol_ba of 1; peak, centre, n and the
    # geometric-mean FWHM (which moves by O(e^2)) the circular fit's; the axes the fp64 SciPy fit's.
    fe = ctx.fit_stamps_elliptical(sym)
    w = _against_circular(fe, ctx.fit_stamps(sym), TOL[prec], tol_ba, axes=('fwhm_geo',))
    record_margin('fit_ell', **{'round_sym_%s_%s' % (prec, k): v for k, v in w.items()})
    assert max(w.values()) <= 1.0, w
    worst = 0.0
    for row, s in zip(fe, sym):
        want, got = M.derived(M.fit(s)), M.gpu_derived(row)
        for k in ('fwhm_major', 'fwhm_minor'):
            worst = max(worst, abs(got[k] - want[k]) / abs(want[k]) / TOL[prec])
    record_margin('fit_ell', **{'round_sym_scipy_%s_axes' % prec: worst})
    assert worst <= 1.0


# ---- 4. symmetry
@pytest.mark.parametrize('prec', PRECS)
def test_transpose_and_row_reversal(ctx, prec, golden):
    refs = _reference_stamps(golden)
    syn = [M.stamp(1.0, 19.2, 20.7, 5.0, 0.8, 30.0, 2.5), M.stamp(1.5, 20.9, 18.6, 8.0, 0.6, 112.0, 3.5)]
    st = np.concatenate([refs['d'][::5], np.array(syn)])
    f0 = ctx.fit_stamps_elliptical(st)
    ft = ctx.fit_stamps_elliptical(np.transpose(st, (0, 2, 1)).copy())
    fr = ctx.fit_stamps_elliptical(st[:, ::-1, :].copy())
    tol = 1e-9 if prec == 'f64' else TOL[prec]
    worst = 0.0
    for a, t, r in zip(f0, ft, fr):
        ba = a[8] / a[7]
        for k in (0, 5, 7, 8):                       # peak, n, fwhm_major, fwhm_minor
            worst = max(worst, abs(t[k] - a[k]) / abs(a[k]) / tol, abs(r[k] - a[k]) / abs(a[k]) / tol)
        worst = max(worst, abs(t[1] - a[2]) / a[2] / tol, abs(t[2] - a[1]) / a[1] / tol)
        worst = max(worst, abs(r[1] - (39.0 - a[1])) / a[1] / tol, abs(r[2] - a[2]) / a[2] / tol)
        worst = max(worst, (1 - ba) * M.rot_diff(t[6], 90.0 - a[6]) / tol,
                    (1 - ba) * M.rot_diff(r[6], 180.0 - a[6]) / tol)
    record_margin('fit_ell', **{'symmetry_%s' % prec: worst})
    assert worst <= 1.0


# ---- 5. plumbing
@pytest.mark.parametrize('prec', PRECS)
def test_batch_single_and_device_forms(ctx, prec, golden):
    import torch
    st = _reference_stamps(golden)['b']
    batch = ctx.fit_stamps_elliptical(st)
    for k in range(len(st)):
        assert np.array_equal(ctx.fit_stamps_elliptical(st[k]), batch[k:k + 1]), k
    dev = torch.device('cuda:0')
    ts = torch.from_numpy(np.ascontiguousarray(st)).to(dev)
    tf = torch.full((len(st), 24), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_stamps_elliptical_device(len(st), ts.data_ptr(), tf.data_ptr())
    ctx.sync()
    assert np.array_equal(tf.cpu().numpy(), batch)


@pytest.mark.parametrize('prec', PRECS)
def test_reconstruct_field_device_chained_into_the_fit(api, prec):
    import torch
    dim = 256
    ps = api.grid_pixscale(dim)
    lb = np.array([500.0, 700.0, 900.0])
    see, gl, l0, three = np.array([1.0, 0.8]), np.array([0.7, 0.5]), np.array([25.0, 20.0]), np.array([0, 1])
    pos = np.array([[0.0, 0.0], [30.0, 0.0], [-20.0, 40.0]])
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    ref = ctx.reconstruct_field(lb, see, gl, l0, three, H, pos)
    dev = torch.device('cuda:0')
    tp = torch.empty(ref['psf'].shape, dtype=torch.float64, device=dev)
    ts = torch.empty(ref['psf_sum'].shape, dtype=torch.float64, device=dev)
    tf = torch.empty(ref['fit'].shape, dtype=torch.float64, device=dev)
    nst = int(np.prod(ref['psf'].shape[:-2]))
    te = torch.empty((nst, 24), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.reconstruct_field_device(lb, see, gl, l0, three, H, 12.0, pos, None, tp.data_ptr(), ts.data_ptr(),
                                 tf.data_ptr())
    ctx.fit_stamps_elliptical_device(nst, tp.data_ptr(), te.data_ptr())
    ctx.sync()
    assert np.array_equal(tp.cpu().numpy(), ref['psf'])
    assert np.array_equal(te.cpu().numpy(), ctx.fit_stamps_elliptical(ref['psf']))
    ctx.close()


@pytest.mark.parametrize('prec', PRECS)
def test_a_few_thousand_stamps(ctx, prec):
    rng = np.random.default_rng(7)
    n = 3000
    pars = [(rng.uniform(0.5, 2), *(19.5 + rng.uniform(-2, 2, 2)), rng.uniform(3, 10), rng.uniform(0.6, 1.0),
             rng.uniform(0, 180), rng.uniform(1.8, 5)) for _ in range(n)]
    st = np.array([M.stamp(*p) for p in pars])
    fit = ctx.fit_stamps_elliptical(st)
    assert fit.shape == (n, 24) and np.all(np.isfinite(fit))
    assert np.all(fit[:, 18].astype(int) & 3 == 0)
    for k in rng.choice(n, 40, replace=False):
        w = _compare(M.gpu_derived(fit[k]), _want(pars[k]), TOL[prec])
        assert max(w.values()) <= 1.0, (k, w)
    # the first stamps alone: the same rows
    assert np.array_equal(ctx.fit_stamps_elliptical(st[:5]), fit[:5])


@pytest.mark.parametrize('prec', PRECS)
def test_all_zero_stamp_is_singular(ctx, prec):
    st = np.zeros((3, 40, 40))
    st[1] = M.stamp(1.0, 20.0, 19.0, 5.0, 0.8, 40.0, 2.5)
    fit = ctx.fit_stamps_elliptical(st)
    assert not np.any(np.isnan(fit))
    assert int(fit[0, 18]) & 3 == 2 and int(fit[2, 18]) & 3 == 2
    assert int(fit[1, 18]) & 3 == 0


def test_compute_field_and_profile_psf_elliptical(api):
    lb = np.array([500.0, 750.0])
    dim = 512
    kw = dict(dim=dim, pixscale=api.grid_pixscale(dim), verbose=False)
    pos = [[0.0, 0.0], [30.0, 0.0], [-50.0, -50.0]]
    tc, pc = api.compute_field_psf(lb, 1.0, 0.7, 25.0, positions=pos, **kw)
    te, pe = api.compute_field_psf(lb, 1.0, 0.7, 25.0, positions=pos, circular=False, **kw)
    assert np.array_equal(pc, pe)
    from muse_psfr_amd import psfrec
    names = list(te.colnames if hasattr(te, 'colnames') else te.keys())
    assert names == ['dir_idx', 'x', 'y'] + list(psfrec._FIT_COLS_ELL) + ['SEEING', 'GL', 'L0']
    assert np.asarray(te['fwhm']).shape == (len(pos) * lb.size, 2)
    assert np.all(np.asarray(te['fwhm'])[:, 0] >= np.asarray(te['fwhm'])[:, 1])
    prof = dict(cn2=[0.6, 0.25, 0.15], h=[0.0, 1000.0, 10000.0], wind_speed=[8.0, 15.0, 30.0],
                wind_dir=[0.3, -1.0, 2.0])
    for p in (None, pos):
        tc, pc = api.compute_profile_psf(lb, 1.0, 25.0, positions=p, **prof, **kw)
        te, pe = api.compute_profile_psf(lb, 1.0, 25.0, positions=p, circular=False, **prof, **kw)
        assert np.array_equal(pc, pe)
        names = list(te.colnames if hasattr(te, 'colnames') else te.keys())
        lead = [] if p is None else ['dir_idx', 'x', 'y']
        assert names == lead + list(psfrec._FIT_COLS_ELL) + ['SEEING', 'GL', 'L0']
        ctx = psfrec.get_context(dim, kw['pixscale'], 40, 'mixed', 0)
        want = ctx.fit_stamps_elliptical(pe)
        np.testing.assert_array_equal(np.asarray(te['rot']), want[:, 6])
