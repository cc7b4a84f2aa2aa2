"""GPU: the PSF energy metrics (mpsfr_stamp_metrics: encircled / ensquared energy with exact pixel overlap, EE radii),
both precision contexts, against the fp64 NumPy reference tests/metrics_ref.py.

1. exact Moffat stamps (the grid of the elliptical-fit test) and the reference's own stamps (tests/golden/g9_profile*):
   flux, peak, centroid, every EE and ensquared energy.  Tolerance: the kernel and the reference are both fp64 sums of
   1600 products in different orders, 1600 x 2^-53 x sum|I| / flux ~ 2e-13, plus a few ulp of r^2 per overlap area from
   the different formulas (1e-12 at r = 60 px): 1e-10 absolute on the fractions, 1e-10 px on the centroid.
2. EE radii: metrics_ref.EE at the kernel's radius equals the fraction within 1e-9 (the stamps are exact Moffats, so
   non-negative: EE is monotone and the radius unique).
3. given centres; 'stamp' against 'centroid' on a 4-fold symmetric stamp.
4. symmetry under transposition and row reversal.
5. independence of the batch, device pointers, a device-output reconstruct chained into the metrics.
6. bad stamps (status 2, NaN energies, neighbours untouched) and the refusals (MPSFR_E_INVALID, `out` untouched).
7. the metrics= argument of the compute_* functions and the METRICS_* HDUs.
8. physical sanity of the reference's stamps.
Worst error / tolerance of 1-4 goes to record_margin('metrics', ...).  Recorded on an MI355X (both precision contexts
alike, the arithmetic is fp64 in both): EE 0.24 of the tolerance on the Moffat grid (its largest radii, where the two
overlap formulas differ by ulps of r^2 and arcsin loses digits near +-1), 3e-6 on the reference's stamps; ensquared
energy 7e-6; centroid 1e-4; flux 4e-6; EE radii 2e-5; symmetry 0.026.  The EE margin leaves no room to tighten 1e-10.
"""
import ctypes as C

import numpy as np
import pytest

import metrics_ref as R
import moffat_ell_ref as M
from conftest import H, record_margin

pytestmark = pytest.mark.gpu

PRECS = ['mixed', 'f64']
TOL_E = 1e-10          # energy fractions (absolute)
TOL_C = 1e-10          # centroid (pixels)
TOL_R = 1e-9           # |EE_ref(r_gpu) - f|
RADII = [0.3, 0.8, 1.0, 2.5, 4.0, 7.3, 13.0, 22.0, 31.0, 45.0, 80.0]     # sub-pixel ... beyond the stamp
BOXES = [0.3, 1.0, 2.0, 3.7, 8.0, 17.0, 40.0, 55.0, 80.0]
FRACS = [0.1, 0.5, 0.8, 0.95]
HEAD = 8


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
    """The grid of tests/test_gpu_fit_ell.py: b/a, orientation, n 1.6-8, FWHM 3-12 px, centres within 2 px of 19.5."""
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
    pars.append((1.0, 19.5, 19.5, 5.0, 1.0, 0.0, 2.5))               # centred
    pars.append((1.0, 20.0, 20.0, 3.0, 0.7, 45.0, 4.0))
    return pars


def _reference_stamps(golden):
    g, gd = golden('g9_profile'), golden('g9_profile_field')
    return np.concatenate([g['a_fin'], g['b_fin'], g['c_fin'], gd['d_fin'].reshape(-1, 40, 40)])


def _compare_rows(rows, stamps, radii, boxes, centers=None):
    """Worst error / tolerance of the head, EE and ensquared-energy fields of `rows` against metrics_ref."""
    worst = dict(flux=0.0, centroid=0.0, ee=0.0, sqe=0.0)
    for k, (row, st) in enumerate(zip(rows, stamps)):
        want = R.metrics(st, radii, boxes, (), None if centers is None else centers[k])
        assert row[6] == 0.0 and row[7] == 0.0, (k, row[:HEAD])
        assert row[1] == want['peak'] and (row[2], row[3]) == (want['peak_p'], want['peak_q']), (k, row[:HEAD])
        worst['flux'] = max(worst['flux'], abs(row[0] - want['flux']) / abs(want['flux']) / TOL_E)
        worst['centroid'] = max(worst['centroid'], np.abs(row[4:6] - want['center']).max() / TOL_C)
        worst['ee'] = max(worst['ee'], np.abs(row[HEAD:HEAD + len(radii)] - want['ee']).max() / TOL_E)
        worst['sqe'] = max(worst['sqe'], np.abs(row[HEAD + len(radii):] - want['sqe']).max() / TOL_E)
    return worst


# ---- 1. energies against the reference
@pytest.mark.parametrize('prec', PRECS)
def test_moffat_stamps_against_the_reference(ctx, prec):
    st = np.array([M.stamp(*p) for p in _synthetic_grid()])
    rows = ctx.stamp_metrics(st, RADII, BOXES, ())
    assert rows.shape == (len(st), HEAD + len(RADII) + len(BOXES))
    worst = _compare_rows(rows, st, RADII, BOXES)
    print('metrics moffat %s: %s' % (prec, worst))
    record_margin('metrics', **{'moffat_%s_%s' % (prec, k): v for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('prec', PRECS)
def test_reference_stamps_against_the_reference(ctx, prec, golden):
    st = _reference_stamps(golden)
    rows = ctx.stamp_metrics(st, RADII, BOXES, ())
    worst = _compare_rows(rows, st, RADII, BOXES)
    print('metrics golden %s: %s' % (prec, worst))
    record_margin('metrics', **{'golden_%s_%s' % (prec, k): v for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


# ---- 2. EE radii, checked through the reference's EE
@pytest.mark.parametrize('prec', PRECS)
def test_ee_radii(ctx, prec):
    pars = _synthetic_grid()[::3]
    st = np.array([M.stamp(*p) for p in pars])          # exact Moffats: non-negative, EE monotone
    assert st.min() >= 0.0
    rows = ctx.stamp_metrics(st, (), (), FRACS)
    assert rows.shape == (len(st), HEAD + len(FRACS))
    worst = 0.0
    for row, s in zip(rows, st):
        assert row[6] == 0.0, row
        c = R.centroid(s)
        for f, r in zip(FRACS, row[HEAD:]):
            assert 0.0 < r < R.r_max(c)
            worst = max(worst, abs(R.EE(s, c, r) - f) / TOL_R)
    print('metrics r_ee %s: %.3g' % (prec, worst))
    record_margin('metrics', **{'r_ee_%s' % prec: worst})
    assert worst <= 1.0
    # fractions in any order, and beside radii and boxes: the same radii
    mixed = ctx.stamp_metrics(st[:4], [1.0, 3.0], [2.0], FRACS[::-1])
    assert np.array_equal(mixed[:, HEAD + 3:], rows[:4, HEAD:][:, ::-1])


# ---- 3. given centres
@pytest.mark.parametrize('prec', PRECS)
def test_given_centres(ctx, prec):
    pars = _synthetic_grid()[5::11]
    st = np.array([M.stamp(*p) for p in pars])
    fit = ctx.fit_stamps_elliptical(st)
    centers = fit[:, 1:3].copy()
    radii, boxes = [0.5, 1.0, 3.0, 9.0, 30.0], [0.5, 1.0, 4.0, 11.0]
    rows = ctx.stamp_metrics(st, radii, boxes, FRACS, centers=centers)
    assert np.array_equal(rows[:, 4:6], centers)
    worst = _compare_rows(rows[:, :HEAD + len(radii) + len(boxes)], st, radii, boxes, centers)
    wr = 0.0
    for row, s, c in zip(rows, st, centers):
        for f, r in zip(FRACS, row[HEAD + len(radii) + len(boxes):]):
            wr = max(wr, abs(R.EE(s, c, r) - f) / TOL_R)
    worst['r_ee'] = wr
    # a centre off the stamp: what of the circle is on the stamp counts
    off = np.array([[-3.0, 44.5]])
    row = ctx.stamp_metrics(st[:1], [10.0, 30.0, 70.0], [20.0, 80.0], [], centers=off)
    worst['off_stamp'] = _compare_rows(row, st[:1], [10.0, 30.0, 70.0], [20.0, 80.0], off)['ee']
    print('metrics centres %s: %s' % (prec, worst))
    record_margin('metrics', **{'centres_%s_%s' % (prec, k): v for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('prec', PRECS)
def test_stamp_centre_on_a_symmetric_stamp(api, prec):
    """4-fold symmetric about the middle of the array (19.5, 19.5): the centroid is the geometric centre."""
    st = np.array([M.stamp(1.0, 19.5, 19.5, 5.0, 1.0, 0.0, 2.5), M.stamp(0.7, 19.5, 19.5, 9.0, 1.0, 0.0, 1.8)])
    st = 0.25 * (st + st[:, ::-1, :] + st[:, :, ::-1] + st[:, ::-1, ::-1])
    ps = 0.2
    a = api.psf_metrics(st, center='centroid', pixscale=ps, precision=prec)
    b = api.psf_metrics(st, center='stamp', pixscale=ps, precision=prec)
    assert np.array_equal(np.asarray(b['center']), np.full((2, 2), 19.5))
    worst = np.abs(np.asarray(a['center']) - 19.5).max() / TOL_C
    for k in ('ee', 'sqe'):
        worst = max(worst, np.abs(np.asarray(a[k]) - np.asarray(b[k])).max() / 1e-10)
    worst = max(worst, np.abs(np.asarray(a['r_ee']) - np.asarray(b['r_ee'])).max() / ps / 1e-10)
    record_margin('metrics', **{'stamp_vs_centroid_%s' % prec: worst})
    assert worst <= 1.0
    assert np.asarray(a['ee']).shape == (2, 5) and np.asarray(a['sqe']).shape == (2, 4)
    assert np.asarray(a['r_ee']).shape == (2, 2)
    assert a.meta['MRAD5'] == 2.0 and a.meta['MBOX1'] == 0.2 and a.meta['MFRAC2'] == 0.8
    assert a.meta['MCENTER'] == 'centroid' and b.meta['MCENTER'] == 'stamp'
    # any leading shape, and radii in arcsec
    c = api.psf_metrics(st.reshape(2, 1, 40, 40), radii=[1.0], boxes=[], fractions=[0.5], pixscale=ps, precision=prec)
    assert np.array_equal(np.asarray(c['ee'])[:, 0], np.asarray(a['ee'])[:, 3])
    assert np.array_equal(np.asarray(c['r_ee'])[:, 0], np.asarray(a['r_ee'])[:, 0])


# ---- 4. symmetry
@pytest.mark.parametrize('prec', PRECS)
def test_transpose_and_row_reversal(ctx, prec, golden):
    syn = [M.stamp(1.0, 19.2, 20.7, 5.0, 0.8, 30.0, 2.5), M.stamp(1.5, 20.9, 18.6, 8.0, 0.6, 112.0, 3.5)]
    st = np.concatenate([_reference_stamps(golden)[::7], np.array(syn)])
    radii, boxes = [0.3, 1.0, 2.0, 5.0, 12.0, 40.0], [0.4, 1.0, 3.0, 9.0]
    m0 = ctx.stamp_metrics(st, radii, boxes, FRACS)
    mt = ctx.stamp_metrics(np.transpose(st, (0, 2, 1)).copy(), radii, boxes, FRACS)
    mr = ctx.stamp_metrics(st[:, ::-1, :].copy(), radii, boxes, FRACS)
    tol = 1e-12
    worst = max(np.abs(mt[:, 4] - m0[:, 5]).max(), np.abs(mt[:, 5] - m0[:, 4]).max(),
                np.abs(mr[:, 4] - (39.0 - m0[:, 4])).max(), np.abs(mr[:, 5] - m0[:, 5]).max()) / tol
    worst = max(worst, np.abs(mt[:, HEAD:] - m0[:, HEAD:]).max() / tol, np.abs(mr[:, HEAD:] - m0[:, HEAD:]).max() / tol)
    print('metrics symmetry %s: %.3g' % (prec, worst))
    record_margin('metrics', **{'symmetry_%s' % prec: worst})
    assert worst <= 1.0
    assert np.array_equal(mt[:, 2], m0[:, 3]) and np.array_equal(mt[:, 3], m0[:, 2])
    assert np.array_equal(mr[:, 2], 39.0 - m0[:, 2]) and np.array_equal(mr[:, 1], m0[:, 1])


# ---- 5. independence of the batch and the device path
@pytest.mark.parametrize('prec', PRECS)
def test_batch_single_and_device_forms(ctx, prec, golden):
    import torch
    rng = np.random.default_rng(7)
    n = 3000
    pars = [(rng.uniform(0.5, 2), *(19.5 + rng.uniform(-2, 2, 2)), rng.uniform(3, 10), rng.uniform(0.6, 1.0),
             rng.uniform(0, 180), rng.uniform(1.8, 5)) for _ in range(n)]
    st = np.array([M.stamp(*p) for p in pars])
    radii, boxes = [1.0, 2.0, 5.0], [1.0, 3.0]
    batch = ctx.stamp_metrics(st, radii, boxes, FRACS)
    assert batch.shape == (n, HEAD + 9) and np.all(np.isfinite(batch)) and np.all(batch[:, 6] == 0.0)
    for k in (0, 1, 77, 1500, n - 1):
        assert np.array_equal(ctx.stamp_metrics(st[k], radii, boxes, FRACS), batch[k:k + 1]), k
    assert np.array_equal(ctx.stamp_metrics(st[100:164], radii, boxes, FRACS), batch[100:164])
    dev = torch.device('cuda:0')
    ts = torch.from_numpy(st).to(dev)
    to = torch.full((n, HEAD + 9), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.stamp_metrics_device(n, ts.data_ptr(), to.data_ptr(), radii, boxes, FRACS)
    ctx.sync()
    assert np.array_equal(to.cpu().numpy(), batch)
    # device centres
    ce = np.ascontiguousarray(batch[:, 2:4] + 0.25)
    tc = torch.from_numpy(ce).to(dev)
    torch.cuda.synchronize()
    ctx.stamp_metrics_device(n, ts.data_ptr(), to.data_ptr(), radii, boxes, FRACS, centers_ptr=tc.data_ptr())
    ctx.sync()
    assert np.array_equal(to.cpu().numpy(), ctx.stamp_metrics(st, radii, boxes, FRACS, centers=ce))


@pytest.mark.parametrize('prec', PRECS)
def test_reconstruct_device_chained_into_the_metrics(api, prec):
    import torch
    dim = 256
    ps = api.grid_pixscale(dim)
    lb = np.array([500.0, 700.0, 900.0])
    see, gl, l0, three = np.array([1.0, 0.8]), np.array([0.7, 0.5]), np.array([25.0, 20.0]), np.array([0, 1])
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    ref = ctx.reconstruct(lb, see, gl, l0, three, H, npsflin=1)
    dev = torch.device('cuda:0')
    tp = torch.empty(ref['psf'].shape, dtype=torch.float64, device=dev)
    ts = torch.empty(ref['psf_sum'].shape, dtype=torch.float64, device=dev)
    tf = torch.empty(ref['fit'].shape, dtype=torch.float64, device=dev)
    nst = int(np.prod(ref['psf'].shape[:-2]))
    radii, boxes = [1.0, 2.0, 5.0, 10.0], [1.0, 2.0, 3.0]
    tm = torch.empty((nst, HEAD + 9), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.reconstruct_device(lb, see, gl, l0, three, H, 12.0, 1, None, tp.data_ptr(), ts.data_ptr(), tf.data_ptr())
    ctx.stamp_metrics_device(nst, tp.data_ptr(), tm.data_ptr(), radii, boxes, [0.5, 0.8])
    ctx.sync()
    assert np.array_equal(tp.cpu().numpy(), ref['psf'])
    got = tm.cpu().numpy()
    assert np.array_equal(got, ctx.stamp_metrics(ref['psf'], radii, boxes, [0.5, 0.8]))
    assert np.all(got[:, 6] == 0.0)
    ctx.close()


# ---- 6. bad stamps and refusals
@pytest.mark.parametrize('prec', PRECS)
def test_bad_stamps(ctx, prec):
    good = M.stamp(1.0, 20.0, 19.0, 5.0, 0.8, 40.0, 2.5)
    st = np.array([good, np.zeros((40, 40)), good, good, good, -good, good])
    st[3, 11, 7] = np.nan
    st[5, 20, 19] += 0.5 * np.abs(st[5]).sum()           # (negative total with a positive peak)
    radii, boxes = [1.0, 4.0], [2.0]
    rows = ctx.stamp_metrics(st, radii, boxes, [0.5, 0.8])
    alone = ctx.stamp_metrics(good, radii, boxes, [0.5, 0.8])
    for k in (0, 2, 4, 6):
        assert np.array_equal(rows[k:k + 1], alone), k
    for k in (1, 3, 5):
        assert rows[k, 6] == 2.0 and rows[k, 7] == 0.0, (k, rows[k])
        assert np.all(np.isnan(rows[k, HEAD:])), (k, rows[k])
    assert rows[1, 0] == 0.0 and rows[1, 1] == 0.0 and np.isnan(rows[3, 0]) and rows[5, 0] < 0.0
    # given centres do not rescue a bad stamp
    rows = ctx.stamp_metrics(st, radii, boxes, [0.5], centers=np.full((7, 2), 19.5))
    assert np.array_equal(rows[:, 6], [0, 2, 0, 2, 0, 2, 0]) and np.all(np.isnan(rows[[1, 3, 5], HEAD:]))
    assert np.all(np.isfinite(rows[[0, 2, 4, 6]]))


@pytest.mark.parametrize('prec', PRECS)
def test_refusals_leave_out_untouched(ctx, prec):
    st = np.ascontiguousarray(np.array([M.stamp(1.0, 20.0, 19.0, 5.0, 0.8, 40.0, 2.5)] * 2))
    dp = C.POINTER(C.c_double)

    def call(nstamp, radii, boxes, fracs, nrad=None, nbox=None, nfrac=None):
        r, b, f = (np.ascontiguousarray(np.asarray(v, dtype=float)) for v in (radii, boxes, fracs))
        out = np.full((2, HEAD + 48), -7.0)
        rc = ctx.lib.mpsfr_stamp_metrics(ctx._h, nstamp, st.ctypes.data_as(C.c_void_p), None,
                                         r.size if nrad is None else nrad, r.ctypes.data_as(dp),
                                         b.size if nbox is None else nbox, b.ctypes.data_as(dp),
                                         f.size if nfrac is None else nfrac, f.ctypes.data_as(dp),
                                         out.ctypes.data_as(C.c_void_p), 0)
        return rc, out

    one = np.ones(17)
    bad = [(2, [], [], []), (0, [1.0], [], []), (-1, [1.0], [], []), (2, one, [], []), (2, [], one, []),
           (2, [], [], one * 0.5), (2, [0.0], [], []), (2, [-1.0], [], []), (2, [np.nan], [], []), (2, [np.inf], [], []),
           (2, [80.5], [], []), (2, [1.0], [0.0], []), (2, [1.0], [np.nan], []), (2, [1.0], [81.0], []),
           (2, [1.0], [], [0.0]), (2, [1.0], [], [1.0]), (2, [1.0], [], [np.nan]), (2, [1.0], [], [-0.5])]
    for args in bad:
        rc, out = call(*args)
        assert rc == -1, args                                # MPSFR_E_INVALID
        assert np.all(out == -7.0), args
    rc, out = call(2, [1.0], [], [], nrad=-1)
    assert rc == -1 and np.all(out == -7.0)
    rc, out = call(2, [80.0], [80.0], [0.5])                   # the limits themselves are accepted
    flat = out.ravel()
    assert rc == 0 and np.all(flat[:2 * (HEAD + 3)] != -7.0) and np.all(flat[2 * (HEAD + 3):] == -7.0)
    # the Python layer refuses the same before the library is called
    for args in (([0.0], [], []), ([], [], []), ([1.0], [81.0], []), ([1.0], [], [1.0])):
        with pytest.raises(ValueError):
            ctx.stamp_metrics(st, *args)
    with pytest.raises(ValueError):
        ctx.stamp_metrics(st, [1.0], [], [], centers=np.zeros((3, 2)))


# ---- 7. the Python API
def _names(t):
    return list(t.colnames if hasattr(t, 'colnames') else t.keys())


def _same_table(a, b, names):
    for k in names:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_compute_functions_with_metrics(api):
    lb = np.array([500.0, 750.0])
    dim = 512
    ps = api.grid_pixscale(dim)
    kw = dict(dim=dim, pixscale=ps, verbose=False)
    pos = [[0.0, 0.0], [30.0, 0.0], [-50.0, -50.0]]
    prof = dict(cn2=[0.6, 0.25, 0.15], h=[0.0, 1000.0, 10000.0], wind_speed=[8.0, 15.0, 30.0], wind_dir=[0.3, -1.0, 2.0])
    mreq = dict(radii=[0.05, 0.1, 0.3], boxes=[0.0762, 0.2], fractions=[0.5, 0.8, 0.9])
    calls = [
        lambda **k: api.compute_psf(lb, 1.0, 0.7, 25.0, **kw, **k),
        lambda **k: api.compute_field_psf(lb, 1.0, 0.7, 25.0, positions=pos, **kw, **k),
        lambda **k: api.compute_field_psf(lb, 1.0, 0.7, 25.0, positions=pos, circular=False, **kw, **k),
        lambda **k: api.compute_band_psf(np.linspace(480.0, 930.0, 10), 1.0, 0.7, 25.0, [(480, 930), (600, 700)],
                                         **kw, **k),
        lambda **k: api.compute_band_psf(np.linspace(480.0, 930.0, 10), 1.0, 0.7, 25.0, [(480, 930), (600, 700)],
                                         positions=pos, **kw, **k),
        lambda **k: api.compute_profile_psf(lb, 1.0, 25.0, **prof, **kw, **k),
        lambda **k: api.compute_profile_psf(lb, 1.0, 25.0, positions=pos, circular=False, **prof, **kw, **k),
    ]
    for f in calls:
        t0, p0 = f()
        t1, p1 = f(metrics=mreq)
        assert np.array_equal(p0, p1)
        assert _names(t1) == _names(t0) + ['ee', 'sqe', 'r_ee']
        _same_table(t0, t1, _names(t0))
        m = api.psf_metrics(p1, pixscale=ps, **mreq)
        n = int(np.prod(p1.shape[:-2]))
        assert len(np.asarray(t1['ee'])) == n == len(np.asarray(t0[_names(t0)[0]]))
        for k, w in (('ee', 3), ('sqe', 2), ('r_ee', 3)):
            assert np.asarray(t1[k]).shape == (n, w)
            assert np.array_equal(np.asarray(t1[k]), np.asarray(m[k])), k
        assert np.all(np.asarray(m['status']) == 0)
    # metrics=True: the defaults (in arcsec, on the pixel scale of the call)
    t1, p1 = api.compute_psf(lb, 1.0, 0.7, 25.0, dim=1280, verbose=False, metrics=True)
    m = api.psf_metrics(p1)
    assert np.asarray(t1['ee']).shape == (2, 5) and np.array_equal(np.asarray(t1['sqe']), np.asarray(m['sqe']))


def _sparta(api, nlines):
    from muse_psfr_amd import _minifits
    hdu = api.create_sparta_table(nlines=nlines, seeing=1.0, L0=20, GL=0.6)
    d = hdu.data
    rng = np.random.default_rng(4)
    for k in range(1, 5):
        d['LGS%d_SEEING' % k] = 0.7 + 0.6 * rng.random(nlines)
        d['LGS%d_TUR_GND' % k] = 0.4 + 0.5 * rng.random(nlines)
        d['LGS%d_L0' % k] = 12 + 15 * rng.random(nlines)
    return _minifits.HDUList([_minifits.PrimaryHDU(), hdu])


def test_sparta_metrics_hdus(api):
    dim = 512
    ps = api.grid_pixscale(dim)
    kw = dict(nl=4, dim=dim, pixscale=ps, device=0, verbose=False, field_positions='grid', npsflin=2,
              bands=[(480, 930)], band_lbda=np.linspace(480.0, 930.0, 10))
    base = api.compute_psf_from_sparta(_sparta(api, 3), **kw)
    assert [h.name for h in base] == ['PRIMARY', 'SPARTA_ATM_DATA', 'FIT_ROWS', 'FIT_MEAN', 'PSF_MEAN', 'PSF_FIELD',
                                      'FIT_FIELD', 'FIT_BAND_ROWS', 'PSF_BAND', 'FIT_BAND']
    mreq = dict(radii=[0.05, 0.1, 0.3], boxes=[0.0762, 0.2], fractions=[0.5, 0.8])
    out = api.compute_psf_from_sparta(_sparta(api, 3), metrics=mreq, **kw)
    names = [h.name for h in out]
    assert names[:len(base)] == [h.name for h in base]
    assert names[len(base):] == ['METRICS_MEAN', 'METRICS_FIELD', 'METRICS_BAND']
    for hb, ho in zip(base, out):
        if hb.data is not None:
            assert np.asarray(hb.data).tobytes() == np.asarray(ho.data).tobytes(), hb.name
    for name, src, n in (('METRICS_MEAN', 'PSF_MEAN', 4), ('METRICS_FIELD', 'PSF_FIELD', 16),
                         ('METRICS_BAND', 'PSF_BAND', 1)):
        d = out[name].data
        m = api.psf_metrics(np.asarray(out[src].data), pixscale=ps, **mreq)
        assert len(d) == n
        for k in ('flux', 'peak', 'center', 'ee', 'sqe', 'r_ee', 'status'):
            assert np.array_equal(np.asarray(d[k]), np.asarray(m[k])), (name, k)
        assert out[name].header['MRAD3'] == 0.3 and out[name].header['MFRAC2'] == 0.8
    assert np.array_equal(np.asarray(out['METRICS_MEAN'].data['lbda']), np.asarray(out['FIT_MEAN'].data['lbda']))
    assert np.array_equal(np.asarray(out['METRICS_FIELD'].data['dir_idx']), np.asarray(out['FIT_FIELD'].data['dir_idx']))
    # the issue's call: the default metrics beside field positions and a band
    kw2 = dict(nl=3, dim=1280, device=0, verbose=False)
    full = api.compute_psf_from_sparta(_sparta(api, 2), metrics=True, field_positions='grid', bands=[(480, 930)], **kw2)
    assert [h.name for h in full][-3:] == ['METRICS_MEAN', 'METRICS_FIELD', 'METRICS_BAND']
    assert np.asarray(full['METRICS_MEAN'].data['ee']).shape == (3, 5)
    plain = api.compute_psf_from_sparta(_sparta(api, 2), **kw2)
    assert [h.name for h in plain] == ['PRIMARY', 'SPARTA_ATM_DATA', 'FIT_ROWS', 'FIT_MEAN', 'PSF_MEAN']


def test_cli_metrics(api, tmp_path):
    from muse_psfr_amd import _minifits, cli
    out, log = str(tmp_path / 'o.fits'), str(tmp_path / 'l.log')
    cli.main(['--values', '1.0,0.7,25', '--no-color', '--metrics', '--logfile', log, '-o', out])
    text = open(log).read()
    assert 'SQE0.2 ' in text and 'R_EE50 ' in text
    fits, _ = api.psfrec._astropy()
    hdul = (fits or _minifits).open(out)
    assert 'METRICS_MEAN' in [h.name for h in hdul]
    sq = np.asarray(hdul['METRICS_MEAN'].data['sqe'])
    assert sq.shape == (3, 4) and np.all(np.diff(sq, axis=1) > 0)


# ---- 8. physical sanity (no tolerance to tune)
@pytest.mark.parametrize('prec', PRECS)
def test_physical_sanity_of_the_reference_stamps(api, prec, golden):
    st = _reference_stamps(golden)
    t = api.psf_metrics(st, radii=(0.2, 0.4, 0.6, 1.0, 2.0, 11.4), precision=prec)       # 0.2 arcsec pixels
    sqe, ee, ree = np.asarray(t['sqe']), np.asarray(t['ee']), np.asarray(t['r_ee'])
    assert np.all(np.asarray(t['status']) == 0)
    assert np.all(sqe[:, 0] > 0) and np.all(np.diff(sqe, axis=1) > 0) and np.all(sqe < 1)
    assert np.all(np.diff(ee[:, :5], axis=1) > 0) and np.all(ee[:, :5] < 1)
    assert np.all(ree[:, 0] < ree[:, 1]) and np.all(ree[:, 0] > 0)
    # 11.4 arcsec = 57 px: beyond the farthest corner of the stamp from any point on it (40 sqrt 2 = 56.6 px)
    assert np.all(np.abs(ee[:, 5] - 1.0) <= 1e-12)
    # a box encloses its inscribed circle and lies inside the circle through its corners
    for k, s in enumerate((0.2, 0.4, 0.6, 1.0)):
        inner = np.asarray(api.psf_metrics(st, radii=(s / 2, s / np.sqrt(2)), boxes=(), fractions=(), precision=prec)['ee'])
        assert np.all(inner[:, 0] < sqe[:, k]) and np.all(sqe[:, k] < inner[:, 1])
