"""Host: the crowded-field fit (mpsfr_fit_frame_psf) without a GPU.

1. the yardstick (frame_fit_ref) checked on itself: the noiseless scene is recovered to the bound; on the noisy scene
   every accepted star lies within 4 marginal sigma of the truth; the fit domain on cases written out by hand (a pixel
   exactly on the radius, a masked centre); the statuses of the scene; the textbook iteration reaches the yardstick within
   the convergence bound in the number of steps the design counts on.
2. the case the feature exists for: group_ref flags the chain of 7 OVERSIZE at crit 3.5.
3. what Context.fit_frame_psf and its device form hand to C (the recording stub of test_render_host.py), every refusal
   of the Python layer before any library call.
4. psfrec.fit_crowded_stars and fit_found_stars(crowded='frame') against an answering stub: the columns, the origins,
   the rows of the crowded stars and the `group` column subtract_stars follows.
5. the constants against the header, the export, the build list.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frame_fit_ref as F
import group_ref as G
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec
from test_group_host import TableLib, _array, crowd
from test_render_host import DEV, HANDLE, make_ctx

NS = 40


# ---- 1. the yardstick
def test_noiseless_scene_is_recovered_to_the_bound():
    s = F.scene(noise=False)
    for radius in (4.0, 8.0):
        acc = F.scene_reference(True, True, radius, noise=False)['acc']
        # (a star the fit leaves out keeps its light in the frame -- at radius 4 two lie in the masked block --, so the
        # frame of this check holds the accepted stars alone; who is accepted depends on the mask, not on the values)
        model, _, _ = F.Y.render(None, s['psf'], s['index'][acc], s['origin'][acc], s['shift'][acc], s['flux'][acc],
                                 shape=F.FRAME)
        image = np.where(np.isnan(s['image']), np.nan, model)
        ref = F.solve(image, s['var'], s['psf'], s['index'], s['origin'], s['shift'], radius, True)
        assert ref['head_status'] == 0 and ref['nacc'] >= 30 and np.array_equal(ref['acc'], acc)
        # the data lie in the column space: the truth is the least-squares solution, and nothing iterates (tol = 0)
        b = F.bounds(ref, 0.0, 0)
        truth = np.concatenate([s['flux'][acc], [0.0]]) * np.sqrt(ref['dg'])
        err = np.linalg.norm(ref['x'] * np.sqrt(ref['dg']) - truth)
        assert err <= b['y'], (err, b['y'])
        assert b['y'] <= 1e-9 * np.linalg.norm(truth)
        assert ref['chi2'] <= 1e-16 * np.sum(ref['w'] * ref['d'] ** 2)


def test_noisy_scene_within_four_marginal_sigma():
    s = F.scene()
    for radius in (4.0, 8.0):
        ref = F.scene_reference(True, True, radius)
        acc = ref['acc']
        pull = np.abs(ref['F'][acc] - s['flux'][acc]) / ref['sigma'][acc]
        assert pull.max() <= 4.0, pull.max()
        assert abs(ref['b'] - F.SKY) <= 4.0 * np.sqrt(np.linalg.inv(ref['N'])[-1, -1])
        dof = ref['nomega'] - ref['nacc'] - 1
        assert abs(ref['chi2'] / dof - 1.0) < 5.0 * np.sqrt(2.0 / dof)
        # the conditional error is optimistic where stars overlap: up to a few times in the chain
        ratio = ref['sigma'][acc] / np.sqrt(1.0 / ref['nkk'][acc])
        assert np.all(ratio >= 1.0 - 1e-12) and 1.5 < ratio.max() < 4.0
        chain = ref['overlap'][s['chain']]
        assert chain.max() > 1.0 and chain[1:-1].min() > ref['overlap'][acc].min() and ref['overlap'][acc].min() < 0.5


def test_scene_statuses_and_condition():
    s = F.scene()
    assert s['image'].shape == F.FRAME and F.FRAME[0] % 32 and F.FRAME[1] % 32
    assert 0.005 < np.isnan(s['image']).mean() < 0.06
    d = s['pos'][s['triple']]
    assert max(np.hypot(*(d[i] - d[j])) for i in range(3) for j in range(3)) < 2.0
    for with_var in (True, False):
        for background in (True, False):
            for radius in (4.0, 8.0):
                ref = F.scene_reference(with_var, background, radius)
                st = ref['status']
                assert st[s['off']] == 1 and st[s['dark']] == 2 and st[s['top']] == 0 and st[s['corner']] == 0
                assert np.all(st[s['chain']] == 0) and np.all(st[s['triple']] == 0)
                assert ref['ndisc'][s['top']] < ref['ndisc'][s['chain'][0]]
                kappa = F.bounds(ref, 1e-10, 100)['kappa']
                assert 5.0 < kappa < 60.0
                # the textbook iteration: a few tens of steps, and within the convergence bound of the yardstick
                x, it, rel = F.pcg(ref, 1e-10, 100)
                assert it <= 30 and rel <= 1e-10
                b = F.bounds(ref, 1e-10, 100)
                assert np.linalg.norm((x - ref['x']) * np.sqrt(ref['dg'])) <= b['y']
                # from the solution, a tolerance of 1/4 asks for at most two steps (tests/test_gpu_frame_fit.py)
                if not background:
                    assert F.pcg(ref, 0.25, 100, x0=x)[1] <= 2


def test_domain_on_hand_made_cases():
    psf = F.Y.models()[:1]
    image = np.ones((40, 40))
    origin = np.array([[-10, -10]], dtype=np.int32)              # centre (10, 10)
    # 3-4-5: the pixel (13, 14) lies exactly on the radius 5
    ref = F.solve(image, None, psf, None, origin, None, 5.0, False)
    assert ref['omega'][13, 14] and ref['omega'][14, 13] and ref['omega'][15, 10] and not ref['omega'][14, 14]
    assert ref['nomega'] == 81 == ref['ndisc'][0]                # the lattice points of the disc of radius 5
    below = float(np.nextafter(5.0, 0.0))
    ref = F.solve(image, None, psf, None, origin, None, below, False)
    assert not ref['omega'][13, 14] and not ref['omega'][15, 10] and ref['omega'][13, 13] and ref['nomega'] == 69
    # a shift moves the disc with the centre: c = 10 + 0.5
    ref = F.solve(image, None, psf, None, origin, np.array([[0.5, 0.0]]), 1.0, False)
    assert sorted(zip(*np.nonzero(ref['omega']))) == [(10, 10), (11, 10)]
    # a masked centre: the star stays, its disc loses the pixel; masked by the variance just the same
    hole = image.copy()
    hole[10, 10] = np.nan
    ref = F.solve(hole, None, psf, None, origin, None, 5.0, True)
    assert ref['status'][0] == 0 and not ref['omega'][10, 10] and ref['nomega'] == 80 and ref['ndisc'][0] == 80
    var = np.ones((40, 40))
    var[10, 10], var[10, 11], var[11, 10] = 0.0, np.inf, -1.0
    ref = F.solve(image, var, psf, None, origin, None, 5.0, True)
    assert ref['nomega'] == 78 and not ref['omega'][10, 11]
    # the disc all masked: status 2, nothing fitted; off the frame: status 1
    hole[5:16, 5:16] = np.nan
    ref = F.solve(hole, None, psf, None, origin, None, 5.0, True)
    assert ref['status'][0] == 2 and ref['head_status'] == 2 and np.array_equal(ref['resid'], hole, equal_nan=True)
    ref = F.solve(image, None, psf, None, np.array([[-60, 0]], dtype=np.int32), None, 5.0, True)
    assert ref['status'][0] == 1 and ref['head_status'] == 2
    # too few pixels for the unknowns: one pixel, two unknowns
    ref = F.solve(np.ones((1, 1)), None, psf, None, np.array([[-20, -20]], dtype=np.int32), None, 5.0, True)
    assert ref['nomega'] == 1 and ref['head_status'] == 2 and ref['status'][0] == 2
    ref = F.solve(np.ones((1, 1)), None, psf, None, np.array([[-20, -20]], dtype=np.int32), None, 5.0, False)
    assert ref['nomega'] == 1 and ref['head_status'] == 2              # |Omega| < unknowns + 1


# ---- 2. the case the feature exists for
def test_group_stars_flags_the_chain_oversize():
    s = F.scene()
    pos = s['pos'][s['chain']]
    ref = G.group(pos, 3.5, F.FRAME)
    assert list(ref['counts']) == [1, 0, 0, 0, 0, 1] and ref['groups'][0, 0] == F.CHAIN
    assert ref['groups'][0, 1] & G.OVERSIZE and np.all(ref['origin'] == G.FILLER_ORIGIN)


# ---- 3. what reaches C
@pytest.fixture
def ctx():
    c = make_ctx()
    yield c
    c._h = None


def _scene_args():
    s = F.scene()
    return s['image'], s['psf'], s['origin']


def test_fit_frame_psf_host_form(ctx):
    s = F.scene()
    n = s['n']
    rows, head = ctx.fit_frame_psf(s['image'], s['psf'], s['origin'], var=s['var'], shift=s['shift'],
                                   psf_index=s['index'])
    assert rows.shape == (n, _lib.NFRAMEFIT) and head.shape == (_lib.NFRAMEFIT,)
    name, a = ctx.lib.calls[0]
    assert name == 'mpsfr_fit_frame_psf' and len(a) == 20 and len(ctx.lib.calls) == 1 and a[0].value == HANDLE
    assert (a[1], a[2], a[5], a[6], a[12], a[13], a[14], a[15], a[19]) == (97, 150, n, 4, 8.0, _lib.FIT_BACKGROUND, 100,
                                                                          1e-10, 0)
    assert all(isinstance(a[i], int) and not isinstance(a[i], bool) for i in (1, 2, 5, 6, 13, 14, 19))
    assert isinstance(a[12], float) and isinstance(a[15], float)
    assert a[11] is None and a[18] is None and a[16].value == rows.ctypes.data and a[17].value == head.ctypes.data
    np.testing.assert_array_equal(_array(a[9], 2 * n, C.c_int32, np.int32).reshape(n, 2), s['origin'])
    np.testing.assert_array_equal(_array(a[8], n, C.c_int32, np.int32), s['index'])
    np.testing.assert_array_equal(_array(a[10], 2 * n, C.c_double, np.float64).reshape(n, 2), s['shift'])
    np.testing.assert_array_equal(_array(a[4], 97 * 150, C.c_double, np.float64).reshape(97, 150), s['var'])
    ctx.lib.calls.clear()
    out = ctx.fit_frame_psf(s['image'].tolist(), s['psf'][0], s['origin'].tolist(), psf_index=[0] * n,
                            scale0=list(range(n)), radius=4, background=False, max_iter=1000, tol=np.float32(0.5),
                            return_residual=True)
    a = ctx.lib.calls[0][1]
    assert len(out) == 3 and out[2].shape == F.FRAME and a[18].value == out[2].ctypes.data
    assert (a[6], a[12], a[13], a[14], a[15]) == (1, 4.0, 0, 1000, 0.5) and a[4] is None and a[10] is None
    np.testing.assert_array_equal(_array(a[11], n, C.c_double, np.float64), np.arange(n))
    # a masked array: masked pixels are NaN
    ctx.lib.calls.clear()
    ctx.fit_frame_psf(np.ma.masked_less(np.arange(6.0).reshape(2, 3), 2.0), s['psf'][:1], [[0, 0]])
    a = ctx.lib.calls[0][1]
    assert np.isnan(_array(a[3], 6, C.c_double, np.float64)[:2]).all() and (a[1], a[2], a[5], a[6]) == (2, 3, 1, 1)


def test_fit_frame_psf_device_form(ctx):
    assert ctx.fit_frame_psf_device(97, 150, DEV['image'], 4096, 4096, DEV['psf'], DEV['origin'], DEV['rows'],
                                    DEV['out']) is None
    name, a = ctx.lib.calls[0]
    assert name == 'mpsfr_fit_frame_psf' and len(a) == 20 and a[19] == 1
    assert (a[1], a[2], a[5], a[6], a[12], a[13], a[14], a[15]) == (97, 150, 4096, 4096, 8.0, 1, 100, 1e-10)
    assert (a[3].value, a[7].value, a[9].value, a[16].value, a[17].value) == \
        (DEV['image'], DEV['psf'], DEV['origin'], DEV['rows'], DEV['out'])
    assert all(a[i] is None for i in (4, 8, 10, 11, 18))
    ctx.lib.calls.clear()
    ctx.fit_frame_psf_device(1, 1, DEV['image'], 2 ** 20, 2 ** 20, DEV['psf'], DEV['origin'], DEV['rows'], DEV['out'],
                             var_ptr=DEV['var'], shift_ptr=DEV['shift'], psf_index_ptr=DEV['index'],
                             scale0_ptr=DEV['scale'], resid_ptr=DEV['stamps'], radius=20, background=False, max_iter=1,
                             tol=0.999)
    a = ctx.lib.calls[0][1]
    assert (a[4].value, a[8].value, a[10].value, a[11].value, a[18].value) == \
        (DEV['var'], DEV['index'], DEV['shift'], DEV['scale'], DEV['stamps'])
    assert (a[12], a[13], a[14], a[15]) == (20.0, 0, 1, 0.999)


def test_fit_frame_psf_refuses(ctx):
    image, psf, origin = _scene_args()
    n = len(origin)
    base = dict(image=image, psf=psf, origin=origin, var=None, shift=None, psf_index=np.zeros(n, dtype=int), scale0=None,
                radius=8.0, background=True, max_iter=100, tol=1e-10, return_residual=False)
    shift = np.zeros((n, 2))
    far, nan = shift.copy(), shift.copy()
    far[3, 1], nan[0, 0] = 8.5, np.nan
    bad = [dict(image=image[0]), dict(image='x'), dict(image=np.zeros((0, 3))), dict(var=np.ones((3, 3))),
           dict(psf=psf[:, :39]), dict(psf='p'), dict(psf_index=None), dict(psf_index=np.full(n, 4)),
           dict(psf_index=np.zeros(n)), dict(psf_index=np.zeros(n - 1, dtype=int)),
           dict(origin=origin[:, :1]), dict(origin=origin.astype(float)), dict(origin=np.zeros((0, 2), dtype=int)),
           dict(origin=np.full((n, 2), 2 ** 30 + 1)),
           dict(shift=far), dict(shift=nan), dict(shift=shift[:-1]), dict(shift='s'),
           dict(scale0=np.zeros(n - 1)), dict(scale0=np.full(n, np.inf)), dict(scale0=np.full(n, np.nan)),
           dict(scale0='s'), dict(scale0=np.zeros((n, 2))),
           dict(radius=0.99), dict(radius=20.01), dict(radius=np.nan), dict(radius=np.inf), dict(radius='8'),
           dict(radius=None), dict(radius=True),
           dict(tol=0.0), dict(tol=1.0), dict(tol=-1e-3), dict(tol=np.nan), dict(tol=None), dict(tol=True),
           dict(max_iter=0), dict(max_iter=1001), dict(max_iter=10.0), dict(max_iter=True), dict(max_iter=None),
           dict(background=1), dict(background=None), dict(return_residual=1)]
    for kw in bad:
        args = dict(base)
        args.update(kw)
        im, ps, og = args.pop('image'), args.pop('psf'), args.pop('origin')
        with pytest.raises(ValueError):
            ctx.fit_frame_psf(im, ps, og, **args)
    ok = (97, 150, 1, 10, 1, 1, 1, 1, 1)
    for k, v in [(0, 0), (1, 16385), (0, 97.0), (2, 0), (3, 0), (3, 2 ** 20 + 1), (3, 1.0), (3, True), (4, 0), (5, 0),
                 (6, 0), (7, 0), (8, None), (2, None)]:
        a = list(ok)
        a[k] = v
        with pytest.raises(ValueError):
            ctx.fit_frame_psf_device(*a, psf_index_ptr=1)
    with pytest.raises(ValueError):
        ctx.fit_frame_psf_device(*ok)                                # npsf != nstar without psf_index_ptr
    for kw in (dict(radius=0.5), dict(radius=21), dict(tol=0), dict(tol=1), dict(max_iter=0), dict(max_iter=1001),
               dict(background=0), dict(tol=np.nan), dict(radius=np.nan)):
        with pytest.raises(ValueError):
            ctx.fit_frame_psf_device(*ok, psf_index_ptr=1, **kw)
    assert ctx.lib.calls == []
    ctx.fit_frame_psf_device(16384, 4096, 1, 2 ** 20, 1, 1, 1, 1, 1, psf_index_ptr=1, radius=1, tol=1e-300,
                             max_iter=1000)                          # the bounds themselves are legal
    assert len(ctx.lib.calls) == 1


# ---- 4. psfrec against an answering stub
class FrameLib(TableLib):
    """TableLib whose mpsfr_fit_frame_psf answers F = 1000 dp + dq of every star's shift (err 1, flux 2 F, err_flux 2,
    overlap 0.25, 50 pixels, N_kk 4, status 0; star 1 of three or more status 2) and the head (3, 0.5, 77, 1234, 9, 1e-11,
    n, 0), the residual the image itself; mpsfr_render_stars copies the image and clears its rows."""

    def mpsfr_fit_frame_psf(self, *a):
        self.calls.append(('mpsfr_fit_frame_psf', a))
        ny, nx, n = a[1], a[2], a[5]
        sh = _array(a[10], 2 * n, C.c_double, np.float64).reshape(n, 2)
        out = _array(a[16], n * 8, C.c_double, np.float64).reshape(n, 8)
        out[:] = 0.0
        out[:, 0] = 1000.0 * sh[:, 0] + sh[:, 1]
        out[:, 1:7] = (1.0, 0.0, 2.0, 0.25, 50.0, 4.0)
        out[:, 2] = 2.0 * out[:, 0]
        if n >= 3:
            out[1] = (0, 0, 0, 0, 0, 0, 0, 2)
        _array(a[17], 8, C.c_double, np.float64)[:] = (3.0, 0.5, 77.0, 1234.0, 9.0, 1e-11, n, 0.0)
        if a[18] is not None:
            _array(a[18], ny * nx, C.c_double, np.float64)[:] = _array(a[3], ny * nx, C.c_double, np.float64)
        return 0

    def mpsfr_render_stars(self, *a):
        self.calls.append(('mpsfr_render_stars', a))
        ny, nx = a[1], a[2]
        _array(a[12], ny * nx, C.c_double, np.float64)[:] = _array(a[3], ny * nx, C.c_double, np.float64)
        if a[13] is not None:
            C.memset(a[13], 0, 8 * _lib.NRENDER * a[4])
        return 0


def _frame_ctx(monkeypatch):
    ctx = make_ctx()
    ctx.lib = FrameLib()
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: ctx)
    return ctx


def test_fit_crowded_stars_table(monkeypatch):
    ctx = _frame_ctx(monkeypatch)
    pos = np.array([[10.4, 20.5], [30.5, 7.25], [-3.0, 12.75], [50.0, 60.0]])
    image, psf = np.arange(70.0 * 80).reshape(70, 80), F.Y.models()[0]
    found = {'position': pos, 'scale': np.array([5.0, 6.0, 7.0, 8.0])}
    fit, origin, resid = psfrec.fit_crowded_stars(image, psf, found, start='found', radius=6, fit_back=False,
                                                  max_iter=50, tol=1e-8, return_residual=True, pixscale=0.25)
    assert tuple(fit.colnames) == psfrec._FIT_COLS_CROWDED == ('scale', 'shift', 'flux', 'err_scale', 'err_flux',
                                                               'overlap', 'npix', 'status')
    want = (np.rint(pos) - 20).astype(np.int32)
    assert origin.dtype == np.int32 and np.array_equal(origin, want)
    sh = pos - (want + 20)
    assert np.all(np.abs(sh) <= 0.5)
    a = ctx.lib.calls[0][1]
    assert [c[0] for c in ctx.lib.calls] == ['mpsfr_fit_frame_psf']
    assert (a[1], a[2], a[5], a[6], a[12], a[13], a[14], a[15]) == (70, 80, 4, 1, 6.0, 0, 50, 1e-8)
    np.testing.assert_array_equal(_array(a[11], 4, C.c_double, np.float64), [5.0, 6.0, 7.0, 8.0])
    np.testing.assert_array_equal(_array(a[8], 4, C.c_int32, np.int32), 0)
    np.testing.assert_array_equal(_array(a[10], 8, C.c_double, np.float64).reshape(4, 2), sh)
    F0 = 1000.0 * sh[:, 0] + sh[:, 1]
    keep = np.array([True, False, True, True])
    np.testing.assert_array_equal(np.asarray(fit['scale'])[keep], F0[keep])
    np.testing.assert_array_equal(np.asarray(fit['flux'])[keep], 2.0 * F0[keep])
    np.testing.assert_array_equal(fit['shift'], sh * 0.25)
    np.testing.assert_array_equal(fit['status'], [0, 2, 0, 0])
    np.testing.assert_array_equal(fit['npix'], [50, 0, 50, 50])
    assert np.asarray(fit['npix']).dtype == np.int64 and np.asarray(fit['status']).dtype == np.int64
    np.testing.assert_array_equal(np.asarray(fit['overlap'])[keep], 0.25)
    np.testing.assert_array_equal(np.asarray(fit['err_scale'])[keep], 1.0)
    np.testing.assert_array_equal(np.asarray(fit['err_flux'])[keep], 2.0)
    assert dict(fit.meta) == dict(back=3.0, err_back=0.5, chi2=77.0, npix=1234, iterations=9, residual=1e-11, status=0)
    assert np.array_equal(resid, image)
    # one model stamp per star, a plain array of positions, no start
    ctx.lib.calls.clear()
    fit, origin = psfrec.fit_crowded_stars(image, F.Y.models(), pos, var=np.ones((70, 80)))
    a = ctx.lib.calls[0][1]
    assert (a[6], a[12], a[13], a[14], a[15]) == (4, 8.0, 1, 100, 1e-10) and a[8] is None and a[11] is None
    assert a[4] is not None and a[18] is None
    # the table is what subtract_stars takes
    ctx.lib.calls.clear()
    res, status = psfrec.subtract_stars(image, F.Y.models(), origin, fit, pixscale=0.2)
    a = ctx.lib.calls[0][1]
    assert ctx.lib.calls[0][0] == 'mpsfr_render_stars' and a[4] == 3 and list(status) == [0, -1, 0, 0]
    np.testing.assert_array_equal(_array(a[10], 3, C.c_double, np.float64), np.asarray(fit['scale'])[keep])
    ctx._h = None


def test_fit_crowded_stars_refuses(monkeypatch):
    ctx = _frame_ctx(monkeypatch)
    image, psf, pos = np.zeros((30, 30)), F.Y.models()[0], np.array([[3.0, 4.0], [5.0, 6.0]])
    for p in (np.zeros(2), 'p', np.zeros((2, 3)), np.array([[np.nan, 1.0]]), np.array([[2.0 ** 31, 1.0]]),
              np.zeros((0, 2))):
        with pytest.raises(ValueError):
            psfrec.fit_crowded_stars(image, psf, p)
    for kw in (dict(radius=0.5), dict(radius=25), dict(fit_back=1), dict(start='find'), dict(start='found'),
               dict(start=np.zeros(3)), dict(start=[np.nan, 1.0]), dict(max_iter=0), dict(tol=1.0), dict(tol=0),
               dict(pixscale=0.0), dict(var=np.ones((3, 3))), dict(psf_index=[0, 1]), dict(return_residual=None)):
        with pytest.raises(ValueError):
            psfrec.fit_crowded_stars(image, psf, pos, **kw)
    for bad_psf in (np.zeros((40, 39)), 'p', np.zeros(40), np.zeros((3, 40, 40))):
        with pytest.raises(ValueError):
            psfrec.fit_crowded_stars(image, bad_psf, pos)
    assert ctx.lib.calls == []
    ctx._h = None


def test_fit_found_stars_crowded_frame(monkeypatch):
    ctx = _frame_ctx(monkeypatch)
    pos, crit, shape = crowd()
    ref = G.group(pos, crit, shape)
    row = {int(r[2]): k for k, r in enumerate(ref['groups'])}
    grp = np.array([row[int(v)] for v in ref['label']])
    crowded = ref['groups'][grp, 1] != 0
    assert crowded.sum() == 9
    image = np.random.default_rng(1).normal(size=shape)
    psf = np.zeros((NS, NS))
    psf[20, 20] = 1.0
    found = {'position': pos, 'scale': np.arange(len(pos)) + 100.0}
    with pytest.raises(ValueError):
        psfrec.fit_found_stars(image, psf, found, crit=crit, crowded='all')
    with pytest.raises(ValueError):
        psfrec.fit_found_stars(image, psf, found, crit=crit, crowded='frame', radius=30)
    assert ctx.lib.calls == []
    skip, origin0 = psfrec.fit_found_stars(image, psf, found, crit=crit, pixscale=0.25)
    names0 = [c[0] for c in ctx.lib.calls]
    assert 'mpsfr_fit_frame_psf' not in names0 and 'mpsfr_render_stars' not in names0
    ctx.lib.calls.clear()
    fit, origin = psfrec.fit_found_stars(image, psf, found, crit=crit, pixscale=0.25, crowded='frame', radius=5.0,
                                         fit_back=False)
    names = [c[0] for c in ctx.lib.calls]
    assert names == names0 + ['mpsfr_render_stars', 'mpsfr_fit_frame_psf']
    assert tuple(fit.colnames) == tuple(skip.colnames) and len(fit) == len(pos)
    # the fitted singles and blends: as before, bit for bit
    for name in fit.colnames:
        np.testing.assert_array_equal(np.asarray(fit[name])[~crowded], np.asarray(skip[name])[~crowded])
    np.testing.assert_array_equal(fit['crowded'], crowded)
    # the render subtracted exactly those; the frame fit got the residual, the crowded stars and their found amplitudes
    r = ctx.lib.calls[-2][1]
    assert r[4] == (~crowded).sum() and r[11] == _lib.RENDER_SUBTRACT
    a = ctx.lib.calls[-1][1]
    idx = np.flatnonzero(crowded)
    own = (np.rint(pos[idx]) - 20).astype(np.int32)
    sh = pos[idx] - (own + 20)
    assert (a[1], a[2], a[5], a[6], a[12], a[13]) == (shape[0], shape[1], 9, 1, 5.0, 0)
    np.testing.assert_array_equal(_array(a[9], 18, C.c_int32, np.int32).reshape(9, 2), own)
    np.testing.assert_array_equal(_array(a[10], 18, C.c_double, np.float64).reshape(9, 2), sh)
    np.testing.assert_array_equal(_array(a[11], 9, C.c_double, np.float64), idx + 100.0)
    # origin gained one row per crowded star and their group column points at it
    assert origin.dtype == np.int32 and origin.shape == (len(origin0) + 9, 2)
    np.testing.assert_array_equal(origin[:len(origin0)], origin0)
    np.testing.assert_array_equal(origin[len(origin0):], own)
    np.testing.assert_array_equal(np.asarray(fit['group'])[idx], len(origin0) + np.arange(9))
    ok = np.ones(9, dtype=bool)
    ok[1] = False                                                # the stub leaves star 1 out
    F0 = 1000.0 * sh[:, 0] + sh[:, 1]
    np.testing.assert_array_equal(np.asarray(fit['scale'])[idx[ok]], F0[ok])
    np.testing.assert_array_equal(np.asarray(fit['flux'])[idx[ok]], 2.0 * F0[ok])
    np.testing.assert_array_equal(np.asarray(fit['shift'])[idx[ok]], sh[ok] * 0.25)
    np.testing.assert_array_equal(np.asarray(fit['err_shift'])[idx[ok]], 0.0)
    for name, val in (('err_scale', 1.0), ('err_flux', 2.0), ('back', 3.0), ('err_back', 0.5), ('chi2', 77.0),
                      ('npix', 1234), ('status', 0)):
        np.testing.assert_array_equal(np.asarray(fit[name])[idx[ok]], val)
    assert fit['status'][idx[1]] == 2 and np.isnan(fit['scale'][idx[1]])
    # subtract_stars now removes every fitted star, the crowded ones at their own origins
    ctx.lib.calls.clear()
    _, status = psfrec.subtract_stars(image, psf, origin, fit, psf_index=np.zeros(len(origin), dtype=int), pixscale=0.25)
    a = ctx.lib.calls[0][1]
    assert a[4] == len(pos) - 1 and np.count_nonzero(status == 0) == len(pos) - 1 and status[idx[1]] == -1
    ctx._h = None


# ---- 5. constants and exports
def test_exports_and_header_constants():
    assert 'mpsfr_fit_frame_psf' in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    assert int(re.search(r'#define MPSFR_NFRAMEFIT\s+(\d+)', hdr).group(1)) == _lib.NFRAMEFIT == 8
    assert float(re.search(r'#define MPSFR_FRAME_FIT_MAX_RADIUS\s+([\d.]+)', hdr).group(1)) == _lib.FRAME_FIT_MAX_RADIUS
    assert int(re.search(r'#define MPSFR_FRAME_FIT_MAX_ITER\s+(\d+)', hdr).group(1)) == _lib.FRAME_FIT_MAX_ITER == 1000
    # a disc stays inside its own footprint at any legal shift
    assert _lib.FRAME_FIT_MAX_RADIUS + _lib.FIT_PSF_MAX_SHIFT + 2 <= NS // 2 + _lib.RENDER_APRON
    assert re.search(r'int mpsfr_fit_frame_psf\(mpsfr_ctx\* ctx, int ny, int nx, const double\* image', hdr)
    assert 'CONDITIONAL' in hdr
    import muse_psfr_amd
    for name in ('fit_crowded_stars', 'fit_found_stars', 'NFRAMEFIT', 'FRAME_FIT_MAX_RADIUS'):
        assert hasattr(muse_psfr_amd, name), name
    assert 'frame_fit.hip' in __import__('muse_psfr_amd._build', fromlist=['SOURCES']).SOURCES
    assert (F.MAX_SHIFT, F.MAX_ORIGIN, F.NS) == (_lib.FIT_PSF_MAX_SHIFT, _lib.MAX_ORIGIN, NS)
