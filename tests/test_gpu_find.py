"""GPU: the star finder (mpsfr_find_stars), both precisions.

1. parity with the NumPy yardstick (find_ref) on the shared scene, with and without var, half 3 and 8, sep 1, 3 and 16:
   the count, the peak pixels, origin_out, the valid-pixel counts and the flags identical, the map NaN exactly where the
   reference has it; T, H, b, the positions and the sharpness within the a-priori bounds find_ref derives from its own
   sums of absolute terms ((n + 2) eps sum|terms| per sum, to first order through the formulas) -- no tuned constant.
   That the discrete answers are unambiguous at this accuracy is asserted on the reference (test_find_host.py).
2. small and odd frames: 1 x 1, 1 x 200, 200 x 1, a star on a tile corner of a 33 x 65 frame, an all-NaN frame, a tile
   masked by var.
3. exact cases: one pixel set in a frame of zeros against the closed expression; two equal pixels: equal bits of T, the
   lower index wins, both are peaks at sep = 1.
4. invariances, bit for bit: host = device pointers, mixed = f64, a second call, a call after other work of the
   context, map_out / origin_out given or NULL, and the scene moved to (5, 11) inside a 110 x 170 frame of NaN (every
   column but the positions, which add the offset to another pixel index: those within 2 ulp of the frame side).
5. overflow and filler rows; every raw call here checks canaries behind each output buffer.
6. the loop find -> cut -> fit -> subtract -> find on host pointers, and the faint neighbour found on the residual.
7. the same chain on device buffers at a fixed max_stars without synchronisation.
8. E_INVALID, degenerate cores in the device form, profiling.
Margins go to record_margin('find', ...).
"""
import ctypes as C

import numpy as np
import pytest

import find_ref as F
from conftest import record_margin

pytestmark = pytest.mark.gpu

PRECS = ['mixed', 'f64']
NS = 40
SENT, ISENT, CAN = -7.25, -77, 16
FILL = F.FILLER_ORIGIN


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


_CTX = {}


def _ctx(api, prec):
    if prec not in _CTX:
        _CTX[prec] = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision=prec)
    return _CTX[prec]


@pytest.fixture
def ctx(api, prec):
    return _ctx(api, prec)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def raw_find(ctx, image, psf, var=None, half=3, sep=3, threshold=5.0, max_stars=256, want_map=True, want_origin=True,
             expect_rc=0, override=None):
    """mpsfr_find_stars on host pointers with canaries behind every output.  Returns a dict: rc, rows (max_stars, 8),
    origin, count, map; after a refusal it asserts that every output is untouched."""
    ny, nx = image.shape
    image = np.ascontiguousarray(image, dtype=np.float64)
    var = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
    psf = np.ascontiguousarray(psf, dtype=np.float64)
    cap = max(max_stars, 1) if max_stars <= 1 << 20 else 1
    rows = np.full(cap * 8 + CAN, SENT)
    origin = np.full(cap * 2 + CAN, ISENT, dtype=np.int32)
    count = np.full(1 + CAN, ISENT, dtype=np.int32)
    tmap = np.full(ny * nx + CAN, SENT)
    a = dict(ny=ny, nx=nx, image=image, var=var, psf=psf, half=half, sep=sep, threshold=threshold, max_stars=max_stars,
             rows=rows, origin=origin if want_origin else None, count=count, map=tmap if want_map else None)
    a.update(override or {})
    rc = ctx.lib.mpsfr_find_stars(ctx._h, a['ny'], a['nx'], _ptr(a['image']), _ptr(a['var']), _ptr(a['psf']), a['half'],
                                  a['sep'], a['threshold'], a['max_stars'], _ptr(a['rows']), _ptr(a['origin']),
                                  _ptr(a['count']), _ptr(a['map']), 0)
    assert rc == expect_rc, (rc, ctx.lib.mpsfr_last_error())
    assert np.all(rows[cap * 8:] == SENT) and np.all(origin[cap * 2:] == ISENT) and np.all(count[1:] == ISENT)
    assert np.all(tmap[ny * nx:] == SENT)
    if rc != 0:
        assert np.all(rows == SENT) and np.all(origin == ISENT) and np.all(count == ISENT) and np.all(tmap == SENT)
    if not want_map:
        assert np.all(tmap == SENT)
    if not want_origin:
        assert np.all(origin == ISENT)
    return dict(rc=rc, rows=rows[:cap * 8].reshape(cap, 8), origin=origin[:cap * 2].reshape(cap, 2), count=int(count[0]),
                map=tmap[:ny * nx].reshape(ny, nx))


def assert_filler(got, n):
    assert np.all(np.isnan(got['rows'][n:])) and np.all(got['origin'][n:] == FILL)


def assert_parity(got, ref, tag=None, with_map=True):
    """The discrete answers identical, the floating-point ones within find_ref's a-priori bounds.  Returns the worst
    ratio error / bound.  with_map=False: of a call that did not take the map, everything but the map."""
    n = ref['count']
    assert got['count'] == n and n <= len(got['rows'])
    rows, want = got['rows'][:n], ref['rows']
    ny, nx = ref['shape']
    pix = (got['origin'][:n, 0].astype(np.int64) + NS // 2) * nx + got['origin'][:n, 1] + NS // 2
    assert np.array_equal(pix, ref['index']) and np.array_equal(got['origin'][:n], ref['origin'])
    assert np.array_equal(rows[:, 6], want[:, 6]) and np.array_equal(rows[:, 7], want[:, 7])
    assert_filler(got, n)
    worst = 0.0
    if with_map:
        nan = np.isnan(ref['map'])
        assert np.array_equal(np.isnan(got['map']), nan)
        err, bnd = np.abs(got['map'] - ref['map'])[~nan], F.stat_bounds(ref)[0][~nan]
        some = bnd > 0
        worst = float(np.max(err[some] / bnd[some])) if some.any() else 0.0
        print('%s map: worst error / bound %.3f' % (tag, worst))
        assert np.all(err <= bnd), ('map', worst)
    if n:
        bound = F.row_bounds(ref)
        assert np.array_equal(np.isnan(rows[:, 5]), np.isnan(want[:, 5]))
        for col in range(6):
            fin = np.isfinite(want[:, col])
            err = np.abs(rows[fin, col] - want[fin, col])
            ratio = float(np.max(err / np.maximum(bound[fin, col], 1e-300))) if fin.any() else 0.0
            exact = bool(np.all(err == 0))
            print('%s column %d: worst error / bound %.3f' % (tag, col, 0.0 if exact else ratio))
            assert exact or ratio <= 1.0, (col, ratio)
            worst = max(worst, 0.0 if exact else ratio)
    return worst


# ---- 1. parity on the scene
@pytest.mark.parametrize('sep', [1, 3, 16])
@pytest.mark.parametrize('half', [3, 8])
@pytest.mark.parametrize('usevar', [True, False])
@pytest.mark.parametrize('prec', PRECS)
def test_parity_with_numpy_on_the_scene(ctx, prec, usevar, half, sep):
    s = F.scene()
    thr = F.THRESHOLD[usevar]
    ref = F.scene_reference(usevar, half, sep, thr)
    assert ref['count'] >= 10
    got = raw_find(ctx, s['image'], s['psf'], s['var'] if usevar else None, half, sep, thr)
    worst = assert_parity(got, ref, 'scene var=%d half=%d sep=%d' % (usevar, half, sep))
    record_margin('find', **{'scene_%s' % prec: worst})


# ---- 2. small and odd frames
@pytest.mark.parametrize('shape', [(1, 1), (1, 200), (200, 1)])
@pytest.mark.parametrize('prec', PRECS)
def test_degenerate_frames_have_no_peaks(ctx, prec, shape):
    rng = np.random.default_rng(4)
    image = 100.0 + rng.normal(size=shape)
    for var in (None, np.ones(shape)):
        got = raw_find(ctx, image, F.model(), var, 3, 3, -1e300, max_stars=9)
        assert got['count'] == 0 and np.all(np.isnan(got['map']))
        assert_filler(got, 0)
    # half = 1 on a single row: 3 of the 9 window pixels at most -- still no majority
    assert raw_find(ctx, image, F.model(), None, 1, 1, -1e300, max_stars=9)['count'] == 0


@pytest.mark.parametrize('prec', PRECS)
def test_a_star_on_a_tile_corner_of_an_odd_frame(ctx, prec):
    rng = np.random.default_rng(8)
    shape = (33, 65)
    var = rng.uniform(0.5, 1.5, shape)
    image = 3.0 + rng.normal(size=shape) * np.sqrt(var) + 800.0 * F.moffat(31.4, 31.6, shape) / F.moffat(20, 20).sum()
    for half, sep in ((3, 3), (8, 16), (1, 1)):
        ref = F.find(image, var, F.model(), half, sep, 12.0)
        got = raw_find(ctx, image, F.model(), var, half, sep, 12.0, max_stars=16)
        assert_parity(got, ref, 'corner half=%d' % half)
        assert 31 * 65 + 32 in ref['index'] or 31 * 65 + 31 in ref['index']


@pytest.mark.parametrize('prec', PRECS)
def test_all_nan_frame_and_a_tile_masked_by_var(ctx, prec):
    got = raw_find(ctx, np.full((70, 40), np.nan), F.model(), None, 3, 3, -1e300, max_stars=5)
    assert got['count'] == 0 and np.all(np.isnan(got['map']))
    assert_filler(got, 0)
    s = F.scene()
    var = s['var'].copy()
    var[32:64, 32:64] = 0.0
    var[64:96, 96:128] = np.nan
    var[0:32, 64:96] = -1.0
    var[70, 10] = np.inf
    ref = F.find(s['image'], var, s['psf'], 3, 3, 5.0)
    got = raw_find(ctx, s['image'], s['psf'], var, 3, 3, 5.0)
    assert_parity(got, ref, 'masked tiles')
    assert np.all(np.isnan(got['map'][32:64, 32:64])) and ref['count'] < F.scene_reference()['count']


# ---- 3. exact cases
@pytest.mark.parametrize('prec', PRECS)
def test_one_pixel_in_a_frame_of_zeros(ctx, prec):
    image = np.zeros((41, 45))
    image[20, 22] = 1.0
    psf = F.model()
    for half in (3, 8):
        K = F.core(psf, half)
        W = 2 * half + 1
        # S0 = W^2, S3 = 1 and S4 = the tap are exact: H = (K_tap - S1 / S0) / den
        S0, S1, S2 = float(W * W), float(np.sum(K.astype(np.longdouble))), float(np.sum(K.astype(np.longdouble) ** 2))
        den = S2 - S1 * S1 / S0
        expr = (K[::-1, ::-1] - S1 / S0) / den                        # pixel (20 + a, 22 + b) sees the pixel at tap (-a, -b)
        thr = 0.5 * float(expr[half, half])
        ref = F.find(image, None, psf, half, 3, thr)
        got = raw_find(ctx, image, psf, None, half, 3, thr, max_stars=4)
        assert_parity(got, ref, 'one pixel')
        dT = F.stat_bounds(ref)[0]
        sl = (slice(20 - half, 21 + half), slice(22 - half, 23 + half))
        assert np.all(np.abs(got['map'][sl] - expr) <= dT[sl])
        # by hand: the core has its only maximum at the centre, so the map has its own at the pixel
        assert got['count'] == 1 and np.array_equal(got['origin'][0], [0, 2])
        row = got['rows'][0]
        assert row[0] == 20.0 and row[1] == 22.0 and row[6] == W * W and row[7] == 0        # a symmetric core: offset 0
        assert row[5] > 3 and abs(row[3] - expr[half, half]) <= dT[20, 22] and row[2] == got['map'][20, 22]


@pytest.mark.parametrize('prec', PRECS)
def test_two_equal_pixels_the_lower_index_wins(ctx, prec):
    y, x = np.mgrid[:NS, :NS]
    psf = np.exp(-((y - 20.0) ** 2 + (x - 20.0) ** 2) / (2 * 0.6 ** 2))       # narrow and left-right symmetric, bit for bit
    assert np.array_equal(psf[:, 1:], psf[:, :0:-1]) and 2 * psf[20, 21] < psf[20, 20]
    image = np.zeros((41, 45))
    image[20, 20] = image[20, 22] = 3.0
    for sep in (2, 3, 16):
        got = raw_find(ctx, image, psf, None, 3, sep, 1.0, max_stars=4)
        m = got['map']
        assert _same(m[20, 20], m[20, 22]) and m[20, 21] < m[20, 20]
        assert got['count'] == 1 and np.array_equal(got['origin'][0] + NS // 2, [20, 20])
    got = raw_find(ctx, image, psf, None, 3, 1, 1.0, max_stars=4)
    assert got['count'] == 2 and np.array_equal(got['origin'][:2] + NS // 2, [[20, 20], [20, 22]])
    assert _same(got['rows'][0, 2:], got['rows'][1, 2:])
    assert_filler(got, 2)


# ---- 4. invariances, bit for bit
def _to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda:0'))


def _device_find(ctx, image, psf, var, half, sep, thr, max_stars, want_map=True, want_origin=True):
    import torch
    ny, nx = image.shape
    dev = torch.device('cuda:0')
    tim, tps = _to_dev(torch, image), _to_dev(torch, psf)
    tva = None if var is None else _to_dev(torch, var)
    trow = torch.full((max_stars * 8 + CAN,), SENT, dtype=torch.float64, device=dev)
    tor = torch.full((max_stars * 2 + CAN,), ISENT, dtype=torch.int32, device=dev)
    tct = torch.full((1 + CAN,), ISENT, dtype=torch.int32, device=dev)
    tmp = torch.full((ny * nx + CAN,), SENT, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.find_stars_device(ny, nx, tim.data_ptr(), tps.data_ptr(), half, sep, thr, max_stars, trow.data_ptr(),
                          tct.data_ptr(), var_ptr=None if tva is None else tva.data_ptr(),
                          origin_ptr=tor.data_ptr() if want_origin else None, map_ptr=tmp.data_ptr() if want_map else None)
    ctx.sync()
    rows, origin, count, tmap = trow.cpu().numpy(), tor.cpu().numpy(), tct.cpu().numpy(), tmp.cpu().numpy()
    assert np.all(rows[max_stars * 8:] == SENT) and np.all(origin[max_stars * 2:] == ISENT)
    assert np.all(count[1:] == ISENT) and np.all(tmap[ny * nx:] == SENT)
    return dict(rows=rows[:max_stars * 8].reshape(-1, 8), origin=origin[:max_stars * 2].reshape(-1, 2),
                count=int(count[0]), map=tmap[:ny * nx].reshape(ny, nx))


_BASE = {}


def _base(api, prec, usevar=True):
    """The scene through the host-pointer call at half = sep = 3, once per precision."""
    if (prec, usevar) not in _BASE:
        s = F.scene()
        _BASE[prec, usevar] = raw_find(_ctx(api, prec), s['image'], s['psf'], s['var'] if usevar else None, 3, 3,
                                       F.THRESHOLD[usevar])
    return _BASE[prec, usevar]


def _equal(a, b):
    return a['count'] == b['count'] and _same(a['rows'], b['rows']) and _same(a['origin'], b['origin']) and \
        _same(a['map'], b['map'])


@pytest.mark.parametrize('usevar', [True, False])
@pytest.mark.parametrize('prec', PRECS)
def test_device_pointers_equal_host_pointers(api, ctx, prec, usevar):
    s = F.scene()
    got = _device_find(ctx, s['image'], s['psf'], s['var'] if usevar else None, 3, 3, F.THRESHOLD[usevar], 256)
    assert _equal(got, _base(api, prec, usevar))
    bare = _device_find(ctx, s['image'], s['psf'], s['var'] if usevar else None, 3, 3, F.THRESHOLD[usevar], 256,
                        want_map=False, want_origin=False)
    assert _same(bare['rows'], got['rows']) and bare['count'] == got['count']
    assert np.all(bare['map'] == SENT) and np.all(bare['origin'] == ISENT)


def test_mixed_equals_f64(api):
    for usevar in (True, False):
        assert _equal(_base(api, 'mixed', usevar), _base(api, 'f64', usevar))
    assert _base(api, 'f64')['count'] == F.scene_reference()['count']


@pytest.mark.parametrize('prec', PRECS)
def test_a_call_does_not_depend_on_the_calls_before_it(api, ctx, prec):
    import render_ref as Y
    s = F.scene()
    base = _base(api, prec)
    assert _equal(raw_find(ctx, s['image'], s['psf'], s['var'], 3, 3, 5.0), base)
    # another frame shape, other parameters, then the renderer and a fit on the same context
    raw_find(ctx, s['image'][:50, :70], s['psf'], None, 8, 16, 100.0, max_stars=3)
    r = Y.scene()
    ctx.render_stars(r['psf'], r['origin'], r['scale'], shift=r['shift'], psf_index=r['index'], image=r['image'])
    stamps = ctx.cut_stamps(s['image'], base['origin'][:6])
    ctx.fit_stamps_psf(stamps, s['psf'][None], psf_index=np.zeros(6, dtype=np.int32))
    assert _equal(raw_find(ctx, s['image'], s['psf'], s['var'], 3, 3, 5.0), base)
    for kw in (dict(want_map=False), dict(want_origin=False), dict(want_map=False, want_origin=False)):
        got = raw_find(ctx, s['image'], s['psf'], s['var'], 3, 3, 5.0, **kw)
        assert got['count'] == base['count'] and _same(got['rows'], base['rows'])
        if kw.get('want_map', True):
            assert _same(got['map'], base['map'])
        if kw.get('want_origin', True):
            assert _same(got['origin'], base['origin'])


@pytest.mark.parametrize('usevar', [True, False])
@pytest.mark.parametrize('prec', PRECS)
def test_the_scene_moved_inside_a_larger_frame(api, ctx, prec, usevar):
    s = F.scene()
    base = _base(api, prec, usevar)
    off, shape = (5, 11), (110, 170)
    image = F.embed(s['image'], shape, off)
    var = F.embed(s['var'], shape, off, fill=1.0) if usevar else None
    got = raw_find(ctx, image, s['psf'], var, 3, 3, F.THRESHOLD[usevar])
    n = base['count']
    assert got['count'] == n
    assert _same(got['rows'][:, 2:], base['rows'][:, 2:])              # T, H, b, sharpness, pixels, flags: the same bits
    assert np.array_equal(got['origin'][:n], base['origin'][:n] + np.array(off, dtype=np.int32))
    assert np.all(got['origin'][n:] == FILL)
    assert np.all(np.abs(got['rows'][:n, :2] - (base['rows'][:n, :2] + off)) <= 2 * F.EPS * max(shape))
    inner = got['map'][off[0]:off[0] + F.FRAME[0], off[1]:off[1] + F.FRAME[1]]
    assert _same(inner, base['map'])
    outer = got['map'].copy()
    outer[off[0]:off[0] + F.FRAME[0], off[1]:off[1] + F.FRAME[1]] = np.nan
    assert np.all(np.isnan(outer))


# ---- 5. overflow and filler
@pytest.mark.parametrize('prec', PRECS)
def test_overflow_and_filler_rows(api, ctx, prec):
    s = F.scene()
    base = _base(api, prec)
    n = base['count']
    for cap in (1, 7):
        got = raw_find(ctx, s['image'], s['psf'], s['var'], 3, 3, 5.0, max_stars=cap)
        assert got['count'] == n and _same(got['rows'], base['rows'][:cap]) and _same(got['origin'], base['origin'][:cap])
    got = raw_find(ctx, s['image'], s['psf'], s['var'], 3, 3, 5.0, max_stars=n)
    assert got['count'] == n and _same(got['rows'], base['rows'][:n])
    got = raw_find(ctx, s['image'], s['psf'], s['var'], 3, 3, 5.0, max_stars=n + 5)
    assert got['count'] == n and _same(got['rows'][:n], base['rows'][:n]) and len(got['rows']) == n + 5
    assert_filler(got, n)
    # a filler origin is legal for the frame calls: an all-NaN stamp, fit status 2, render status 1 or 2
    stamps = ctx.cut_stamps(s['image'], got['origin'][n:])
    assert np.all(np.isnan(stamps))
    fit = ctx.fit_stamps_psf(stamps, s['psf'][None], psf_index=np.zeros(5, dtype=np.int32))
    assert np.all(fit[:, 10] == 2)
    # the wrapper of the context trims to the count
    rows, origin, nfound = ctx.find_stars(s['image'], s['psf'], var=s['var'], max_stars=n + 5)
    assert nfound == n and _same(rows, base['rows'][:n]) and _same(origin, base['origin'][:n])
    rows, origin, nfound, tmap = ctx.find_stars(s['image'], s['psf'], var=s['var'], max_stars=7, return_map=True)
    assert nfound == n and _same(rows, base['rows'][:7]) and _same(tmap, base['map'])


# ---- 6. the loop on host pointers
def _loop_field():
    """12 well-separated stars on a 230 x 300 frame of background 5 and unit-variance noise, rendered by the library's
    own resampling: (truth positions, fluxes)."""
    rng = np.random.default_rng(12)
    grid = np.array([(40 + 50 * i, 40 + 55 * j) for i in range(3) for j in range(4)], dtype=float)
    return grid + rng.uniform(-3, 3, grid.shape), rng.uniform(800, 3000, 12)


def _loop_frame(ctx, extra=None):
    pos, flux = _loop_field()
    if extra is not None:
        pos, flux = np.concatenate([pos, extra[0]]), np.concatenate([flux, extra[1]])
    origin = (np.rint(pos) - NS // 2).astype(np.int32)
    psf = F.model()[None]
    noise = np.random.default_rng(13).normal(size=(230, 300))
    frame = ctx.render_stars(psf, origin, flux, shift=pos - np.rint(pos), psf_index=np.zeros(len(pos), dtype=np.int32),
                             image=5.0 + noise)
    return frame, np.ones_like(frame), psf, pos, flux


@pytest.mark.parametrize('prec', PRECS)
def test_find_cut_fit_subtract_find_again(api, ctx, prec, monkeypatch):
    monkeypatch.setattr(api.psfrec, 'get_context', lambda *a, **k: ctx)
    frame, var, psf, pos, flux = _loop_frame(ctx)
    ps = 0.2
    found = api.find_stars(frame, psf[0], var, threshold=5.0, half=3, pixscale=ps)
    assert len(found) == 12
    stamps, vstamps, origin = api.cut_star_stamps(frame, found['position'], var, pixscale=ps)
    assert np.array_equal(origin, found['origin'])
    index = np.zeros(12, dtype=np.int32)
    fit = api.fit_stars_with_psf(stamps, psf, var=vstamps, psf_index=index, shift=found['shift'], pixscale=ps)
    assert np.all(np.asarray(fit['status']) == 0)
    where = origin + NS // 2 + np.asarray(fit['shift']) / ps
    near = np.argmin(((where[:, None] - pos[None]) ** 2).sum(-1), axis=1)
    assert sorted(near) == list(range(12))
    err = np.abs(where - pos[near]) / (np.asarray(fit['err_shift']) / ps)
    print('loop %s: worst position error %.2f sigma' % (prec, err.max()))
    assert err.max() < 5.0                                                # within the fit's own error
    assert np.all(np.abs(np.asarray(fit['scale']) - flux[near]) < 5 * np.asarray(fit['err_scale']))
    residual, status = api.subtract_stars(frame, psf, origin, fit, psf_index=index, pixscale=ps)
    assert np.all(status == 0)
    assert len(api.find_stars(residual, psf[0], var, threshold=5.0, half=3, pixscale=ps)) == 0
    # a faint star 5 px from one ten times brighter: no peak of the frame at sep = 5, found on the residual
    k = int(np.argmax(flux))
    faint = pos[k] + np.array([5.0, 0.3])
    frame2, var, psf, pos2, flux2 = _loop_frame(ctx, (faint[None], np.array([flux[k] / 10])))
    found = api.find_stars(frame2, psf[0], var, threshold=5.0, half=3, sep=5, pixscale=ps)
    assert len(found) == 12 and np.min(np.abs(np.asarray(found['position']) - faint).max(axis=1)) > 2.0
    stamps, vstamps, origin = api.cut_star_stamps(frame2, found['position'], var, pixscale=ps)
    fit = api.fit_stars_with_psf(stamps, psf, var=vstamps, psf_index=index, shift=found['shift'], pixscale=ps)
    residual, status = api.subtract_stars(frame2, psf, origin, fit, psf_index=index, pixscale=ps)
    again = api.find_stars(residual, psf[0], var, threshold=5.0, half=3, sep=5, pixscale=ps)
    assert len(again) >= 1
    assert np.abs(np.asarray(again['position'])[0] - faint).max() < 1.0     # the brightest peak of the residual


# ---- 7. the same chain on device buffers
@pytest.mark.parametrize('prec', PRECS)
def test_the_chain_on_device_buffers_at_a_fixed_size(api, ctx, prec):
    import torch
    frame, var, psf, pos, flux = _loop_frame(ctx)
    ny, nx = frame.shape
    M = 32
    # host pointers, on the rows that are there
    rows, origin, n = ctx.find_stars(frame, psf[0], var=var, half=3, sep=3, threshold=5.0, max_stars=M)
    assert n == 12
    start = rows[:, :2] - (origin + NS // 2)
    stamps, vstamps = ctx.cut_stamps(frame, origin, var=var)
    index = np.zeros(n, dtype=np.int32)
    fit = ctx.fit_stamps_psf(stamps, psf, var=vstamps, psf_index=index, shift=start)
    assert np.all(fit[:, 10] == 0)
    res, rstat = ctx.render_stars(psf, origin, fit[:, 0], shift=fit[:, 1:3], psf_index=index, image=frame, subtract=True,
                                  return_status=True)
    # device buffers of one context, at the fixed size M, nothing waited for in between
    dev = torch.device('cuda:0')
    tfr, tva, tps = _to_dev(torch, frame), _to_dev(torch, var), _to_dev(torch, psf)
    tix = torch.zeros(M, dtype=torch.int32, device=dev)
    trow = torch.empty((M, 8), dtype=torch.float64, device=dev)
    tor = torch.empty((M, 2), dtype=torch.int32, device=dev)
    tct = torch.empty(1, dtype=torch.int32, device=dev)
    tst = torch.empty((M, NS, NS), dtype=torch.float64, device=dev)
    tvs = torch.empty((M, NS, NS), dtype=torch.float64, device=dev)
    tfit = torch.empty((M, api.NFIT_PSF), dtype=torch.float64, device=dev)
    tstart = torch.empty((M, 2), dtype=torch.float64, device=dev)
    tsc, tsh = torch.empty(M, dtype=torch.float64, device=dev), torch.empty((M, 2), dtype=torch.float64, device=dev)
    tres = torch.empty_like(tfr)
    trs = torch.empty((M, 4), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ext = torch.cuda.ExternalStream(ctx.stream_handle())
    ctx.find_stars_device(ny, nx, tfr.data_ptr(), tps.data_ptr(), 3, 3, 5.0, M, trow.data_ptr(), tct.data_ptr(),
                          var_ptr=tva.data_ptr(), origin_ptr=tor.data_ptr())
    with torch.cuda.stream(ext):                                   # (on the context's own stream: no sync)
        tstart.copy_(trow[:, :2] - (tor + NS // 2))
    ctx.cut_stamps_device(ny, nx, tfr.data_ptr(), M, tor.data_ptr(), tst.data_ptr(), var_ptr=tva.data_ptr(),
                          var_stamps_ptr=tvs.data_ptr())
    ctx.fit_stamps_psf_device(M, tst.data_ptr(), 1, tps.data_ptr(), tfit.data_ptr(), var_ptr=tvs.data_ptr(),
                              psf_index_ptr=tix.data_ptr(), shift_ptr=tstart.data_ptr())
    with torch.cuda.stream(ext):
        tsc.copy_(tfit[:, 0])
        tsh.copy_(tfit[:, 1:3])
    ctx.render_stars_device(ny, nx, M, 1, tps.data_ptr(), tor.data_ptr(), tsc.data_ptr(), tres.data_ptr(),
                            image_ptr=tfr.data_ptr(), shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr(),
                            star_out_ptr=trs.data_ptr(), subtract=True)
    ctx.sync()
    drow, dor, dfit, drs = trow.cpu().numpy(), tor.cpu().numpy(), tfit.cpu().numpy(), trs.cpu().numpy()
    assert int(tct.cpu().numpy()[0]) == n
    assert _same(drow[:n], rows) and _same(dor[:n], origin) and _same(dfit[:n], fit) and _same(drs[:n], rstat)
    assert np.all(np.isnan(drow[n:])) and np.all(dor[n:] == FILL)
    assert np.all(dfit[n:, 10] == 2) and np.all((drs[n:, 0] == 1) | (drs[n:, 0] == 2))
    assert _same(tres.cpu().numpy(), res)                               # the filler rows changed nothing


# ---- 8. refusals, degenerate cores, profiling
def test_bad_arguments_are_refused_and_leave_the_outputs(api):
    ctx = _ctx(api, 'mixed')
    rng = np.random.default_rng(6)
    image, var, psf = rng.normal(size=(50, 70)), np.ones((50, 70)), F.model()
    flat, bad = psf.copy(), psf.copy()
    flat[17:24, 17:24] = 0.5
    bad[18, 23] = np.nan
    inf = psf.copy()
    inf[20, 20] = np.inf
    cases = [dict(ny=0), dict(nx=0), dict(ny=-1), dict(ny=16385), dict(nx=16385), dict(ny=8193, nx=8192),
             dict(image=None), dict(psf=None), dict(rows=None), dict(count=None),
             dict(half=0), dict(half=9), dict(half=-3), dict(half=21), dict(sep=0), dict(sep=17), dict(sep=-1),
             dict(max_stars=0), dict(max_stars=-4), dict(max_stars=(1 << 24) + 1),
             dict(threshold=np.nan), dict(threshold=np.inf), dict(threshold=-np.inf),
             dict(psf=flat), dict(psf=bad), dict(psf=inf)]
    for kw in cases:
        for v in (None, var):
            raw_find(ctx, image, psf, v, 3, 3, 5.0, max_stars=8, expect_rc=-1, override=kw)
        assert b'find_stars' in ctx.lib.mpsfr_last_error(), kw
    # their neighbours are legal: the core constant at half = 3 is a filter at half = 4, the NaN lies outside half = 1
    assert raw_find(ctx, image, flat, None, 4, 16, -1e300, max_stars=1 << 10)['count'] > 0
    assert raw_find(ctx, image, bad, var, 1, 1, 0.0, max_stars=8)['rc'] == 0
    assert raw_find(ctx, image, psf, var, 8, 16, 1e300, max_stars=8)['count'] == 0
    # the device form does not look at the core: no peaks, count 0
    for core in (flat, bad, inf, np.full((NS, NS), 1.0 / 3.0), np.zeros((NS, NS))):
        for v in (None, var):
            got = _device_find(ctx, image, core, v, 3, 3, -1e300, 8)
            assert got['count'] == 0 and np.all(np.isnan(got['map'])), core[20, 20]
            assert np.all(np.isnan(got['rows'])) and np.all(got['origin'] == FILL)


def test_timed_under_the_profiling_id_of_the_fit(api):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    s = F.scene()
    assert ctx.lib.mpsfr_profile_count() == 16 and ctx.lib.mpsfr_version() == 102
    ctx.set_option('profile', 1)
    ctx.profile_reset()
    rows, origin, n = ctx.find_stars(s['image'], s['psf'], var=s['var'])
    prof = ctx.profile()
    assert n == F.scene_reference()['count'] and prof['fit'][1] == 1 and prof['fit'][0] > 0
    ctx.find_stars(s['image'], s['psf'], half=8, sep=16, threshold=F.THRESHOLD[False], return_map=True)
    prof = ctx.profile()
    assert prof['fit'][1] == 2
    assert all(v[1] == 0 for k, v in prof.items() if k != 'fit'), prof
    ctx.close()
