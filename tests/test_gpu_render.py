"""GPU: the frame calls (mpsfr_cut_stamps, mpsfr_render_stars), both precisions.

1. parity with the NumPy yardstick (render_ref) on the shared scene -- a 97 x 150 frame, 64 stars on four models over
   every tile border, the four edges, two corners and off the frame, and a pile of 300 stars that is longer than the
   list the kernel sorts in LDS -- in add and in subtract mode: per pixel |gpu - ref| <= 1e-13 S, S = |image_in| + the
   sum over the stars reaching the pixel of |scale| max|P| (derived in DESIGN.md section 21, not tuned); NaN pixels stay
   NaN and poison nothing; the pixel counts of star_out; degenerate frames 1 x 1, 1 x 200, 200 x 1.
2. exact cases, bit for bit: one star without shift is the model stamp itself, whole-pixel shifts displace it.
3. invariances, bit for bit: split calls, in place, host = device pointers, mixed = f64, the scene moved in a larger
   frame, skipped stars interleaved, two disjoint stars swapped, a shared model stamp, a second identical call.
4. cut: NumPy slicing bit for bit, NaN / 0 off the frame, device = host.
5. the loop frame -> cut -> fit -> subtract, on host and on device pointers; the psfrec wrappers.
6. refusals and skipped rows.  7. profiling.
Margins go to record_margin('render', ...).
"""
import ctypes as C

import numpy as np
import pytest

import render_ref as Y
from conftest import H, record_margin

pytestmark = pytest.mark.gpu

TOL = {'f64': 1e-8, 'mixed': 1e-4}            # tests/test_gpu_psf_fit.py
PARITY = 1e-13
PRECS = ['mixed', 'f64']
NS = 40


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


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _render(ctx, s, rows=slice(None), image='scene', **kw):
    return ctx.render_stars(s['psf'], s['origin'][rows], s['scale'][rows], shift=s['shift'][rows],
                            psf_index=s['index'][rows], image=s['image'] if isinstance(image, str) else image, **kw)


_BASE = {}


def _base(ctx, prec):
    """The add-mode render of the scene with its rows, once per precision."""
    if prec not in _BASE:
        _BASE[prec] = _render(ctx, Y.scene(), return_status=True)
    return _BASE[prec]


def _worst_ratio(got, want, S):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    return float(np.max(np.abs(got - want)[~nan] / S[~nan]))


# ---- 1. parity
@pytest.mark.parametrize('subtract', [False, True])
@pytest.mark.parametrize('prec', PRECS)
def test_parity_with_numpy_on_the_scene(api, ctx, prec, subtract):
    s = Y.scene()
    assert Y.PILE > api.RENDER_SORT_CHUNK and Y.longest_tile_list(s) > api.RENDER_SORT_CHUNK
    want, npix, S = Y.scene_reference(subtract)
    got, rows = _render(ctx, s, subtract=subtract, return_status=True)
    assert got.shape == Y.FRAME and rows.shape == (s['n'], api.NRENDER)
    # NaN pixels of the image stay NaN and nothing else is: 136 pixels in 97 x 150
    assert np.array_equal(np.isnan(got), np.isnan(s['image'])) and np.isnan(got).sum() > 50
    worst = _worst_ratio(got, want, S)
    print('render parity %s %s: worst |gpu - ref| / S %.2e' % (prec, 'subtract' if subtract else 'add', worst))
    record_margin('render', **{'parity_%s_%s' % (prec, 'sub' if subtract else 'add'): worst / PARITY})
    assert worst <= PARITY
    assert np.array_equal(rows[:, 1], npix) and np.all(rows[:, 2:] == 0)
    assert np.array_equal(rows[:, 0], np.where(npix == 0, 1, 0))
    assert sorted(np.flatnonzero(rows[:, 0] == 1)) == sorted(s['off_frame'])


@pytest.mark.parametrize('shape', [(1, 1), (1, 200), (200, 1)])
@pytest.mark.parametrize('prec', PRECS)
def test_parity_on_degenerate_frames(ctx, prec, shape):
    rng = np.random.default_rng(shape[1])
    psf = Y.models()
    origin = np.array([[-20, -20], [-45, shape[1] - 30], [shape[0] - 5, -49], [-3, shape[1] // 2 - 20], [-60, 0]],
                      dtype=np.int32)
    shift, scale, index = rng.uniform(-8, 8, (5, 2)), rng.uniform(-50, 50, 5), np.array([3, 2, 1, 0, 2], dtype=np.int32)
    image = rng.normal(size=shape)
    for subtract in (False, True):
        want, npix, S = Y.render(image, psf, index, origin, shift, scale, subtract)
        got, rows = ctx.render_stars(psf, origin, scale, shift=shift, psf_index=index, image=image, subtract=subtract,
                                     return_status=True)
        worst = _worst_ratio(got, want, S)
        record_margin('render', **{'parity_%s_%dx%d' % (prec, shape[0], shape[1]): worst / PARITY})
        assert worst <= PARITY
        assert np.array_equal(rows[:, 1], npix) and npix[0] > 0 and npix[4] == 0 and rows[4, 0] == 1
    # without an image: zeros
    want, _, S = Y.render(None, psf, index, origin, shift, scale, shape=shape)
    got = ctx.render_stars(psf, origin, scale, shift=shift, psf_index=index, shape=shape)
    assert np.max(np.abs(got - want) / np.where(S > 0, S, 1.0)) <= PARITY


# ---- 2. exact cases
@pytest.mark.parametrize('prec', PRECS)
def test_one_star_is_its_model_stamp_bit_for_bit(ctx, prec):
    P = Y.models()[1][None]
    shape, origin = (90, 110), np.array([[23, 37]], dtype=np.int32)
    for scale in (1.0, 2.0 ** -7):
        for shift in ((0.0, 0.0), (2.0, -3.0), (-8.0, 8.0)):
            got = ctx.render_stars(P, origin, [scale], shift=None if shift == (0.0, 0.0) and scale == 1.0 else [shift],
                                   shape=shape)
            want = np.zeros(shape)
            y, x = 23 + int(shift[0]), 37 + int(shift[1])
            want[y:y + NS, x:x + NS] = scale * P[0]
            assert _same(got, want), (scale, shift)              # (+0 everywhere else: the bit patterns are compared)


# ---- 3. invariances, bit for bit
@pytest.mark.parametrize('prec', PRECS)
def test_one_call_equals_two_consecutive_calls(ctx, prec):
    s = Y.scene()
    base, rows = _base(ctx, prec)
    for m in (1, 17, 63, 64 + 150):
        first = _render(ctx, s, slice(0, m))
        both = _render(ctx, s, slice(m, None), image=first)
        assert _same(both, base), m
    # a second identical call on the same context: the work lists hold no stale state
    again, rows2 = _render(ctx, s, return_status=True)
    assert _same(again, base) and _same(rows2, rows)


def test_mixed_equals_f64(api):
    ctxs = {p: _CTX.get(p) or api.Context(dim=128, pixscale=api.grid_pixscale(128), precision=p) for p in PRECS}
    _CTX.update(ctxs)
    a, ra = _base(ctxs['mixed'], 'mixed')
    b, rb = _base(ctxs['f64'], 'f64')
    assert _same(a, b) and _same(ra, rb)
    s = Y.scene()
    assert _same(_render(ctxs['mixed'], s, subtract=True), _render(ctxs['f64'], s, subtract=True))


def _to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda:0'))


@pytest.mark.parametrize('prec', PRECS)
def test_device_pointers_and_in_place_equal_host_pointers(ctx, prec):
    import torch
    s = Y.scene()
    base, rows = _base(ctx, prec)
    n, (ny, nx) = s['n'], Y.FRAME
    tim, tps, tix = _to_dev(torch, s['image']), _to_dev(torch, s['psf']), _to_dev(torch, s['index'])
    tor, tsh, tsc = _to_dev(torch, s['origin']), _to_dev(torch, s['shift']), _to_dev(torch, s['scale'])
    tout = torch.full((ny, nx), -1.0, dtype=torch.float64, device=tim.device)
    trow = torch.full((n, 4), -1.0, dtype=torch.float64, device=tim.device)
    torch.cuda.synchronize()
    ctx.render_stars_device(ny, nx, n, 4, tps.data_ptr(), tor.data_ptr(), tsc.data_ptr(), tout.data_ptr(),
                            image_ptr=tim.data_ptr(), shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr(),
                            star_out_ptr=trow.data_ptr())
    # in place, queued behind it on the same stream
    ctx.render_stars_device(ny, nx, n, 4, tps.data_ptr(), tor.data_ptr(), tsc.data_ptr(), tim.data_ptr(),
                            image_ptr=tim.data_ptr(), shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr())
    ctx.sync()
    assert _same(tout.cpu().numpy(), base) and _same(trow.cpu().numpy(), rows)
    assert _same(tim.cpu().numpy(), base)


@pytest.mark.parametrize('prec', PRECS)
def test_the_scene_moved_inside_a_larger_frame(ctx, prec):
    base, _ = _base(ctx, prec)
    moved = _render(ctx, Y.scene((5, 11), (110, 170)))
    assert moved.shape == (110, 170)
    assert _same(moved[5:5 + Y.FRAME[0], 11:11 + Y.FRAME[1]], base)


@pytest.mark.parametrize('prec', PRECS)
def test_skipped_and_swapped_stars_and_shared_stamps(ctx, prec):
    import torch
    s = Y.scene()
    base, rows = _base(ctx, prec)
    n = s['n']
    # a star off the frame (status 1) after every fifth star: nothing changes
    keep = np.ones(n + n // 5, dtype=bool)
    keep[5::6] = False
    def spread(a, fill):
        out = np.empty((keep.size,) + a.shape[1:], dtype=a.dtype)
        out[keep], out[~keep] = a, fill
        return out
    t = dict(psf=s['psf'], image=s['image'], origin=spread(s['origin'], np.array([-70, 400], dtype=np.int32)),
             shift=spread(s['shift'], 0.5), scale=spread(s['scale'], 1e6), index=spread(s['index'], 1))
    got, r = _render(ctx, t, return_status=True)
    assert _same(got, base) and _same(r[keep], rows) and np.all(r[~keep, 0] == 1) and np.all(r[~keep, 1] == 0)
    # the same with stars that are skipped (status 2) in the device form: an index out of range, a NaN scale, a shift
    # outside the domain, an origin beyond 2^30
    bad = np.flatnonzero(~keep)
    t['origin'][bad] = t['origin'][bad - 1]                        # on the frame, were they valid
    t['index'][bad[0::4]] = 4
    t['scale'][bad[1::4]] = np.nan
    t['shift'][bad[2::4], 1] = -8.5
    t['origin'][bad[3::4], 0] = 2 ** 30 + 1
    t['index'][bad[4::8]] = -1
    t['scale'][bad[5::8]] = -np.inf
    t['shift'][bad[6::8], 0] = np.nan
    m, (ny, nx) = keep.size, Y.FRAME
    dev = {k: _to_dev(torch, v) for k, v in t.items()}
    tout = torch.full((ny, nx), -1.0, dtype=torch.float64, device=dev['psf'].device)
    trow = torch.full((m, 4), -1.0, dtype=torch.float64, device=dev['psf'].device)
    torch.cuda.synchronize()
    ctx.render_stars_device(ny, nx, m, 4, dev['psf'].data_ptr(), dev['origin'].data_ptr(), dev['scale'].data_ptr(),
                            tout.data_ptr(), image_ptr=dev['image'].data_ptr(), shift_ptr=dev['shift'].data_ptr(),
                            psf_index_ptr=dev['index'].data_ptr(), star_out_ptr=trow.data_ptr())
    ctx.sync()
    r = trow.cpu().numpy()
    assert _same(tout.cpu().numpy(), base) and _same(r[keep], rows)
    assert np.all(r[~keep, 0] == 2) and np.all(r[~keep, 1:] == 0)
    # two stars whose footprints share no pixel trade places
    # (neighbours in the list: no star between them sees its place in the order change)
    o = s['origin'].astype(int)
    i = next(k for k in range(63) if np.max(np.abs(o[k + 1] - o[k])) >= Y.SIDE and rows[k, 1] > 0 and rows[k + 1, 1] > 0)
    j = i + 1
    perm = np.arange(n)
    perm[[i, j]] = [j, i]
    sw = dict(s, origin=s['origin'][perm], shift=s['shift'][perm], scale=s['scale'][perm], index=s['index'][perm])
    assert _same(_render(ctx, sw), base)
    # one model stamp per star, copied, instead of the shared four
    got = ctx.render_stars(s['psf'][s['index']], s['origin'], s['scale'], shift=s['shift'], image=s['image'])
    assert _same(got, base)


@pytest.mark.parametrize('prec', PRECS)
def test_a_nan_in_a_model_stays_inside_that_stars_footprint(ctx, prec):
    s = Y.scene()
    base, _ = _base(ctx, prec)
    psf = np.concatenate([s['psf'], s['psf'][:1]])
    psf[4, 20, 20] = np.nan
    index = s['index'].copy()
    k = next(k for k in range(64) if _base(ctx, prec)[1][k, 1] == Y.SIDE ** 2)      # a star wholly on the frame
    index[k] = 4
    got = ctx.render_stars(psf, s['origin'], s['scale'], shift=s['shift'], psf_index=index, image=s['image'])
    y0, y1, x0, x1 = Y.footprint(Y.FRAME, s['origin'][k])
    inside = np.zeros(Y.FRAME, dtype=bool)
    inside[y0:y1, x0:x1] = True
    assert _same(got[~inside], base[~inside])
    assert np.isnan(got[inside]).sum() > np.isnan(base[inside]).sum()


# ---- 4. cut
@pytest.mark.parametrize('prec', PRECS)
def test_cut_is_numpy_slicing_bit_for_bit(ctx, prec):
    import torch
    rng = np.random.default_rng(4)
    ny, nx = 97, 150
    image = rng.normal(size=(ny, nx))
    image[rng.uniform(size=image.shape) < 0.01] = np.nan
    image[3, 4], image[5, 6] = np.inf, -0.0
    var = rng.uniform(-0.1, 2.0, (ny, nx))
    origin = np.array([[0, 0], [-39, -39], [ny - 1, nx - 1], [-40, 10], [10, nx], [30, 60], [57, 110], [-17, 133],
                       [5000, 5000], [-(2 ** 30), 2 ** 30], [2 ** 30, -(2 ** 30)], [2 ** 30, 20], [20, -(2 ** 30)]],
                      dtype=np.int32)
    want, vwant = Y.cut(image, var, origin)
    assert np.isfinite(want[1]).sum() <= 1 and np.isfinite(want[2]).sum() <= 1 and np.all(np.isnan(want[8:]))
    got, vgot = ctx.cut_stamps(image, origin, var=var)
    assert _same(got, want) and _same(vgot, vwant)
    assert np.all(np.isnan(got[3])) and np.all(vgot[3] == 0) and np.all(np.isnan(got[4]))
    assert _same(ctx.cut_stamps(image, origin), want)
    # the device form
    tim, tva, tor = _to_dev(torch, image), _to_dev(torch, var), _to_dev(torch, origin)
    ts = torch.full((len(origin), NS, NS), -1.0, dtype=torch.float64, device=tim.device)
    tv = torch.full((len(origin), NS, NS), -1.0, dtype=torch.float64, device=tim.device)
    torch.cuda.synchronize()
    ctx.cut_stamps_device(ny, nx, tim.data_ptr(), len(origin), tor.data_ptr(), ts.data_ptr(), var_ptr=tva.data_ptr(),
                          var_stamps_ptr=tv.data_ptr())
    ctx.sync()
    assert _same(ts.cpu().numpy(), want) and _same(tv.cpu().numpy(), vwant)
    # a stamp wholly off the frame: the fits answer status 2
    fit = ctx.fit_stamps_psf(got[[5, 8]], Y.models()[:2])
    assert fit[1, 10] == 2


# ---- 5. the loop
def _field():
    """12 well-separated stars and three pairs 5 px apart on a 230 x 300 frame: (psf, positions of the 12, positions of
    the pairs (3, 2, 2), fluxes likewise)."""
    rng = np.random.default_rng(12)
    psf = Y.models()
    grid = np.array([(40 + 50 * i, 40 + 55 * j) for i in range(3) for j in range(4)], dtype=float)
    singles = grid + rng.uniform(-3, 3, grid.shape)
    pc = np.array([(205.3, 60.8), (204.1, 150.2), (206.6, 240.5)])
    ang = rng.uniform(0, np.pi, 3)
    half = 2.5 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    pairs = np.stack([pc - half, pc + half], axis=1)
    return psf, singles, pairs, rng.uniform(100, 1000, 12), rng.uniform(100, 1000, (3, 2))


def _truth_frame(ctx):
    psf, singles, pairs, fs, fp = _field()
    pos = np.concatenate([singles, pairs.reshape(-1, 2)])
    origin = (np.rint(pos) - NS // 2).astype(np.int32)
    shift = pos - np.rint(pos)
    index = (np.arange(len(pos)) % 4).astype(np.int32)
    index[12:] = np.repeat(index[12::2], 2)                        # the stars of a pair share their model
    frame = ctx.render_stars(psf, origin, np.concatenate([fs, fp.ravel()]), shift=shift, psf_index=index,
                             shape=(230, 300))
    return frame, psf, pos, index


@pytest.mark.parametrize('prec', PRECS)
def test_frame_cut_fit_subtract_on_host_and_device(api, ctx, prec):
    import torch
    frame, psf, pos, index = _truth_frame(ctx)
    peak = frame.max()
    assert peak > 10
    # singles: stamps at their rounded positions; pairs: one stamp at the rounded midpoint
    o1 = (np.rint(pos[:12]) - NS // 2).astype(np.int32)
    mid = 0.5 * (pos[12::2] + pos[13::2])
    o2 = (np.rint(mid) - NS // 2).astype(np.int32)
    centre = o2 + NS // 2
    start = np.stack([pos[12::2] - centre, pos[13::2] - centre], axis=1) + 0.2          # (3, 2, 2): off by 0.2 px
    i1, i2 = index[:12], index[12::2]
    st1, st2 = ctx.cut_stamps(frame, o1), ctx.cut_stamps(frame, o2)
    f1 = ctx.fit_stamps_psf(st1, psf, psf_index=i1, background=False)
    # (the stars of the neighbouring stamps are far away: 50 px; the pairs are fitted after the singles are gone)
    res1 = ctx.render_stars(psf, o1, f1[:, 0], shift=f1[:, 1:3], psf_index=i1, image=frame, subtract=True)
    st2 = ctx.cut_stamps(res1, o2)
    f2 = ctx.fit_groups_psf(st2, psf, start, psf_index=i2, background=False)
    assert np.all(f1[:, 10] == 0) and np.all(f2[:, 4] == 0)
    src = f2[:, 8:24].reshape(3, 2, 8)
    res, rows = ctx.render_stars(psf, np.repeat(o2, 2, axis=0), src[:, :, 0].ravel(), shift=src[:, :, 1:3].reshape(6, 2),
                                 psf_index=np.repeat(i2, 2), image=res1, subtract=True, return_status=True)
    assert np.all(rows[:, 0] == 0)
    worst = float(np.max(np.abs(res)) / peak)
    print('loop %s: residual %.2e of the brightest pixel' % (prec, worst))
    record_margin('render', **{'loop_%s' % prec: worst / TOL[prec]})
    assert worst <= TOL[prec]
    # the same chain on device pointers, one context, no sync in between
    dev = torch.device('cuda:0')
    tfr, tps = _to_dev(torch, frame), _to_dev(torch, psf)
    to1, to2, ti1, ti2 = _to_dev(torch, o1), _to_dev(torch, o2), _to_dev(torch, i1), _to_dev(torch, i2)
    tstart = _to_dev(torch, start)
    to22, ti22 = _to_dev(torch, np.repeat(o2, 2, axis=0)), _to_dev(torch, np.repeat(i2, 2))
    ts1 = torch.empty((12, NS, NS), dtype=torch.float64, device=dev)
    ts2 = torch.empty((3, NS, NS), dtype=torch.float64, device=dev)
    tf1 = torch.empty((12, api.NFIT_PSF), dtype=torch.float64, device=dev)
    tf2 = torch.empty((3, api.NFIT_GROUP), dtype=torch.float64, device=dev)
    tres = torch.empty_like(tfr)
    trow = torch.empty((6, 4), dtype=torch.float64, device=dev)
    # the fit rows hold scale and shift side by side; the renderer takes them as arrays of their own
    tsc1, tsh1 = torch.empty(12, dtype=torch.float64, device=dev), torch.empty((12, 2), dtype=torch.float64, device=dev)
    tsc2, tsh2 = torch.empty(6, dtype=torch.float64, device=dev), torch.empty((6, 2), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ext = torch.cuda.ExternalStream(ctx.stream_handle())
    ny, nx = frame.shape
    ctx.cut_stamps_device(ny, nx, tfr.data_ptr(), 12, to1.data_ptr(), ts1.data_ptr())
    ctx.fit_stamps_psf_device(12, ts1.data_ptr(), 4, tps.data_ptr(), tf1.data_ptr(), psf_index_ptr=ti1.data_ptr(),
                              background=False)
    with torch.cuda.stream(ext):                                   # (gathers on the context's own stream: no sync)
        tsc1.copy_(tf1[:, 0])
        tsh1.copy_(tf1[:, 1:3])
    ctx.render_stars_device(ny, nx, 12, 4, tps.data_ptr(), to1.data_ptr(), tsc1.data_ptr(), tres.data_ptr(),
                            image_ptr=tfr.data_ptr(), shift_ptr=tsh1.data_ptr(), psf_index_ptr=ti1.data_ptr(),
                            subtract=True)
    ctx.cut_stamps_device(ny, nx, tres.data_ptr(), 3, to2.data_ptr(), ts2.data_ptr())
    ctx.fit_groups_psf_device(3, 2, ts2.data_ptr(), 4, tps.data_ptr(), tstart.data_ptr(), tf2.data_ptr(),
                              psf_index_ptr=ti2.data_ptr(), background=False)
    with torch.cuda.stream(ext):
        g = tf2[:, 8:24].reshape(3, 2, 8)
        tsc2.copy_(g[:, :, 0].reshape(6))
        tsh2.copy_(g[:, :, 1:3].reshape(6, 2))
    ctx.render_stars_device(ny, nx, 6, 4, tps.data_ptr(), to22.data_ptr(), tsc2.data_ptr(), tres.data_ptr(),
                            image_ptr=tres.data_ptr(), shift_ptr=tsh2.data_ptr(), psf_index_ptr=ti22.data_ptr(),
                            star_out_ptr=trow.data_ptr(), subtract=True)
    ctx.sync()
    assert _same(tf1.cpu().numpy(), f1) and _same(tf2.cpu().numpy(), f2)
    assert _same(tres.cpu().numpy(), res) and _same(trow.cpu().numpy(), rows)


@pytest.mark.parametrize('prec', PRECS)
def test_psfrec_wrappers_are_the_context_methods(api, ctx, prec):
    frame, psf, pos, index = _truth_frame(ctx)
    c02 = api.psfrec.get_context(128, 0.2, 40, prec, 0)
    st, vs, origin = api.cut_star_stamps(frame, pos[:12], precision=prec)
    assert vs is None and np.array_equal(origin, (np.rint(pos[:12]) - 20).astype(np.int32))
    assert _same(st, c02.cut_stamps(frame, origin))
    var = np.full(frame.shape, 0.25)
    st2, vs2, _ = api.cut_star_stamps(frame, pos[:12], var=var, precision=prec)
    assert _same(st2, st) and np.all(vs2 == 0.25)
    table = api.fit_stars_with_psf(st, psf, psf_index=index[:12], fit_back=False, pixscale=0.2, precision=prec)
    keep = np.zeros(12, dtype=bool)
    keep[3] = True
    res, status = api.subtract_stars(frame, psf, origin, table, psf_index=index[:12], pixscale=0.2, keep=keep,
                                     precision=prec)
    rows = np.flatnonzero(~keep)
    sc, sh = np.asarray(table['scale']), np.asarray(table['shift']) / 0.2
    want = c02.render_stars(psf, origin[rows], sc[rows], shift=sh[rows], psf_index=index[:12][rows], image=frame,
                            subtract=True)
    assert _same(res, want) and list(status) == [0, 0, 0, -1] + [0] * 8
    y, x = origin[3] + 20
    assert res[y, x] > 0.5 * frame[y, x] and abs(res[origin[2, 0] + 20, origin[2, 1] + 20]) <= TOL[prec] * frame.max()
    # the pairs: a group table, subtracted from the frame the singles have left
    mid = 0.5 * (pos[12::2] + pos[13::2])
    stg, _, og = api.cut_star_stamps(frame, mid, precision=prec)
    rel = np.stack([pos[12::2], pos[13::2]], axis=1) - (og + 20)[:, None, :]
    gt = api.fit_star_groups_with_psf(stg, psf, rel * 0.2, psf_index=index[12::2], fit_back=False, pixscale=0.2,
                                      precision=prec)
    assert list(np.asarray(gt['group'])) == [0, 0, 1, 1, 2, 2]
    resg, stat = api.subtract_stars(frame, psf, og, gt, psf_index=index[12::2], pixscale=0.2, precision=prec)
    assert list(stat) == [0] * 6
    assert np.max(np.abs(resg[180:])) <= TOL[prec] * frame.max()
    # render_star_field: arcsec in, the same frame as the context method
    field, fstat = api.render_star_field(frame.shape, psf, origin, sc, shift=np.asarray(table['shift']),
                                         psf_index=index[:12], pixscale=0.2, return_status=True, precision=prec)
    assert _same(field, c02.render_stars(psf, origin, sc, shift=sh, psf_index=index[:12], shape=frame.shape))
    assert list(fstat) == [0] * 12


@pytest.mark.parametrize('prec', PRECS)
def test_reconstructed_field_psfs_rendered_from_device_memory(api, prec):
    import torch
    ps = api.grid_pixscale(128)
    lb, see, gl, l0, three = np.array([700.0]), np.array([0.9]), np.array([0.6]), np.array([22.0]), np.array([0])
    pos = np.array([[0.0, 0.0], [-20.0, 40.0]])
    ctx = api.Context(dim=128, pixscale=ps, precision=prec)
    ref = ctx.reconstruct_field(lb, see, gl, l0, three, H, pos)
    models = ref['psf'].reshape(2, NS, NS)
    origin = np.array([[3, 5], [30, 41]], dtype=np.int32)
    scale, shift = np.array([500.0, 800.0]), np.array([[0.3, -0.4], [-1.6, 2.2]])
    dev = torch.device('cuda:0')
    tp = torch.empty(ref['psf'].shape, dtype=torch.float64, device=dev)
    tsum = torch.empty(ref['psf_sum'].shape, dtype=torch.float64, device=dev)
    tfit = torch.empty(ref['fit'].shape, dtype=torch.float64, device=dev)
    tor, tsc, tsh = _to_dev(torch, origin), _to_dev(torch, scale), _to_dev(torch, shift)
    tout = torch.empty((90, 100), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.reconstruct_field_device(lb, see, gl, l0, three, H, 12.0, pos, None, tp.data_ptr(), tsum.data_ptr(),
                                 tfit.data_ptr())
    ctx.render_stars_device(90, 100, 2, 2, tp.data_ptr(), tor.data_ptr(), tsc.data_ptr(), tout.data_ptr(),
                            shift_ptr=tsh.data_ptr())
    ctx.sync()
    want = ctx.render_stars(models, origin, scale, shift=shift, shape=(90, 100))
    assert _same(tout.cpu().numpy(), want)
    ref_frame, _, S = Y.render(None, models, None, origin, shift, scale, shape=(90, 100))
    assert np.max(np.abs(want - ref_frame) / np.where(S > 0, S, 1.0)) <= PARITY
    ctx.close()


# ---- 6. refusals
def test_bad_arguments_are_refused_and_leave_the_outputs(api):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    vp = C.c_void_p
    P = Y.models()
    image = np.random.default_rng(6).normal(size=(50, 70))
    var = np.ones((50, 70))
    origin = np.array([[0, 0], [20, 30]], dtype=np.int32)
    scale, shift, index = np.array([3.0, 2.0]), np.zeros((2, 2)), np.array([0, 3], dtype=np.int32)
    out, rows = np.full((50, 70), -7.0), np.full((2, 4), -7.0)
    stamps, vstamps = np.full((2, NS, NS), -7.0), np.full((2, NS, NS), -7.0)

    def ptr(a):
        return None if a is None else vp(a.ctypes.data)

    def cut(ny=50, nx=70, image=image, var=None, nstar=2, origin=origin, stamps=stamps, var_out=None):
        return ctx.lib.mpsfr_cut_stamps(ctx._h, ny, nx, ptr(image), ptr(var), nstar, ptr(origin), ptr(stamps),
                                        ptr(var_out), 0)

    def render(ny=50, nx=70, image=image, nstar=2, npsf=4, psf=P, index=index, origin=origin, shift=shift, scale=scale,
               flags=0, out=out, rows=rows):
        return ctx.lib.mpsfr_render_stars(ctx._h, ny, nx, ptr(image), nstar, npsf, ptr(psf), ptr(index), ptr(origin),
                                          ptr(shift), ptr(scale), flags, ptr(out), ptr(rows), 0)

    frames = (dict(ny=0), dict(nx=0), dict(ny=-1), dict(ny=16385), dict(nx=16385), dict(ny=8193, nx=8192))
    for kw in frames + (dict(nstar=0), dict(image=None), dict(origin=None), dict(stamps=None), dict(var=var),
                        dict(var_out=vstamps)):
        assert cut(**kw) == -1, kw
        assert np.all(stamps == -7.0) and np.all(vstamps == -7.0), kw
    bad_values = (dict(index=np.array([0, 4], dtype=np.int32)), dict(index=np.array([-1, 0], dtype=np.int32)),
                  dict(shift=np.array([[0.0, np.nan], [0.0, 0.0]])), dict(shift=np.array([[0.0, 0.0], [8.5, 0.0]])),
                  dict(scale=np.array([1.0, np.inf])), dict(scale=np.array([np.nan, 1.0])),
                  dict(origin=np.array([[0, 2 ** 30 + 1], [0, 0]], dtype=np.int32)),
                  dict(origin=np.array([[0, 0], [-(2 ** 31), 0]], dtype=np.int32)))
    for kw in frames + (dict(nstar=0), dict(npsf=0), dict(psf=None), dict(origin=None), dict(scale=None), dict(out=None),
                        dict(flags=2), dict(flags=-1), dict(flags=3), dict(flags=1, image=None),
                        dict(index=None)) + bad_values:                     # (no index, npsf != nstar)
        assert render(**kw) == -1, kw
        assert np.all(out == -7.0) and np.all(rows == -7.0), kw
    for kw in (dict(), dict(var=var, var_out=vstamps)):
        assert cut(**kw) == 0, kw
    assert np.array_equal(stamps[0], image[:NS, :NS]) and np.all(vstamps[1, :30] == 1.0) and np.all(vstamps[1, 30:] == 0)
    for kw in (dict(), dict(image=None), dict(flags=1), dict(shift=None, rows=None), dict(index=None, npsf=2),
               dict(scale=np.zeros(2))):
        out[:] = -7.0
        assert render(**kw) == 0, kw
        assert not np.any(out == -7.0), kw
    assert np.all(rows[:, 0] == 0) and _same(out, image)               # scale 0 is rendered: image + 0
    # the same bad values in the device form: status 2 on that row, the neighbour as if alone
    import torch
    tim, tps = _to_dev(torch, image), _to_dev(torch, P)
    for kw in bad_values:
        a = dict(index=index, shift=shift, scale=scale, origin=origin)
        a.update(kw)
        t = {k: _to_dev(torch, v) for k, v in a.items()}
        tout = torch.full((50, 70), -7.0, dtype=torch.float64, device=tim.device)
        trow = torch.full((2, 4), -7.0, dtype=torch.float64, device=tim.device)
        torch.cuda.synchronize()
        ctx.render_stars_device(50, 70, 2, 4, tps.data_ptr(), t['origin'].data_ptr(), t['scale'].data_ptr(),
                                tout.data_ptr(), image_ptr=tim.data_ptr(), shift_ptr=t['shift'].data_ptr(),
                                psf_index_ptr=t['index'].data_ptr(), star_out_ptr=trow.data_ptr())
        ctx.sync()
        r = trow.cpu().numpy()
        good = int(np.flatnonzero(r[:, 0] == 0)[0])
        assert sorted(r[:, 0]) == [0, 2] and r[1 - good, 1] == 0, (kw, r)
        g = slice(good, good + 1)
        alone = ctx.render_stars(P, a['origin'][g], a['scale'][g], shift=a['shift'][g], psf_index=a['index'][g], image=image)
        assert _same(tout.cpu().numpy(), alone), kw
    ctx.close()


# ---- 7. profiling
def test_timed_under_the_profiling_id_of_the_fit(api):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    s = Y.scene()
    ctx.set_option('profile', 1)
    ctx.profile_reset()
    _render(ctx, s)
    prof = ctx.profile()
    assert prof['fit'][1] == 1 and prof['fit'][0] > 0
    ctx.cut_stamps(s['image'], s['origin'][:8])
    prof = ctx.profile()
    assert prof['fit'][1] == 2
    assert all(v[1] == 0 for k, v in prof.items() if k != 'fit'), prof
    ctx.close()
