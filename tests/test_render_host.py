"""Host: the frame calls (mpsfr_cut_stamps, mpsfr_render_stars) without a GPU.

1. the yardstick (render_ref): its window on the 40 x 40 stamp is the model of the PSF fit; a split star list gives the
   same bits; the shared scene holds what the GPU test needs.
2. what the new Context methods hand to C, argument by argument, against a stub library that records each call (the
   prototypes of include/mpsfr.h written out by hand), NULLs and on_device included.
3. the ValueErrors of the wrappers.
4. the row selection of subtract_stars: status-2 rows, keep, group tables.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import psf_fit_ref as R
import render_ref as Y
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec
from muse_psfr_amd._lib import NRENDER, Context

NS = 40
HANDLE = 0xBEE0
_rng = np.random.default_rng(21)
IMAGE = _rng.normal(size=(23, 31))
VAR = _rng.uniform(0.5, 1.5, (23, 31))
PSF = Y.models()[:3]
ORIGIN = np.array([[-5, 3], [10, -12], [2, 7], [100, 100], [0, 0]])
SCALE = np.array([3.0, -2.0, 0.0, 10.0, 7.5])
SHIFT = np.array([[0.5, -0.25], [8.0, -8.0], [0.0, 0.0], [1.0, 2.0], [-3.5, 3.5]])
INDEX = np.array([0, 2, 1, 1, 0])
DEV = dict(image=0x1000, var=0x2000, origin=0x3000, stamps=0x4000, vstamps=0x5000, psf=0x6000, scale=0x7000,
           shift=0x8000, index=0x9000, out=0xA000, rows=0xB000)


# ---- 1. the yardstick
def test_window_on_the_stamp_is_the_model_of_the_fit():
    rng = np.random.default_rng(3)
    for P in Y.models():
        for _ in range(6):
            F, dp, dq = rng.uniform(-1000, 1000), *rng.uniform(-8, 8, 2)
            w = F * Y.window(P, dp, dq)[Y.APRON:Y.APRON + NS, Y.APRON:Y.APRON + NS]
            assert np.max(np.abs(w - R.model(P, (F, dp, dq, 0.0)))) <= 1e-15 * abs(F) * P.max()
    # zero shift: the window is the stamp itself, zero around it; whole-pixel shifts displace it
    P = Y.models()[1]
    w = Y.window(P, 0.0, 0.0)
    assert np.array_equal(w[10:50, 10:50], P) and w.sum() == P.sum()
    assert np.array_equal(Y.window(P, 2.0, -3.0)[12:52, 7:47], P)
    assert np.array_equal(Y.window(P, -8.0, 8.0)[2:42, 18:58], P)


def test_split_star_list_gives_the_same_bits():
    s = Y.scene()
    full = Y.scene_reference(False)[0]
    for m in (1, 17, 63, 64 + 150):
        a = Y.render(s['image'], s['psf'], s['index'][:m], s['origin'][:m], s['shift'][:m], s['scale'][:m])[0]
        b = Y.render(a, s['psf'], s['index'][m:], s['origin'][m:], s['shift'][m:], s['scale'][m:])[0]
        assert np.array_equal(b, full, equal_nan=True), m


def test_scene_holds_what_the_gpu_test_needs():
    s = Y.scene()
    out, npix, S = Y.scene_reference(False)
    assert s['n'] == 64 + Y.PILE and Y.PILE > _lib.RENDER_SORT_CHUNK
    assert Y.longest_tile_list(s) > _lib.RENDER_SORT_CHUNK
    assert list(npix[s['off_frame']]) == [0, 0, 0] and np.count_nonzero(npix == 0) == 3
    assert np.array_equal(np.isnan(out), np.isnan(s['image'])) and np.isnan(out).sum() > 50
    assert len(np.unique(s['index'][:64])) == 4 and s['scale'].min() < 0 < s['scale'].max()
    assert np.abs(s['shift']).max() > 7.9 and np.abs(s['shift']).max() <= 8.0


def test_constants_match_the_header_and_the_kernels():
    hdr = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    for name, val in (('RENDER_SUBTRACT', _lib.RENDER_SUBTRACT), ('NRENDER', _lib.NRENDER),
                      ('MAX_IMAGE_SIDE', _lib.MAX_IMAGE_SIDE), ('RENDER_SORT_CHUNK', _lib.RENDER_SORT_CHUNK)):
        assert int(re.search(r'#define MPSFR_%s\s+(\d+)' % name, hdr).group(1)) == val, name
    src = open(os.path.join(ROOT, 'muse_psfr_amd', 'csrc', 'render.hip')).read()
    assert int(re.search(r'constexpr int kSortChunk = (\d+);', src).group(1)) == _lib.RENDER_SORT_CHUNK
    assert int(re.search(r'constexpr int kTile = (\d+);', src).group(1)) == Y.TILE
    com = open(os.path.join(ROOT, 'muse_psfr_amd', 'csrc', 'fit_psf_common.h')).read()
    assert int(re.search(r'constexpr int kPsfApron = (\d+);', com).group(1)) == Y.APRON == _lib.RENDER_APRON


# ---- 2. what reaches C
class StubLib:
    """Every attribute is a C function that records (name, args) and returns 0; mpsfr_render_stars also clears its
    star_out, as a run that renders every star would."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == 'mpsfr_render_stars' and args[14] == 0 and args[13] is not None:
                C.memset(args[13], 0, 8 * NRENDER * args[4])
            return 0
        return fn


def make_ctx():
    ctx = Context.__new__(Context)
    ctx.lib = StubLib()
    ctx.dim, ctx.pixscale, ctx.dimpsf, ctx.precision = 128, 0.2, NS, 'mixed'
    ctx._h = C.c_void_p(HANDLE)
    ctx._pending, ctx._abandoned = {}, set()
    return ctx


@pytest.fixture
def ctx():
    c = make_ctx()
    yield c
    c._h = None            # (nothing to destroy)


_CT = {np.dtype(np.float64): C.c_double, np.dtype(np.int32): C.c_int32}
NULL = ('null',)


def I(v):
    return ('int', v)


def A(a, dtype=np.float64):
    """A host array: a void* to these values of this element type."""
    return ('array', np.asarray(a, dtype=dtype))


def OUT(a):
    return ('out', a)


def DEVP(addr):
    return ('dev', addr)


def expect(lib, name, items):
    assert len(lib.calls) == 1
    got, args = lib.calls[0]
    assert got == name and len(args) == len(items) + 1, (got, len(args))
    assert isinstance(args[0], C.c_void_p) and args[0].value == HANDLE
    for k, (arg, item) in enumerate(zip(args[1:], items)):
        kind, where = item[0], (name, k + 1, item[0])
        if kind == 'int':
            assert isinstance(arg, (int, np.integer)) and not isinstance(arg, bool) and arg == item[1], where + (arg,)
        elif kind == 'null':
            assert arg is None, where + (arg,)
        elif kind == 'dev':
            assert isinstance(arg, C.c_void_p) and arg.value == item[1], where + (arg,)
        elif kind == 'out':
            assert isinstance(arg, C.c_void_p) and arg.value == item[1].ctypes.data, where
            assert item[1].dtype == np.float64 and item[1].flags.c_contiguous, where
        else:
            want = item[1]
            assert isinstance(arg, C.c_void_p) and arg.value, where
            held = getattr(arg, '_arr', None)       # (numpy's data_as keeps the array: its own dtype and size)
            if held is not None:
                assert held.dtype == want.dtype and held.size == want.size and held.flags.c_contiguous, where
            buf = (_CT[want.dtype] * int(want.size)).from_address(arg.value)
            np.testing.assert_array_equal(np.frombuffer(buf, dtype=want.dtype).reshape(want.shape), want, err_msg=str(where))


# mpsfr_cut_stamps(ctx, ny, nx, image, var, nstar, origin, stamps_out, var_out, on_device)
def test_cut_stamps_host(ctx):
    st = ctx.cut_stamps(IMAGE, ORIGIN)
    assert st.shape == (5, NS, NS) and st.dtype == np.float64
    expect(ctx.lib, 'mpsfr_cut_stamps', [I(23), I(31), A(IMAGE), NULL, I(5), A(ORIGIN, np.int32), OUT(st), NULL, I(0)])


def test_cut_stamps_host_with_var_and_a_masked_image(ctx):
    masked = np.ma.masked_array(IMAGE, mask=IMAGE > 1.5)
    st, vs = ctx.cut_stamps(masked, ORIGIN.astype(np.int16), var=VAR.astype(np.float32))
    assert st.shape == vs.shape == (5, NS, NS)
    expect(ctx.lib, 'mpsfr_cut_stamps', [I(23), I(31), A(np.where(IMAGE > 1.5, np.nan, IMAGE)),
                                         A(VAR.astype(np.float32)), I(5), A(ORIGIN, np.int32), OUT(st), OUT(vs), I(0)])


def test_cut_stamps_device(ctx):
    assert ctx.cut_stamps_device(23, 31, DEV['image'], 5, DEV['origin'], DEV['stamps']) is None
    expect(ctx.lib, 'mpsfr_cut_stamps', [I(23), I(31), DEVP(DEV['image']), NULL, I(5), DEVP(DEV['origin']),
                                         DEVP(DEV['stamps']), NULL, I(1)])
    ctx.lib.calls.clear()
    ctx.cut_stamps_device(23, 31, DEV['image'], 5, DEV['origin'], DEV['stamps'], var_ptr=DEV['var'],
                          var_stamps_ptr=DEV['vstamps'])
    expect(ctx.lib, 'mpsfr_cut_stamps', [I(23), I(31), DEVP(DEV['image']), DEVP(DEV['var']), I(5), DEVP(DEV['origin']),
                                         DEVP(DEV['stamps']), DEVP(DEV['vstamps']), I(1)])


# mpsfr_render_stars(ctx, ny, nx, image_in, nstar, npsf, psf, psf_index, origin, shift, scale, flags, image_out, star_out,
#                    on_device)
def test_render_stars_host_minimal(ctx):
    out = ctx.render_stars(np.concatenate([PSF, PSF[:2]]), ORIGIN, SCALE, shape=(23, 31))
    assert out.shape == (23, 31) and out.dtype == np.float64
    expect(ctx.lib, 'mpsfr_render_stars', [I(23), I(31), NULL, I(5), I(5), A(np.concatenate([PSF, PSF[:2]])), NULL,
                                           A(ORIGIN, np.int32), NULL, A(SCALE), I(0), OUT(out), NULL, I(0)])


def test_render_stars_host_everything(ctx):
    out, rows = ctx.render_stars(PSF, ORIGIN, list(SCALE), shift=SHIFT, psf_index=INDEX, image=IMAGE, shape=(23, 31),
                                 subtract=True, return_status=True)
    assert out.shape == (23, 31) and rows.shape == (5, NRENDER) and out is not IMAGE
    expect(ctx.lib, 'mpsfr_render_stars', [I(23), I(31), A(IMAGE), I(5), I(3), A(PSF), A(INDEX, np.int32),
                                           A(ORIGIN, np.int32), A(SHIFT), A(SCALE), I(1), OUT(out), OUT(rows), I(0)])


def test_render_stars_device(ctx):
    assert ctx.render_stars_device(23, 31, 5, 5, DEV['psf'], DEV['origin'], DEV['scale'], DEV['out']) is None
    expect(ctx.lib, 'mpsfr_render_stars', [I(23), I(31), NULL, I(5), I(5), DEVP(DEV['psf']), NULL, DEVP(DEV['origin']),
                                           NULL, DEVP(DEV['scale']), I(0), DEVP(DEV['out']), NULL, I(1)])
    ctx.lib.calls.clear()
    ctx.render_stars_device(23, 31, 5, 3, DEV['psf'], DEV['origin'], DEV['scale'], DEV['image'], image_ptr=DEV['image'],
                            shift_ptr=DEV['shift'], psf_index_ptr=DEV['index'], star_out_ptr=DEV['rows'], subtract=True)
    expect(ctx.lib, 'mpsfr_render_stars', [I(23), I(31), DEVP(DEV['image']), I(5), I(3), DEVP(DEV['psf']),
                                           DEVP(DEV['index']), DEVP(DEV['origin']), DEVP(DEV['shift']),
                                           DEVP(DEV['scale']), I(1), DEVP(DEV['image']), DEVP(DEV['rows']), I(1)])


# ---- 3. the ValueErrors
def test_cut_stamps_refuses(ctx):
    bad = [dict(image=IMAGE[0]), dict(image=IMAGE[None]), dict(image=np.zeros((0, 4))), dict(image='frame'),
           dict(image=np.zeros((1, 16385))), dict(origin=ORIGIN[:, 0]), dict(origin=ORIGIN.astype(float)),
           dict(origin=np.zeros((0, 2), int)), dict(origin=[[0, 2 ** 30 + 1]]), dict(origin=[[-2 ** 31, 0]]),
           dict(var=VAR[:-1]), dict(var=VAR.T), dict(var='v')]
    for kw in bad:
        args = dict(image=IMAGE, origin=ORIGIN, var=None)
        args.update(kw)
        with pytest.raises(ValueError):
            ctx.cut_stamps(args['image'], args['origin'], var=args['var'])
    for a in [(0, 31, 1, 5, 1, 1), (23, 16385, 1, 5, 1, 1), (8193, 8193, 1, 5, 1, 1), (23, 31, 0, 5, 1, 1),
              (23, 31, 1, 0, 1, 1), (23, 31, 1, 5, 0, 1), (23, 31, 1, 5, 1, 0), (23.0, 31, 1, 5, 1, 1)]:
        with pytest.raises(ValueError):
            ctx.cut_stamps_device(*a)
    with pytest.raises(ValueError):
        ctx.cut_stamps_device(23, 31, 1, 5, 1, 1, var_ptr=1)
    with pytest.raises(ValueError):
        ctx.cut_stamps_device(23, 31, 1, 5, 1, 1, var_stamps_ptr=1)
    assert ctx.lib.calls == []
    ctx.cut_stamps(np.zeros((1, 16384)), [[2 ** 30, -2 ** 30]])            # the bounds themselves are legal
    assert len(ctx.lib.calls) == 1


def test_render_stars_refuses(ctx):
    base = dict(psf=PSF, origin=ORIGIN, scale=SCALE, shift=SHIFT, psf_index=INDEX, image=IMAGE, shape=None,
                subtract=False, return_status=False)
    bad = [dict(psf=PSF[:, :39]), dict(psf='p'), dict(psf_index=None),              # 3 model stamps for 5 stars
           dict(psf_index=[0, 1, 2, 3, 0]), dict(psf_index=[0, 1, -1, 2, 0]), dict(psf_index=INDEX[:4]),
           dict(psf_index=INDEX.astype(float)), dict(origin=ORIGIN[:4]), dict(origin=ORIGIN + 0.5),
           dict(scale=SCALE[:4]), dict(scale=np.where(SCALE == 0, np.nan, SCALE)), dict(scale=np.full(5, np.inf)),
           dict(scale='s'), dict(scale=SCALE[None].T), dict(shift=SHIFT[:4]), dict(shift=SHIFT.T),
           dict(shift=SHIFT + 8.0), dict(shift=np.where(SHIFT == 0, np.nan, SHIFT)), dict(image=None),   # nor a shape
           dict(image=None, shape=(23, 31), subtract=True), dict(image=None, shape=(0, 31)), dict(image=None, shape=23),
           dict(image=None, shape=(16385, 2)), dict(shape=(23, 30)), dict(image=IMAGE[0]), dict(subtract=1),
           dict(return_status='yes')]
    for kw in bad:
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError):
            ctx.render_stars(**args)
    for a, kw in [((0, 31, 5, 5, 1, 1, 1, 1), {}), ((23, 31, 0, 5, 1, 1, 1, 1), {}), ((23, 31, 5, 0, 1, 1, 1, 1), {}),
                  ((23, 31, 5, 5, 0, 1, 1, 1), {}), ((23, 31, 5, 5, 1, 0, 1, 1), {}), ((23, 31, 5, 5, 1, 1, 0, 1), {}),
                  ((23, 31, 5, 5, 1, 1, 1, 0), {}), ((23, 31, 5, 3, 1, 1, 1, 1), {}),            # no index, npsf != nstar
                  ((23, 31, 5, 5, 1, 1, 1, 1), dict(subtract=True)), ((23, 31, 5, 5, 1, 1, 1, 1), dict(subtract=2))]:
        with pytest.raises(ValueError):
            ctx.render_stars_device(*a, **kw)
    assert ctx.lib.calls == []


def test_psfrec_wrappers_refuse(monkeypatch):
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: make_ctx())
    for pos in ([1.0, 2.0], [[1.0, np.nan]], [[np.inf, 0.0]], np.zeros((0, 2)), 'p', [[2.0 ** 31, 0.0]]):
        with pytest.raises(ValueError):
            psfrec.cut_star_stamps(IMAGE, pos)
    with pytest.raises(ValueError):
        psfrec.cut_star_stamps(IMAGE, [[3.0, 4.0]], var=VAR[:5])
    with pytest.raises(ValueError):
        psfrec.render_star_field((23, 31), PSF, ORIGIN[:3], SCALE[:3], pixscale=0.0)
    with pytest.raises(ValueError):
        psfrec.render_star_field((23, 31), PSF, ORIGIN[:3], SCALE[:3], shift=SHIFT[:3] * 0.2, pixscale=0.1)   # 16 px
    with pytest.raises(ValueError):
        psfrec.render_star_field(None, PSF, ORIGIN[:3], SCALE[:3])


# ---- 4. the wrappers of psfrec
def _one_ctx(monkeypatch):
    ctx = make_ctx()
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: ctx)
    return ctx


def test_cut_star_stamps_rounds_the_positions(monkeypatch):
    ctx = _one_ctx(monkeypatch)
    pos = np.array([[10.4, 20.6], [0.5, -0.5], [22.49, 1.5], [-3.2, 40.0]])
    st, vs, origin = psfrec.cut_star_stamps(IMAGE, pos)
    want = np.array([[-10, 1], [-20, -20], [2, -18], [-23, 20]])            # rint: halves to even
    assert vs is None and origin.dtype == np.int32 and np.array_equal(origin, want)
    expect(ctx.lib, 'mpsfr_cut_stamps', [I(23), I(31), A(IMAGE), NULL, I(4), A(want, np.int32), OUT(st), NULL, I(0)])
    ctx.lib.calls.clear()
    st, vs, origin = psfrec.cut_star_stamps(IMAGE, pos, var=VAR)
    expect(ctx.lib, 'mpsfr_cut_stamps', [I(23), I(31), A(IMAGE), A(VAR), I(4), A(want, np.int32), OUT(st), OUT(vs), I(0)])


def test_render_star_field_takes_arcsec(monkeypatch):
    ctx = _one_ctx(monkeypatch)
    out, status = psfrec.render_star_field((23, 31), PSF, ORIGIN, SCALE, shift=SHIFT * 0.25, psf_index=INDEX, pixscale=0.25,
                                           return_status=True)
    assert status.shape == (5,) and status.dtype == np.int64 and np.all(status == 0)
    got = ctx.lib.calls[0][1]
    assert got[3] is None and got[11] == 0
    buf = (C.c_double * 10).from_address(got[9].value)
    assert np.array_equal(np.frombuffer(buf).reshape(5, 2), SHIFT)


def _table(**cols):
    return psfrec.Table(cols)


def _render_call(ctx):
    assert len(ctx.lib.calls) == 1 and ctx.lib.calls[0][0] == 'mpsfr_render_stars'
    a = ctx.lib.calls[0][1]
    n = a[4]

    def arr(p, count, ct, dt):
        return np.frombuffer((ct * count).from_address(p.value), dtype=dt).copy()
    return dict(n=n, npsf=a[5], index=arr(a[7], n, C.c_int32, np.int32), origin=arr(a[8], 2 * n, C.c_int32, np.int32).reshape(n, 2),
                shift=arr(a[9], 2 * n, C.c_double, np.float64).reshape(n, 2), scale=arr(a[10], n, C.c_double, np.float64),
                flags=a[11], image=arr(a[3], IMAGE.size, C.c_double, np.float64).reshape(IMAGE.shape))


def test_subtract_stars_selects_the_rows(monkeypatch):
    ctx = _one_ctx(monkeypatch)
    fit = _table(scale=SCALE, shift=SHIFT * 0.2, status=np.array([0, 2, 1, 6, 4]))
    res, status = psfrec.subtract_stars(IMAGE, PSF, ORIGIN, fit, psf_index=INDEX, pixscale=0.2)
    c = _render_call(ctx)
    rows = [0, 2, 4]                                   # status & 3 == 2: rows 1 and 3 stay in the frame
    assert c['n'] == 3 and c['npsf'] == 3 and c['flags'] == _lib.RENDER_SUBTRACT
    assert np.array_equal(c['origin'], ORIGIN[rows]) and np.array_equal(c['index'], INDEX[rows])
    assert np.array_equal(c['scale'], SCALE[rows]) and np.allclose(c['shift'], SHIFT[rows], rtol=0, atol=1e-15)
    assert np.array_equal(c['image'], IMAGE) and res.shape == IMAGE.shape
    assert list(status) == [0, -1, 0, -1, 0]
    # keep: the target stays, the neighbours go; without psf_index star k has model stamp k
    ctx.lib.calls.clear()
    keep = np.array([True, False, False, False, False])
    res, status = psfrec.subtract_stars(IMAGE, np.concatenate([PSF, PSF[:2]]), ORIGIN, fit, keep=keep)
    c = _render_call(ctx)
    assert c['n'] == 2 and c['npsf'] == 5 and list(c['index']) == [2, 4] and list(status) == [-1, -1, 0, -1, 0]
    # values that cannot be rendered are skipped like status 2; nothing left: no call, the image comes back
    ctx.lib.calls.clear()
    odd = _table(scale=np.array([np.nan, 1.0, 2.0]), shift=np.array([[0.0, 0.0], [2.0, 0.0], [0.0, np.inf]]),
                 status=np.array([0, 0, 1]))
    res, status = psfrec.subtract_stars(IMAGE, PSF, ORIGIN[:3], odd)
    assert ctx.lib.calls == [] and list(status) == [2, 2, 2] and np.array_equal(res, IMAGE) and res is not IMAGE
    for kw in (dict(keep=[1, 0, 0, 0, 0]), dict(keep=keep[:4]), dict(pixscale=-1.0)):
        with pytest.raises(ValueError):
            psfrec.subtract_stars(IMAGE, PSF, ORIGIN, fit, psf_index=INDEX, **kw)
    with pytest.raises(ValueError):
        psfrec.subtract_stars(IMAGE, PSF, ORIGIN[:4], fit, psf_index=INDEX[:4])        # a row without an origin
    with pytest.raises(ValueError):
        psfrec.subtract_stars(IMAGE, PSF, ORIGIN, _table(scale=SCALE, status=np.zeros(5, int)))


def test_subtract_stars_takes_a_group_table(monkeypatch):
    ctx = _one_ctx(monkeypatch)
    group = np.array([0, 1, 1, 1, 2, 2])               # a single star, a triple, a pair: three stamps
    scale = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    shift = np.array([[0.1, 0.2], [-1.0, 1.0], [0.0, 0.0], [1.5, -1.5], [0.3, 0.3], [-0.3, -0.3]])
    fit = _table(group=group, source=np.array([0, 0, 1, 2, 0, 1]), scale=scale, shift=shift,
                 status=np.array([0, 2, 2, 2, 1, 1]))
    index = np.array([2, 0, 1])
    res, status = psfrec.subtract_stars(IMAGE, PSF, ORIGIN[:3], fit, psf_index=index, pixscale=0.1,
                                        keep=np.array([False, False, False, False, True, False]))
    c = _render_call(ctx)
    assert c['n'] == 2 and np.array_equal(c['origin'], ORIGIN[[0, 2]]) and list(c['index']) == [2, 1]
    assert list(c['scale']) == [1.0, 6.0] and np.allclose(c['shift'], shift[[0, 5]] / 0.1, rtol=0, atol=1e-14)
    assert list(status) == [0, -1, -1, -1, -1, 0]
