"""Host: the star finder (mpsfr_find_stars) without a GPU.

1. the yardstick alone (find_ref): the model on a constant background gives back its scale, the background and
   sharpness 1 within the derived rounding bound; on the shared scene every star and the hot pixel are found and nothing
   else, at three thresholds; the margins that make the GPU's discrete answers unambiguous -- no T within 1e-9 relative of
   the threshold, no candidate within 1e-9 relative of its best rival, every curvature well below zero or flagged.
2. what the new Context methods hand to C, argument by argument, against the recording stub library of
   test_render_host.py, NULLs and on_device included; the exports and the header constants.
3. the ValueErrors of the wrappers, with no library call made.
4. psfrec.find_stars against a stub that answers with rows: sep=None, the second call, the stable descending sort, the
   sharpness bounds, shift = offset x pixscale.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import find_ref as F
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec
from test_render_host import DEV, HANDLE, StubLib, make_ctx

NS = 40
PSF = F.model()
_rng = np.random.default_rng(5)
IMAGE = _rng.normal(size=(23, 31))
VAR = _rng.uniform(0.5, 1.5, (23, 31))
PARITY_SETTINGS = [(usevar, half, sep) for usevar in (True, False) for half in (3, 8) for sep in (1, 3, 16)]


# ---- 1. the yardstick
@pytest.mark.parametrize('half', [1, 3, 8])
@pytest.mark.parametrize('usevar', [False, True])
def test_the_model_on_a_constant_background_gives_back_its_scale(usevar, half):
    rng = np.random.default_rng(half)
    for scale, back in ((250.0, 10.0), (3.5, -2.0), (1e4, 0.0)):
        frame = np.full((70, 64), back)
        frame[12:12 + NS, 9:9 + NS] += scale * PSF
        var = rng.uniform(0.5, 1.5, frame.shape) if usevar else None
        ref = F.find(frame, var, PSF, half, 3, 1e-3 * scale)
        k = int(np.flatnonzero(ref['index'] == 32 * 64 + 29)[0])        # the model's centre: (12 + 20, 9 + 20)
        row, bound = ref['rows'][k], F.row_bounds(ref)[k]
        assert abs(row[3] - scale) <= bound[3] and bound[3] < 1e-9 * scale
        assert abs(row[4] - back) <= bound[4] and bound[4] < 1e-9 * max(abs(back), 1.0)
        assert abs(row[5] - 1.0) <= bound[5] + 4 * F.EPS and bound[5] < 1e-9
        assert row[6] == (2 * half + 1) ** 2 and row[7] == 0
        if not usevar:                                                   # a symmetric model: the top is the pixel
            assert abs(row[0] - 32) < 1e-6 and abs(row[1] - 29) < 1e-6
        assert np.array_equal(ref['origin'][k], [12, 9])


@pytest.mark.parametrize('threshold', [5.0, 8.0, 12.0])
def test_every_scene_star_is_found_and_nothing_else(threshold):
    s = F.scene()
    ref = F.scene_reference(True, 3, 3, threshold)
    rows, truth = ref['rows'], s['truth']
    assert len(truth) == 78 and ref['count'] == len(truth) + 1 == len(rows)
    dist = np.sqrt(((rows[:, None, :2] - truth[None]) ** 2).sum(-1))
    assert dist.min(axis=0).max() < 1.0                                  # every star within 1 px of a peak
    hot = np.all(np.rint(rows[:, :2]) == s['hot'], axis=1)
    assert hot.sum() == 1 and np.all(dist.min(axis=1)[~hot] < 1.0)      # every peak a star or the hot pixel
    assert np.median(dist.min(axis=0)) < 0.1
    assert rows[hot, 5][0] > 3 and np.all((rows[~hot, 5] > 0.5) & (rows[~hot, 5] < 1.5))
    assert rows[:, 2].min() > 25                                         # the weakest star: far above every threshold
    # the amplitude is the flux scale of the model: within 5 sigma_H of the truth (sigma_H = H / T)
    near = dist.argmin(axis=1)
    sigma = rows[:, 3] / rows[:, 2]
    inside = ~hot & (rows[:, 6] == 49) & (dist.min(axis=1) < 0.3)
    assert inside.sum() > 30 and np.all(np.abs(rows[inside, 3] - s['flux'][near[inside]]) < 0.15 * s['flux'][near[inside]])
    assert np.all(sigma > 0)


def test_scene_holds_what_the_gpu_test_needs():
    s = F.scene()
    ref = F.scene_reference()
    Y, X = np.divmod(ref['index'], F.FRAME[1])
    for border in (31, 32, 63, 64):
        assert np.count_nonzero(Y == border) >= 2 and np.count_nonzero(X == border) >= 2, border
    assert np.any((Y == 31) & (X == 32)) and np.any((Y == 64) & (X == 64))
    assert np.any(Y <= 1) and np.any(Y >= F.FRAME[0] - 2) and np.any(X <= 1) and np.any(X >= F.FRAME[1] - 2)
    assert np.any((Y <= 2) & (X <= 2)) and np.any((Y >= F.FRAME[0] - 3) & (X >= F.FRAME[1] - 3))
    assert np.any(s['truth'][:, 0] < -0.5) and Y.min() == 0              # the star centred off the frame, found on row 0
    assert np.isnan(s['image']).sum() > 100
    rows = ref['rows']
    assert set(rows[:, 7]) >= {0.0, 1.0} and np.any(rows[:, 6] < 49)     # flagged parabolas, windows with masked pixels
    assert np.isnan(ref['map']).sum() >= np.isnan(s['image']).sum()


@pytest.mark.parametrize('usevar,half,sep', PARITY_SETTINGS)
def test_margins_that_make_the_discrete_answers_unambiguous(usevar, half, sep):
    """The condition of the GPU parity test, asserted on the reference alone: 1e-9 relative is more than twenty times
    the a-priori rounding bound of T (stat_bounds: up to 2e-11 relative on this scene, whose background of 10 enters the
    sums of the absolute terms)."""
    thr = F.THRESHOLD[usevar]
    ref = F.scene_reference(usevar, half, sep, thr)
    T = ref['map']
    fin = np.isfinite(T)
    dT = F.stat_bounds(ref)[0]
    assert np.all(dT[fin] < 0.05 * 1e-9 * np.maximum(np.abs(T[fin]), thr))
    assert np.all(np.abs(T[fin] - thr) > 1e-9 * np.maximum(np.abs(T[fin]), thr))
    ny, nx = T.shape
    index = np.arange(ny * nx).reshape(ny, nx)
    for i in np.flatnonzero(fin.ravel() & (np.nan_to_num(T.ravel(), nan=-np.inf) >= thr)):
        Y, X = divmod(int(i), nx)
        sl = (slice(max(Y - sep, 0), Y + sep + 1), slice(max(X - sep, 0), X + sep + 1))
        others = np.isfinite(T[sl]) & (index[sl] != i)
        if others.any():
            assert np.min(np.abs(T[sl][others] - T[Y, X])) > 1e-9 * abs(T[Y, X]), (Y, X)
    # the parabolas: a curvature well below zero, or the flag
    for row, i in zip(ref['rows'], ref['index']):
        Y, X = divmod(int(i), nx)
        for bit, tm, tp in ((1, T[Y - 1, X] if Y else np.nan, T[Y + 1, X] if Y + 1 < ny else np.nan),
                            (2, T[Y, X - 1] if X else np.nan, T[Y, X + 1] if X + 1 < nx else np.nan)):
            if not int(row[7]) & bit:
                assert tm - 2 * T[Y, X] + tp < -1e-3 * T[Y, X], (Y, X, bit)
    # the defined / undefined border of the map: den stays away from 0 wherever the window is valid
    den, ok = ref['den'], 2 * ref['nvalid'] > ref['K'].size
    assert np.all(den[ok] > 1e-6 * ref['S'][2][ok])


def test_tie_break_and_plateau_in_the_reference():
    T = np.full((9, 12), np.nan)
    T[4, 3] = T[4, 5] = 7.0
    T[2, 8] = T[2, 9] = T[3, 8] = 6.0
    assert list(F.peaks(T, 2, 5.0)) == [2 * 12 + 8, 4 * 12 + 3]
    assert list(F.peaks(T, 1, 5.0)) == [2 * 12 + 8, 4 * 12 + 3, 4 * 12 + 5]
    assert list(F.peaks(T, 2, 6.5)) == [4 * 12 + 3] and list(F.peaks(T, 2, 7.0)) == [4 * 12 + 3]
    assert F.parabola(1.0, 2.0, 1.0) == (0.0, False) and F.parabola(1.0, 2.0, 1.9)[0] == pytest.approx(0.45 / 1.1, abs=1e-15)
    assert F.parabola(np.nan, 2.0, 1.0) == (0.0, True) and F.parabola(2.0, 2.0, 2.0) == (0.0, True)
    assert F.parabola(1.0, 2.0, np.inf) == (0.0, True) and F.parabola(3.0, 2.0, 3.0) == (0.0, True)
    assert F.parabola(0.0, 1.0, 1.5) == (0.5, False) and F.parabola(1.5, 1.0, 0.0) == (-0.5, False)      # clamped


# ---- 2. what reaches C
@pytest.fixture
def ctx():
    c = make_ctx()
    yield c
    c._h = None


def _array(arg, count, ct, dt):
    assert isinstance(arg, C.c_void_p) and arg.value
    return np.frombuffer((ct * count).from_address(arg.value), dtype=dt).copy()


def _find_call(lib):
    """The one recorded call as a dict of its arguments (pointers as they came)."""
    assert len(lib.calls) == 1
    name, a = lib.calls[0]
    assert name == 'mpsfr_find_stars' and len(a) == 15
    assert isinstance(a[0], C.c_void_p) and a[0].value == HANDLE
    for k in (1, 2, 6, 7, 9, 14):
        assert isinstance(a[k], int) and not isinstance(a[k], bool), k
    assert isinstance(a[8], float)
    names = ('ny', 'nx', 'image', 'var', 'psf', 'half', 'sep', 'threshold', 'max_stars', 'rows', 'origin', 'count', 'map',
             'on_device')
    return dict(zip(names, a[1:]))


# mpsfr_find_stars(ctx, ny, nx, image, var, psf, half, sep, threshold, max_stars, star_out, origin_out, count_out, map_out,
#                  on_device)
def test_find_stars_host_minimal(ctx):
    rows, origin, nfound = ctx.find_stars(IMAGE, PSF)
    assert rows.shape == (0, _lib.NFIND) and origin.shape == (0, 2) and origin.dtype == np.int32 and nfound == 0
    c = _find_call(ctx.lib)
    assert (c['ny'], c['nx'], c['half'], c['sep'], c['threshold'], c['max_stars'], c['on_device']) == \
        (23, 31, 3, 3, 5.0, 4096, 0)
    assert np.array_equal(_array(c['image'], IMAGE.size, C.c_double, np.float64).reshape(IMAGE.shape), IMAGE)
    assert np.array_equal(_array(c['psf'], NS * NS, C.c_double, np.float64).reshape(NS, NS), PSF)
    assert c['var'] is None and c['map'] is None
    assert c['rows'].value == rows.ctypes.data and c['origin'].value == origin.ctypes.data
    assert rows.base is not None and rows.base.shape == (4096, _lib.NFIND) and rows.base.dtype == np.float64
    assert origin.base.shape == (4096, 2) and origin.base.flags.c_contiguous and rows.base.flags.c_contiguous
    assert list(_array(c['count'], 1, C.c_int32, np.int32)) == [0]


def test_find_stars_host_everything(ctx):
    masked = np.ma.masked_array(IMAGE, mask=IMAGE > 1.5)
    rows, origin, nfound, tmap = ctx.find_stars(masked, PSF.astype(np.float32), var=VAR.astype(np.float32), half=8, sep=16,
                                                threshold=-3, max_stars=7, return_map=True)
    c = _find_call(ctx.lib)
    assert (c['ny'], c['nx'], c['half'], c['sep'], c['threshold'], c['max_stars'], c['on_device']) == \
        (23, 31, 8, 16, -3.0, 7, 0)
    assert np.array_equal(_array(c['image'], IMAGE.size, C.c_double, np.float64).reshape(IMAGE.shape),
                          np.where(IMAGE > 1.5, np.nan, IMAGE), equal_nan=True)
    assert np.array_equal(_array(c['var'], VAR.size, C.c_double, np.float64).reshape(VAR.shape), VAR.astype(np.float32))
    assert np.array_equal(_array(c['psf'], NS * NS, C.c_double, np.float64).reshape(NS, NS), PSF.astype(np.float32))
    assert tmap.shape == IMAGE.shape and tmap.dtype == np.float64 and tmap.flags.c_contiguous
    assert c['map'].value == tmap.ctypes.data and rows.base.shape == (7, _lib.NFIND) and origin.base.shape == (7, 2)


def test_find_stars_device(ctx):
    assert ctx.find_stars_device(23, 31, DEV['image'], DEV['psf'], 3, 5, 6.5, 100, DEV['rows'], DEV['out']) is None
    c = _find_call(ctx.lib)
    assert (c['ny'], c['nx'], c['half'], c['sep'], c['threshold'], c['max_stars'], c['on_device']) == \
        (23, 31, 3, 5, 6.5, 100, 1)
    assert (c['image'].value, c['psf'].value, c['rows'].value, c['count'].value) == \
        (DEV['image'], DEV['psf'], DEV['rows'], DEV['out'])
    assert c['var'] is None and c['origin'] is None and c['map'] is None
    ctx.lib.calls.clear()
    ctx.find_stars_device(23, 31, DEV['image'], DEV['psf'], 1, 1, 0, 1, DEV['rows'], DEV['out'], var_ptr=DEV['var'],
                          origin_ptr=DEV['origin'], map_ptr=DEV['stamps'])
    c = _find_call(ctx.lib)
    assert (c['half'], c['sep'], c['threshold'], c['max_stars'], c['on_device']) == (1, 1, 0.0, 1, 1)
    assert (c['var'].value, c['origin'].value, c['map'].value) == (DEV['var'], DEV['origin'], DEV['stamps'])


def test_exports_and_header_constants():
    assert 'mpsfr_find_stars' in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    for name, val in (('NFIND', _lib.NFIND), ('FIND_MAX_HALF', _lib.FIND_MAX_HALF), ('FIND_MAX_SEP', _lib.FIND_MAX_SEP)):
        assert int(re.search(r'#define MPSFR_%s\s+(\d+)' % name, hdr).group(1)) == val, name
    assert (_lib.NFIND, _lib.FIND_MAX_HALF, _lib.FIND_MAX_SEP) == (8, 8, 16)
    import muse_psfr_amd
    assert (muse_psfr_amd.NFIND, muse_psfr_amd.FIND_MAX_HALF, muse_psfr_amd.FIND_MAX_SEP) == (8, 8, 16)
    assert muse_psfr_amd.find_stars is psfrec.find_stars and 'find_stars' in muse_psfr_amd.__doc__
    src = open(os.path.join(ROOT, 'muse_psfr_amd', 'csrc', 'find.hip')).read()
    assert int(re.search(r'constexpr int kTile = (\d+);', src).group(1)) == F.TILE
    assert re.search(r'constexpr int kMaxHalf = (\d+), kMaxSep = (\d+);', src).groups() == ('8', '16')


# ---- 3. the ValueErrors
def test_find_stars_refuses(ctx):
    flat, bad_core = PSF.copy(), PSF.copy()
    flat[17:24, 17:24] = 0.25                                            # constant over the 7 x 7 core, not beyond
    bad_core[20, 22] = np.nan
    base = dict(image=IMAGE, psf=PSF, var=None, half=3, sep=3, threshold=5.0, max_stars=10, return_map=False)
    bad = [dict(image=IMAGE[0]), dict(image=IMAGE[None]), dict(image=np.zeros((0, 4))), dict(image='frame'),
           dict(image=np.zeros((1, 16385))), dict(var=VAR[:-1]), dict(var=VAR.T), dict(var='v'),
           dict(psf=PSF[None]), dict(psf=PSF[:39]), dict(psf='p'), dict(psf=flat), dict(psf=bad_core),
           dict(psf=np.where(PSF == PSF.max(), np.inf, PSF)),
           dict(half=0), dict(half=9), dict(half=3.0), dict(half=True), dict(sep=0), dict(sep=17), dict(sep=2.0),
           dict(threshold=np.nan), dict(threshold=np.inf), dict(threshold=-np.inf), dict(threshold='5'),
           dict(threshold=None), dict(max_stars=0), dict(max_stars=2 ** 24 + 1), dict(max_stars=10.0),
           dict(return_map=1)]
    for kw in bad:
        args = dict(base)
        args.update(kw)
        image, psf = args.pop('image'), args.pop('psf')
        with pytest.raises(ValueError):
            ctx.find_stars(image, psf, **args)
    dev_ok = (23, 31, 1, 1, 3, 3, 5.0, 10, 1, 1)
    for k, v in [(0, 0), (1, 16385), (0, 23.0), (2, 0), (3, 0), (4, 0), (4, 9), (5, 0), (5, 17), (6, np.nan),
                 (6, np.inf), (7, 0), (7, 2 ** 24 + 1), (8, 0), (9, 0), (8, None)]:
        a = list(dev_ok)
        a[k] = v
        with pytest.raises(ValueError):
            ctx.find_stars_device(*a)
    with pytest.raises(ValueError):
        ctx.find_stars_device(8193, 8193, 1, 1, 3, 3, 5.0, 10, 1, 1)
    assert ctx.lib.calls == []
    # the bounds themselves are legal; a core constant at half = 3 is a filter at half = 4
    ctx.find_stars(np.zeros((1, 16384)), flat, half=4, sep=16, threshold=-1e300, max_stars=1)
    ctx.find_stars_device(16384, 4096, 1, 1, 8, 16, -5, 2 ** 24, 1, 1)
    assert len(ctx.lib.calls) == 2


def test_psfrec_find_stars_refuses(monkeypatch):
    ctx = make_ctx()
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: ctx)
    for kw in (dict(pixscale=0.0), dict(pixscale=np.nan), dict(sharp=1.0), dict(sharp=(0.5,)), dict(sharp=('a', None)),
               dict(sharp=(np.nan, 2.0)), dict(half=0), dict(sep=17), dict(threshold=np.inf), dict(max_stars=0)):
        with pytest.raises(ValueError):
            psfrec.find_stars(IMAGE, PSF, **kw)
    with pytest.raises(ValueError):
        psfrec.find_stars(IMAGE, PSF, VAR[:5])
    assert ctx.lib.calls == []


# ---- 4. psfrec.find_stars
class AnsweringLib(StubLib):
    """The recording stub, whose mpsfr_find_stars answers with the first max_stars of `rows` (pixel order) and their
    number, as the library would."""

    def __init__(self, rows):
        super().__init__()
        self.rows = np.asarray(rows, dtype=np.float64)

    def mpsfr_find_stars(self, *a):
        self.calls.append(('mpsfr_find_stars', a))
        n, cap = len(self.rows), a[9]
        out = np.full((cap, 8), np.nan)
        org = np.full((cap, 2), -(1 << 30), dtype=np.int32)
        m = min(n, cap)
        out[:m] = self.rows[:m]
        org[:m] = np.rint(self.rows[:m, :2]).astype(np.int32) - NS // 2
        C.memmove(a[10], out.ctypes.data, out.nbytes)
        C.memmove(a[11], org.ctypes.data, org.nbytes)
        C.memmove(a[12], np.array([n], dtype=np.int32).ctypes.data, 4)
        return 0


ROWS = np.array([[3.25, 7.5, 9.0, 90.0, 1.0, 1.1, 49, 0],        # pixel order; statistic 9, 30, 9, 12, 30
                 [5.0, 2.0, 30.0, 300.0, 2.0, 0.9, 49, 2],
                 [8.75, 20.25, 9.0, 91.0, 3.0, 12.0, 40, 0],       # a hot pixel: sharpness 12
                 [10.5, 11.5, 12.0, 120.0, 4.0, np.nan, 30, 4],
                 [15.0, 25.4, 30.0, 301.0, 5.0, 0.4, 49, 1]])


def _answering(monkeypatch, rows=ROWS):
    ctx = make_ctx()
    ctx.lib = AnsweringLib(rows)
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: ctx)
    return ctx


def test_psfrec_find_stars_sorts_stably_and_converts(monkeypatch):
    ctx = _answering(monkeypatch)
    t = psfrec.find_stars(IMAGE, PSF, VAR, threshold=6, half=2, pixscale=0.25)
    assert len(ctx.lib.calls) == 1
    a = ctx.lib.calls[0][1]
    assert (a[6], a[7], a[8], a[9], a[14]) == (2, 2, 6.0, 4096, 0) and a[4] is not None      # sep=None: half
    order = [1, 4, 3, 0, 2]                                              # descending; ties keep pixel order
    assert tuple(t.colnames) == ('position', 'origin', 'statistic', 'scale', 'back', 'sharp', 'npix', 'flags', 'shift')
    assert np.array_equal(t['statistic'], ROWS[order, 2]) and np.array_equal(t['position'], ROWS[order, :2])
    assert np.array_equal(t['scale'], ROWS[order, 3]) and np.array_equal(t['back'], ROWS[order, 4])
    assert np.array_equal(t['sharp'], ROWS[order, 5], equal_nan=True)
    assert np.asarray(t['npix']).dtype == np.int64 and list(t['npix']) == [49, 49, 30, 49, 40]
    assert np.asarray(t['flags']).dtype == np.int64 and list(t['flags']) == [2, 1, 4, 0, 0]
    origin = np.rint(ROWS[order, :2]).astype(np.int32) - NS // 2
    assert np.asarray(t['origin']).dtype == np.int32 and np.array_equal(t['origin'], origin)
    offset = ROWS[order, :2] - np.rint(ROWS[order, :2])
    assert np.allclose(t['shift'], offset * 0.25, rtol=0, atol=1e-14) and np.abs(t['shift']).max() <= 0.125
    ctx.lib.calls.clear()
    psfrec.find_stars(IMAGE, PSF, half=2, sep=5)
    a = ctx.lib.calls[0][1]
    assert (a[6], a[7], a[8]) == (2, 5, 5.0) and a[4] is None


def test_psfrec_find_stars_calls_again_when_the_buffer_was_short(monkeypatch):
    ctx = _answering(monkeypatch)
    t = psfrec.find_stars(IMAGE, PSF, max_stars=3)
    assert [c[1][9] for c in ctx.lib.calls] == [3, 5] and len(t) == 5
    assert np.array_equal(t['statistic'], [30.0, 30.0, 12.0, 9.0, 9.0])
    ctx.lib.calls.clear()
    assert len(psfrec.find_stars(IMAGE, PSF, max_stars=5)) == 5 and len(ctx.lib.calls) == 1


def test_psfrec_find_stars_applies_the_sharpness_bounds(monkeypatch):
    _answering(monkeypatch)
    assert list(psfrec.find_stars(IMAGE, PSF, sharp=(0.5, 1.5))['scale']) == [300.0, 90.0]
    assert list(psfrec.find_stars(IMAGE, PSF, sharp=(None, 1.5))['scale']) == [300.0, 301.0, 90.0]
    assert list(psfrec.find_stars(IMAGE, PSF, sharp=(1.0, None))['scale']) == [90.0, 91.0]   # NaN fails every bound
    assert len(psfrec.find_stars(IMAGE, PSF, sharp=(None, None))) == 5
    empty = psfrec.find_stars(IMAGE, PSF, sharp=(100.0, None))
    assert len(empty) == 0 and np.asarray(empty['shift']).shape == (0, 2)
    _answering(monkeypatch, np.zeros((0, 8)))
    none = psfrec.find_stars(IMAGE, PSF)
    assert len(none) == 0 and np.asarray(none['origin']).shape == (0, 2)
