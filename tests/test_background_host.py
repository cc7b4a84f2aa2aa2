"""Host: the background map (mpsfr_frame_background) without a GPU.

1. the yardstick alone (background_ref): a plane on the nodes is reproduced within the a-priori bound; on a constant plus
   unit Gaussian noise every cell's level and rms lie within six asymptotic deviations of a median and of a MAD; the cases
   written out by hand.
2. the sky loop on the references (frame_fit_ref + background_ref): on a background with a gradient the loop beats the
   single constant and comes within 1.5 x the error of the same stars and noise on a flat background.
3. what the new Context methods hand to C, argument by argument, against the recording stub of test_render_host.py; the
   ValueErrors of the validators, with no library call made; background_map on a frame and on a cube; the call sequence
   and the arithmetic of fit_crowded_stars(sky=...); sky=None makes exactly the one call it made before.
4. the exports, the header constants, the prototype against the ctypes binding, the header's "What a call writes".
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import background_ref as B
import frame_fit_ref as R
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec
from test_render_host import DEV, HANDLE, StubLib, make_ctx

NAN = np.nan
KC = np.float64(3.0) * np.float64(1.4826)


# ---- 1. the yardstick
@pytest.mark.parametrize('box', [16, 32])
def test_a_plane_on_the_nodes_is_reproduced_within_the_bound(box):
    ny, nx = B.FRAME
    my, mx = B.mesh_shape(ny, nx, box)
    a, b, c = 3.1, 0.27, -0.113
    yn, xn = (np.arange(my) + 0.5) * box - 0.5, (np.arange(mx) + 0.5) * box - 0.5
    M = a + b * yn[:, None] + c * xn[None, :]
    got, bound = B.interpolate(M, ny, nx, box)
    Y, X = np.mgrid[:ny, :nx]
    want = a + b * Y + c * X
    # the nodes and `want` are themselves rounded sums of three terms (3 eps of their absolute terms each); a node's
    # error reaches a pixel through weights of absolute sum <= (5/4)^2 and, at the edge, a continuation whose
    # absolute factors sum to 1 + 2 + 2 = 5 per axis: 3 eps mag (25 x 25/16 + 1) < 128 eps mag
    mag = abs(a) + abs(b) * (my * box + box) + abs(c) * (mx * box + box)
    err = np.abs(got - want)
    print('box %d: worst error %.3g, bound %.3g, slack %.3g' % (box, err.max(), bound.max(), 128 * B.EPS * mag))
    assert np.all(err <= bound + 128 * B.EPS * mag) and err.max() < 1e-13
    # replicated edge nodes would not: the outer half cell of a gradient needs the linear continuation
    assert abs(got[0, 0] - want[0, 0]) < 1e-13 < abs(M[0, 0] - want[0, 0])


def test_level_and_rms_of_gaussian_noise_lie_within_six_asymptotic_deviations():
    rng = np.random.default_rng(1)
    const = 100.0
    ref = B.background(const + rng.normal(size=(320, 320)), box=32, filter=1)
    mesh = ref['mesh'][0]
    assert mesh.shape == (10, 10, 8) and np.all(mesh[..., 5] == 1024) and np.all(ref['head'] == [0, 100, 0, 0])
    n_used = mesh[..., 4]
    dl = np.abs(mesh[..., 2] - const) * np.sqrt(n_used) / 1.2533
    dr = np.abs(mesh[..., 3] - 1.0) * np.sqrt(n_used) / (0.78 * 1.4826)
    print('worst level deviation %.2f, worst rms deviation %.2f of 6' % (dl.max(), dr.max()))
    assert dl.max() <= 6.0 and dr.max() <= 6.0
    assert np.all(n_used >= 1000) and np.any(mesh[..., 6] >= 1) and np.all(mesh[..., 7] == 0)      # 3 sigma: a few clipped
    assert np.array_equal(mesh[..., 0], mesh[..., 2]) and np.array_equal(mesh[..., 1], mesh[..., 3])     # filter 1
    assert np.abs(ref['map'] - const).max() < 0.5 and np.abs(ref['rms'] - 1.0).max() < 0.3


def test_cells_written_out_by_hand():
    est = B.cell_estimate
    # one valid pixel: the level is the pixel, MAD 0
    assert est([2.5], 64, KC, 5, 1 / 64) == [2.5, 0.0, 1.0, 1.0, 0.0, float(B.FLAT)]
    # two: the mean; both deviations equal the MAD, nothing is rejected
    assert est([-1.0, 4.0], 64, KC, 5, 1 / 64) == [1.5, 1.4826 * 2.5, 2.0, 2.0, 0.0, 0.0]
    # three: the middle one; d = 1, 0, 7, MAD 1, t = 4.4478: 9 goes in pass 1; then m = 1.5, d = 0.5, 0.5: stop
    assert est([2.0, 1.0, 9.0], 64, KC, 5, 1 / 64) == [1.5, 1.4826 * 0.5, 2.0, 3.0, 1.0, 0.0]
    # an outlier among nine: rejected in pass 1, the second pass rejects nothing
    x = [10.0, 11.0, 12.0, 13.0, 14.0, 15.0, 16.0, 17.0, 1000.0]
    assert est(x, 9, KC, 5, 0.25) == [13.5, 1.4826 * 2.0, 8.0, 9.0, 1.0, 0.0]
    # max_clip = 0: median and MAD of everything, flagged
    assert est(x, 9, KC, 0, 0.25) == [14.0, 1.4826 * 2.0, 9.0, 9.0, 0.0, float(B.CLIP_CAP)]
    # max_clip = 1: the cap falls on the pass that would have rejected nothing
    assert est(x, 9, KC, 1, 0.25) == [13.5, 1.4826 * 2.0, 8.0, 9.0, 1.0, float(B.CLIP_CAP)]
    # a flat cell (more than half of the values equal), also at max_clip = 0: both flags
    assert est([5.0] * 6 + [1.0, 9.0], 8, KC, 5, 0.25) == [5.0, 0.0, 8.0, 8.0, 0.0, float(B.FLAT)]
    assert est([5.0] * 6 + [1.0, 9.0], 8, KC, 0, 0.25) == [5.0, 0.0, 8.0, 8.0, 0.0, float(B.FLAT | B.CLIP_CAP)]
    # -0 and +0 in one cell: the level is +0 whatever the order
    for zeros in ([-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0], [-0.0, 0.0, -0.0]):
        row = est(zeros, 4, KC, 5, 0.25)
        assert row[0] == 0.0 and not np.signbit(row[0]) and row[1:] == [0.0, len(zeros), len(zeros), 0.0, float(B.FLAT)]
    # too few valid pixels: (double) n_valid >= min_frac (double) npix, one rounded product
    assert est([1.0] * 15, 64, KC, 5, 0.25)[5] == B.FILLED and est([1.0] * 16, 64, KC, 5, 0.25)[5] == B.FLAT
    row = est([], 64, KC, 5, 1e-300)
    assert np.isnan(row[0]) and np.isnan(row[1]) and row[2:] == [0.0, 0.0, 0.0, float(B.FILLED)]


def test_an_invalid_cell_is_filled_from_the_first_ring_that_holds_a_valid_one():
    # 7 x 7 cells of side 8; only the cells at distance 3 of the centre in row 0 are valid: filter 3 has h = 1, the rings
    # at r = 1 and 2 are empty, the one at r = h + 2 = 3 holds them
    image = np.full((56, 56), NAN)
    for j, v in ((0, 1.0), (2, 5.0), (5, 2.0), (6, 10.0)):
        image[0:8, 8 * j:8 * j + 8] = v
    ref = B.background(image, box=8, filter=3)
    mesh = ref['mesh'][0]
    assert np.all(ref['head'] == [1, 4, 45, 0])
    assert mesh[3, 3, 0] == 0.5 * 2.0 + 0.5 * 5.0 and mesh[3, 3, 7] == B.FILLED and np.isnan(mesh[3, 3, 2])
    assert mesh[0, 0, 0] == 1.0 and mesh[0, 1, 0] == 3.0 and mesh[0, 2, 0] == 5.0          # valid cells: their window
    assert mesh[0, 3, 0] == 5.0 and mesh[0, 4, 0] == 2.0                                   # filled at r = h: a neighbour
    assert mesh[6, 3, 0] == 3.5 and mesh[6, 0, 0] == 3.5                                   # r = 6: the whole row
    assert np.all(np.isfinite(mesh[..., :2])) and np.all(np.isfinite(ref['map']))


def test_an_all_nan_layer_beside_a_good_one():
    rng = np.random.default_rng(2)
    good = rng.normal(size=(20, 30))
    ref = B.background(np.stack([good, np.full((20, 30), NAN)]), box=8)
    one = B.background(good, box=8)
    assert np.array_equal(ref['mesh'][0], one['mesh'][0]) and np.array_equal(ref['map'][0], one['map'])
    assert np.all(ref['head'][1] == [2, 0, 12, 0]) and np.all(np.isnan(ref['mesh'][1][..., :4]))
    assert np.all(ref['mesh'][1][..., 4:7] == 0) and np.all(ref['mesh'][1][..., 7] == B.FILLED)
    assert np.all(np.isnan(ref['map'][1])) and np.all(np.isnan(ref['rms'][1]))


def test_scene_holds_what_the_gpu_test_needs():
    s = B.scene()
    for box, filled in ((8, True), (16, True), (33, True), (64, False)):
        ref = B.scene_reference(True, box, 3, 5)
        flags = ref['mesh'][0][..., 7].astype(int)
        assert bool(np.any(flags & B.FILLED)) == filled and ref['head'][0][0] == (1.0 if filled else 0.0)
        assert np.all(np.isfinite(ref['map'])) and np.isnan(ref['applied']).sum() == 1
        assert np.any(ref['mesh'][0][..., 6] >= 2)                       # the sources cost more than one pass somewhere
    assert np.any(B.scene_reference(True, 8, 3, 0)['mesh'][0][..., 7].astype(int) & B.CLIP_CAP)
    assert not np.array_equal(B.scene_reference(True, 16, 3, 5)['mesh'], B.scene_reference(False, 16, 3, 5)['mesh'])
    assert np.isinf(s['image']).sum() == 2 and np.isnan(s['image']).sum() > 1000


# ---- 2. the sky loop on the references
def test_the_sky_loop_beats_the_constant_and_comes_close_to_a_flat_background():
    """Measured on the references: rms flux error 6.92 on the flat background, 395 with one constant on the gradient,
    and 1.15 x the flat one with the loop (box 16, filter 1, 2 passes); 1.11 after a third pass."""
    s = B.sky_scene()

    def fit(frame, back=True):
        r = R.solve(frame, None, s['psf'], s['index'], s['origin'], s['shift'], B.SKY_RADIUS, back)
        assert r['head_status'] == 0 and np.all(r['status'] == 0)
        return r['F'], r['resid']

    def rms(F):
        return float(np.sqrt(np.mean((F - s['flux']) ** 2)))
    passes = B.SKY_PAR['passes']
    par = {k: v for k, v in B.SKY_PAR.items() if k != 'passes'}
    flat, const = rms(fit(s['flat'])[0]), rms(fit(s['image'])[0])
    sky, frame = B.sky_loop(s['image'], fit, passes, **par)
    loop = rms(fit(frame)[0])
    print('rms flux error: flat %.3f, constant b %.3f, sky loop %.3f (%.3f x flat); map error rms %.3f'
          % (flat, const, loop, loop / flat, np.sqrt(np.mean((sky - s['sky']) ** 2))))
    assert loop < const and loop <= 1.5 * flat
    assert const > 20 * flat                                             # (the scene is one a constant cannot fit)


# ---- 3. what reaches C
@pytest.fixture
def ctx():
    c = make_ctx()
    yield c
    c._h = None


_rng = np.random.default_rng(8)
IMAGE = _rng.normal(size=(23, 31))
VAR = _rng.uniform(0.5, 1.5, (23, 31))
CUBE = _rng.normal(size=(3, 23, 31))
NAMES = ('nl', 'ny', 'nx', 'image', 'var', 'box', 'filter', 'kappa', 'max_clip', 'min_frac', 'apply_to', 'mesh', 'head',
         'map', 'rms', 'applied', 'on_device')


def _array(arg, count):
    assert isinstance(arg, C.c_void_p) and arg.value
    return np.frombuffer((C.c_double * count).from_address(arg.value), dtype=np.float64).copy()


def _back_call(call):
    name, a = call
    assert name == 'mpsfr_frame_background' and len(a) == 18
    assert isinstance(a[0], C.c_void_p) and a[0].value == HANDLE
    for k in (1, 2, 3, 6, 7, 9, 17):
        assert isinstance(a[k], int) and not isinstance(a[k], bool), k
    assert isinstance(a[8], float) and isinstance(a[10], float)
    return dict(zip(NAMES, a[1:]))


# mpsfr_frame_background(ctx, nl, ny, nx, image, var, box, filter, kappa, max_clip, min_frac, apply_to, mesh_out, head_out,
#                        map_out, rms_out, applied_out, on_device)
def test_frame_background_host_minimal(ctx):
    out = ctx.frame_background(IMAGE)
    assert len(out) == 4
    bmap, rms, mesh, head = out
    c = _back_call(ctx.lib.calls[0])
    assert len(ctx.lib.calls) == 1
    assert [c[k] for k in ('nl', 'ny', 'nx', 'box', 'filter', 'kappa', 'max_clip', 'min_frac', 'on_device')] == \
        [1, 23, 31, 32, 3, 3.0, 5, 0.25, 0]
    assert np.array_equal(_array(c['image'], IMAGE.size).reshape(IMAGE.shape), IMAGE)
    assert c['var'] is None and c['apply_to'] is None and c['applied'] is None
    assert bmap.shape == rms.shape == (23, 31) and mesh.shape == (1, 1, 8) and head.shape == (4,)
    assert (c['mesh'].value, c['head'].value, c['map'].value, c['rms'].value) == \
        (mesh.ctypes.data, head.ctypes.data, bmap.ctypes.data, rms.ctypes.data)
    assert all(a.flags.c_contiguous and a.dtype == np.float64 for a in out)


def test_frame_background_host_everything(ctx):
    masked = np.ma.masked_array(CUBE, mask=CUBE > 1.5)
    var = np.stack([VAR] * 3).astype(np.float32)
    bmap, rms, mesh, head, applied = ctx.frame_background(masked, var, box=8, filter=5, kappa=2, max_clip=0, min_frac=1,
                                                          apply_to=CUBE + 1.0, return_rms=False)
    c = _back_call(ctx.lib.calls[0])
    assert [c[k] for k in ('nl', 'ny', 'nx', 'box', 'filter', 'kappa', 'max_clip', 'min_frac', 'on_device')] == \
        [3, 23, 31, 8, 5, 2.0, 0, 1.0, 0]
    assert np.array_equal(_array(c['image'], CUBE.size).reshape(CUBE.shape), np.where(CUBE > 1.5, NAN, CUBE), equal_nan=True)
    assert np.array_equal(_array(c['var'], CUBE.size).reshape(CUBE.shape), var)
    assert np.array_equal(_array(c['apply_to'], CUBE.size).reshape(CUBE.shape), CUBE + 1.0)
    assert rms is None and c['rms'] is None
    assert mesh.shape == (3, 3, 4, 8) and head.shape == (3, 4) and bmap.shape == applied.shape == CUBE.shape
    assert (c['mesh'].value, c['head'].value, c['map'].value, c['applied'].value) == \
        (mesh.ctypes.data, head.ctypes.data, bmap.ctypes.data, applied.ctypes.data)


def test_frame_background_device(ctx):
    assert ctx.frame_background_device(2, 23, 31, DEV['image'], DEV['rows'], DEV['out']) is None
    c = _back_call(ctx.lib.calls[0])
    assert [c[k] for k in ('nl', 'ny', 'nx', 'box', 'filter', 'kappa', 'max_clip', 'min_frac', 'on_device')] == \
        [2, 23, 31, 32, 3, 3.0, 5, 0.25, 1]
    assert (c['image'].value, c['mesh'].value, c['head'].value) == (DEV['image'], DEV['rows'], DEV['out'])
    assert all(c[k] is None for k in ('var', 'apply_to', 'map', 'rms', 'applied'))
    ctx.lib.calls.clear()
    ctx.frame_background_device(1, 23, 31, DEV['image'], DEV['rows'], DEV['out'], var_ptr=DEV['var'], map_ptr=DEV['stamps'],
                                rms_ptr=DEV['vstamps'], apply_to_ptr=DEV['psf'], applied_ptr=DEV['psf'], box=64, filter=1,
                                kappa=100, max_clip=16, min_frac=0.5)
    c = _back_call(ctx.lib.calls[0])
    assert [c[k] for k in ('box', 'filter', 'kappa', 'max_clip', 'min_frac', 'on_device')] == [64, 1, 100.0, 16, 0.5, 1]
    assert [c[k].value for k in ('var', 'map', 'rms', 'apply_to', 'applied')] == \
        [DEV['var'], DEV['stamps'], DEV['vstamps'], DEV['psf'], DEV['psf']]                # in place: one buffer


BAD_PARAMETERS = [dict(box=7), dict(box=65), dict(box=32.0), dict(box=True), dict(box=None), dict(filter=0), dict(filter=2),
                  dict(filter=4), dict(filter=7), dict(filter=3.0), dict(filter=True), dict(kappa=0.99), dict(kappa=100.1),
                  dict(kappa=NAN), dict(kappa=np.inf), dict(kappa='3'), dict(kappa=True), dict(max_clip=-1),
                  dict(max_clip=17), dict(max_clip=5.0), dict(min_frac=0), dict(min_frac=0.0), dict(min_frac=1.01),
                  dict(min_frac=NAN), dict(min_frac=-0.25), dict(min_frac=None)]


def test_frame_background_refuses(ctx):
    for kw in BAD_PARAMETERS + [dict(return_rms=1), dict(apply_to=IMAGE[:-1]), dict(apply_to='a'), dict(var=VAR.T),
                                dict(var='v')]:
        with pytest.raises(ValueError):
            ctx.frame_background(IMAGE, **kw)
    for kw in BAD_PARAMETERS:
        with pytest.raises(ValueError):
            _lib.background_parameters(**dict(B.DEFAULTS, **kw))
    too_many = np.broadcast_to(np.float64(0.0), (2, 8192, 4097))        # 2^26 + 2^14 pixels (a view: nothing allocated)
    for image in (IMAGE[0], CUBE[None], np.zeros((0, 4)), 'frame', np.zeros((1, 16385)), too_many):
        with pytest.raises(ValueError):
            ctx.frame_background(image)
    dev_ok = dict(nl=1, ny=23, nx=31, image_ptr=1, mesh_ptr=1, head_ptr=1)
    for kw in [dict(nl=0), dict(nl=1.0), dict(ny=0), dict(nx=16385), dict(nl=1 << 13, ny=128, nx=65), dict(image_ptr=0),
               dict(mesh_ptr=None), dict(head_ptr=0), dict(apply_to_ptr=5), dict(applied_ptr=5),
               dict(apply_to_ptr=5, applied_ptr=1)] + BAD_PARAMETERS:
        with pytest.raises(ValueError):
            ctx.frame_background_device(**dict(dev_ok, **kw))
    assert ctx.lib.calls == []
    # the bounds themselves are legal
    ctx.frame_background(np.zeros((1, 16384)), box=8, filter=1, kappa=1, max_clip=0, min_frac=1e-300)
    ctx.frame_background_device(1 << 12, 128, 128, 1, 1, 1, box=64, filter=5, kappa=100.0, max_clip=16, min_frac=1.0)
    assert len(ctx.lib.calls) == 2


class AnsweringLib(StubLib):
    """The recording stub, whose background call answers with map = `level` (+ the call's number), mesh rows 0 .. 7 and
    a head, and whose frame fit answers with F = the call's number, status 0 and the residual = image - 1."""

    def __init__(self, level=2.0):
        super().__init__()
        self.level = level
        self.images = []

    def mpsfr_frame_background(self, *a):
        self.calls.append(('mpsfr_frame_background', a))
        nl, ny, nx, box = a[1], a[2], a[3], a[6]
        self.images.append(_array(a[4], nl * ny * nx).reshape(nl, ny, nx))
        my, mx = B.mesh_shape(ny, nx, box)
        nback = sum(1 for c in self.calls if c[0] == 'mpsfr_frame_background')
        mesh = np.tile(np.arange(8.0), (nl * my * mx, 1)) + np.arange(nl * my * mx)[:, None] * 10
        head = np.tile([1.0, 5.0, 2.0, 0.0], (nl, 1)) + np.arange(nl)[:, None]
        for ptr, arr in ((a[12], mesh), (a[13], head), (a[14], np.full(nl * ny * nx, self.level * nback)),
                         (a[15], np.full(nl * ny * nx, 0.5))):
            if ptr is not None:
                assert arr.flags.c_contiguous
                C.memmove(ptr, arr.ctypes.data, arr.nbytes)
        return 0

    def mpsfr_fit_frame_psf(self, *a):
        self.calls.append(('mpsfr_fit_frame_psf', a))
        ny, nx, nstar = a[1], a[2], a[5]
        nfit = sum(1 for c in self.calls if c[0] == 'mpsfr_fit_frame_psf')
        image = _array(a[3], ny * nx)
        self.images.append(image.reshape(ny, nx))
        rows = np.zeros((nstar, 8))
        rows[:, 0] = nfit
        C.memmove(a[16], rows.ctypes.data, rows.nbytes)
        head, resid = np.zeros(8), image - 1.0
        C.memmove(a[17], head.ctypes.data, head.nbytes)
        if a[18] is not None:
            C.memmove(a[18], resid.ctypes.data, resid.nbytes)
        return 0


def _answering(monkeypatch, **kw):
    ctx = make_ctx()
    ctx.lib = AnsweringLib(**kw)
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: ctx)
    return ctx


def test_background_map_of_a_frame_and_of_a_cube(monkeypatch):
    ctx = _answering(monkeypatch)
    bmap, rms, mesh = psfrec.background_map(IMAGE, VAR, box=8, filter=1, kappa=2.5, max_clip=3, min_frac=0.5)
    c = _back_call(ctx.lib.calls[0])
    assert [c[k] for k in ('nl', 'ny', 'nx', 'box', 'filter', 'kappa', 'max_clip', 'min_frac', 'on_device')] == \
        [1, 23, 31, 8, 1, 2.5, 3, 0.5, 0]
    assert c['var'] is not None and c['apply_to'] is None and c['applied'] is None and c['rms'] is not None
    assert bmap.shape == rms.shape == IMAGE.shape and np.all(bmap == 2.0) and np.all(rms == 0.5)
    assert tuple(mesh.colnames) == ('level', 'rms', 'raw_level', 'raw_rms', 'n_used', 'n_valid', 'passes', 'flags')
    assert len(mesh) == 3 * 4 and list(mesh['level']) == [10.0 * k for k in range(12)]
    assert list(mesh['raw_rms']) == [10.0 * k + 3 for k in range(12)] and list(mesh['flags']) == [10 * k + 7 for k in range(12)]
    assert np.asarray(mesh['n_used']).dtype == np.int64 and np.asarray(mesh['level']).dtype == np.float64
    assert dict(mesh.meta) == dict(box=8, shape=(3, 4), status=1, valid_cells=5, filled_cells=2)
    ctx.lib.calls.clear()
    bmap, rms, mesh = psfrec.background_map(CUBE)
    c = _back_call(ctx.lib.calls[0])
    assert [c[k] for k in ('nl', 'ny', 'nx', 'box', 'filter', 'kappa', 'max_clip', 'min_frac')] == [3, 23, 31, 32, 3, 3.0, 5, 0.25]
    assert bmap.shape == rms.shape == CUBE.shape and len(mesh) == 3 and c['var'] is None
    assert dict(mesh.meta) == dict(box=32, shape=(3, 1, 1), status=[1, 2, 3], valid_cells=[5, 6, 7], filled_cells=[2, 3, 4])
    for kw in (dict(pixscale=0.0), dict(box=7), dict(filter=2)):
        with pytest.raises(ValueError):
            psfrec.background_map(IMAGE, **kw)
    with pytest.raises(ValueError):
        psfrec.background_map(IMAGE, VAR[:5])
    assert len(ctx.lib.calls) == 1


PSF = R.Y.models()[0]
POS = np.array([[5.0, 6.5], [12.25, 20.0], [18.0, 9.0]])


def test_sky_none_makes_exactly_the_call_it_made_before(monkeypatch):
    ctx = _answering(monkeypatch)
    fit, origin = psfrec.fit_crowded_stars(IMAGE, PSF, POS, var=VAR, radius=5.0, fit_back=False, start=[1.0, 2.0, 3.0],
                                           max_iter=7, tol=1e-3)
    assert [c[0] for c in ctx.lib.calls] == ['mpsfr_fit_frame_psf']
    a = ctx.lib.calls[0][1]
    assert len(a) == 20 and (a[1], a[2], a[5], a[6], a[12], a[13], a[14], a[15], a[19]) == (23, 31, 3, 1, 5.0, 0, 7, 1e-3, 0)
    assert np.array_equal(ctx.lib.images[0], IMAGE) and list(_array(a[11], 3)) == [1.0, 2.0, 3.0] and a[18] is None
    assert 'sky_passes' not in fit.meta and list(fit['scale']) == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        psfrec.fit_crowded_stars(IMAGE, PSF, POS, return_sky=True)
    for sky in (False, 1, 'yes', dict(boxes=8), dict(passes=0), dict(passes=9), dict(passes=2.0), dict(box=7),
                dict(filter=2), dict(kappa=0.5), dict(max_clip=17), dict(min_frac=0.0)):
        with pytest.raises(ValueError):
            psfrec.fit_crowded_stars(IMAGE, PSF, POS, sky=sky)
    with pytest.raises(ValueError):
        psfrec.fit_crowded_stars(IMAGE, PSF, POS, sky=True, return_sky=1)
    assert len(ctx.lib.calls) == 1


def test_the_call_sequence_and_the_arithmetic_of_the_sky_loop(monkeypatch):
    ctx = _answering(monkeypatch, level=0.3)
    masked = np.ma.masked_array(IMAGE, mask=IMAGE > 1.5)
    image = np.where(IMAGE > 1.5, NAN, IMAGE)
    fit, origin, resid, sky = psfrec.fit_crowded_stars(masked, PSF, POS, var=VAR, fit_back=False, start=[4.0, 5.0, 6.0],
                                                      sky=dict(box=8, filter=1, kappa=2.0, max_clip=1, min_frac=0.5,
                                                               passes=3),
                                                      return_residual=True, return_sky=True)
    names = [c[0] for c in ctx.lib.calls]
    assert names == ['mpsfr_fit_frame_psf', 'mpsfr_frame_background'] * 3 + ['mpsfr_fit_frame_psf']
    # the maps: 0.3, 0.6, 0.9 from the stub, summed in order; every frame is image - map, one rounded subtraction
    m1 = np.zeros(IMAGE.shape) + 0.3
    m2 = m1 + 0.6
    m3 = m2 + 0.9
    frames = [image, image - m1, image - m2, image - m3]
    fits = [c[1] for c in ctx.lib.calls if c[0] == 'mpsfr_fit_frame_psf']
    backs = [_back_call(c) for c in ctx.lib.calls if c[0] == 'mpsfr_frame_background']
    for k, (a, frame) in enumerate(zip(fits, frames)):
        assert np.array_equal(ctx.lib.images[2 * k], frame, equal_nan=True), k
        assert a[13] == (0 if k == 3 else _lib.FIT_BACKGROUND)           # one constant inside the loop, fit_back at the end
        assert (a[18] is not None) and a[4] is not None                  # the residual, the variances
        assert list(_array(a[11], 3)) == ([4.0, 5.0, 6.0] if k == 0 else [float(k)] * 3)     # started from the last fluxes
    for k, c in enumerate(backs):
        assert np.array_equal(ctx.lib.images[2 * k + 1][0], frames[k] - 1.0, equal_nan=True)     # the fit's residual
        assert [c[n] for n in ('nl', 'box', 'filter', 'kappa', 'max_clip', 'min_frac')] == [1, 8, 1, 2.0, 1, 0.5]
        assert c['var'] is not None and c['rms'] is None and c['apply_to'] is None and c['map'] is not None
    assert np.array_equal(sky, m3) and np.array_equal(resid, frames[3] - 1.0, equal_nan=True)
    assert fit.meta['sky_passes'] == 3 and list(fit['scale']) == [4.0] * 3
    # sky=True: the defaults, two passes
    ctx.lib.calls.clear()
    fit, origin = psfrec.fit_crowded_stars(IMAGE, PSF, POS, sky=True)
    assert [c[0] for c in ctx.lib.calls] == ['mpsfr_fit_frame_psf', 'mpsfr_frame_background'] * 2 + ['mpsfr_fit_frame_psf']
    c = _back_call(ctx.lib.calls[1])
    assert [c[n] for n in ('box', 'filter', 'kappa', 'max_clip', 'min_frac')] == [32, 3, 3.0, 5, 0.25] and c['var'] is None
    assert fit.meta['sky_passes'] == 2 and ctx.lib.calls[-1][1][13] == _lib.FIT_BACKGROUND


# ---- 4. exports, constants, prototype
def test_exports_and_header_constants():
    import muse_psfr_amd
    assert 'mpsfr_frame_background' in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    for name in ('NBACK', 'NBACK_HEAD', 'BACKGROUND_MIN_BOX', 'BACKGROUND_MAX_BOX', 'BACKGROUND_MAX_CLIP', 'BACK_FILLED',
                 'BACK_CLIP_CAP', 'BACK_FLAT'):
        val = int(re.search(r'#define MPSFR_%s\s+(\d+)' % name, hdr).group(1))
        assert val == getattr(_lib, name) == getattr(muse_psfr_amd, name), name
    assert (_lib.NBACK, _lib.NBACK_HEAD, _lib.BACKGROUND_MIN_BOX, _lib.BACKGROUND_MAX_BOX, _lib.BACKGROUND_MAX_CLIP) == \
        (B.NBACK, B.NHEAD, 8, 64, 16)
    assert (_lib.BACK_FILLED, _lib.BACK_CLIP_CAP, _lib.BACK_FLAT) == (B.FILLED, B.CLIP_CAP, B.FLAT) == (1, 2, 4)
    assert muse_psfr_amd.background_map is psfrec.background_map and 'background_map' in muse_psfr_amd.__doc__
    src = open(os.path.join(ROOT, 'muse_psfr_amd', 'csrc', 'background.hip')).read()
    assert re.search(r'constexpr int kMinBox = (\d+), kMaxBox = (\d+);', src).groups() == ('8', '64')
    assert re.search(r'constexpr double kMadToSigma = ([\d.]+);', src).group(1) == '1.4826' == repr(B.MAD_TO_SIGMA)
    build = __import__('muse_psfr_amd._build', fromlist=['SOURCES'])
    assert 'background.hip' in build.SOURCES


def test_the_prototype_agrees_with_the_ctypes_binding():
    hdr = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    proto = re.search(r'\bint mpsfr_frame_background\((.*?)\);', hdr, flags=re.S).group(1)
    args = [' '.join(a.split()) for a in proto.split(',')]
    assert [a.rsplit(' ', 1)[-1].lstrip('*') for a in args] == ['ctx'] + [
        'nl', 'ny', 'nx', 'image', 'var', 'box', 'filter', 'kappa', 'max_clip', 'min_frac', 'apply_to', 'mesh_out', 'head_out',
        'map_out', 'rms_out', 'applied_out', 'on_device']
    want = [C.c_void_p if '*' in a else C.c_double if a.startswith('double') else C.c_int for a in args]
    lib = _lib.load()
    assert list(lib.mpsfr_frame_background.argtypes) == want and lib.mpsfr_frame_background.restype is C.c_int
    assert [a for a in args if '*' in a and 'const' not in a] == ['mpsfr_ctx* ctx', 'double* mesh_out', 'double* head_out',
                                                                    'double* map_out', 'double* rms_out', 'double* applied_out']


def test_what_a_call_writes_names_the_call():
    hdr = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    para = re.search(r'/\* What a call writes\..*?\*/', hdr, flags=re.S).group(0)
    assert 'fifteen' in para and 'mpsfr_frame_background' in para
    assert 'mpsfr_frame_background' in hdr[hdr.index('int mpsfr_fit_frame_psf(') - 6000:hdr.index('int mpsfr_fit_frame_psf(')]
