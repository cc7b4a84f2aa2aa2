"""GPU: the background map (mpsfr_frame_background), both precisions.

1. parity with the NumPy restatement (background_ref) on the 97 x 150 scene, with and without var, box 8, 16, 33 and 64,
   filter 1, 3 and 5, max_clip 0 and 5: mesh_out and head_out bit for bit; map_out, rms_out and applied_out within the
   reference's a-priori bound, NaN exactly where the reference has it.
2. the shapes and cell contents where the kernel can go wrong, against the same reference; the case table of
   background_cases.py, each case certified on the reference to reach its path: rows of more than 256 pixels (each map
   also asked for alone), more than 256 cells, a cube of dense, sparse and dead layers (each layer = the call on it,
   device = host), the ring search on sparse and long meshes, ties on a ring, n_valid across the sort sizes, 16 passes and
   one-sided clipping, min_frac at equality, the rms clamp (exactly 0 where the unclamped reference is negative).
3. invariances, bit for bit: host = device pointers, mixed = f64, a second call, a call after other work of the context,
   each optional output given or NULL, a layer of a cube = the call on that layer, permutations inside the cells,
   negation, a factor 2^11, the scene moved inside a NaN frame.
4. call history and writes: the checked call after a larger, a smaller, another tenant's, a non-finite and a refused call
   equals a fresh context; the device form into buffers prefilled with 0xA5; every refusal writes nothing.
5. the chain fit -> background of the residual -> subtract -> fit on device buffers against the same chain on host
   pointers, bit for bit, and stage by stage against the references; fit_crowded_stars(sky=...) against the two
   assertions of the reference loop (test_background_host.py).
6. profiling.
Every raw call has canaries behind each output.  Margins go to record_margin('background', ...).
"""
import ctypes as C

import numpy as np
import pytest

import background_cases as K
import background_ref as B
from conftest import record_margin

pytestmark = pytest.mark.gpu

PRECS = ['mixed', 'f64']
SENT, CAN = -7.25, 16
OUTS = ('mesh', 'head', 'map', 'rms', 'applied')


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


def _sizes(nl, ny, nx, box):
    box = box if 1 <= box <= 1 << 20 else 8
    my, mx = B.mesh_shape(max(ny, 1), max(nx, 1), box)
    nl = max(nl, 1)
    npix = min(nl * max(ny, 1) * max(nx, 1), 1 << 20)
    return dict(mesh=min(nl * my * mx * 8, 1 << 20), head=min(nl * 4, 1 << 20), map=npix, rms=npix, applied=npix), (my, mx)


def raw_back(ctx, image, var=None, apply_to=None, want=('map', 'rms'), expect_rc=0, override=None, **par):
    """mpsfr_frame_background on host pointers with canaries behind every output.  Returns a dict of the outputs (None for
    one not asked for); after a refusal it asserts that every output is untouched."""
    p = dict(B.DEFAULTS)
    p.update(par)
    image = np.ascontiguousarray(image, dtype=np.float64)
    cube = image.reshape((-1,) + image.shape[-2:])
    nl, ny, nx = cube.shape
    a = dict(nl=nl, ny=ny, nx=nx, image=cube, var=None if var is None else np.ascontiguousarray(var, dtype=np.float64),
             apply=None if apply_to is None else np.ascontiguousarray(apply_to, dtype=np.float64), **p)
    a.update({k: v for k, v in (override or {}).items() if k not in OUTS})
    size, (my, mx) = _sizes(a['nl'], a['ny'], a['nx'], a['box'])
    want = set(want) | {'mesh', 'head'} | ({'applied'} if apply_to is not None else set())
    buf = {k: np.full(size[k] + CAN, SENT) for k in OUTS}
    given = {k: (buf[k] if k in want else None) for k in OUTS}
    given.update({k: v for k, v in (override or {}).items() if k in OUTS})
    rc = ctx.lib.mpsfr_frame_background(ctx._h, a['nl'], a['ny'], a['nx'], _ptr(a['image']), _ptr(a['var']), a['box'],
                                        a['filter'], a['kappa'], a['max_clip'], a['min_frac'], _ptr(a['apply']),
                                        _ptr(given['mesh']), _ptr(given['head']), _ptr(given['map']), _ptr(given['rms']),
                                        _ptr(given['applied']), 0)
    assert rc == expect_rc, (rc, ctx.lib.mpsfr_last_error())
    for k in OUTS:
        assert np.all(buf[k][size[k]:] == SENT), k
        if rc != 0 or given[k] is None:
            assert np.all(buf[k] == SENT), k
    if rc != 0:
        return dict(rc=rc)
    out = dict(rc=rc, mesh=buf['mesh'][:size['mesh']].reshape(nl, my, mx, 8), head=buf['head'][:size['head']].reshape(nl, 4))
    for k in ('map', 'rms', 'applied'):
        out[k] = buf[k][:size[k]].reshape(image.shape) if given[k] is not None else None
    return out


def assert_parity(got, ref, tag, apply=None):
    """mesh and head bit for bit, the maps within the a-priori bounds; returns the worst error / bound.
    applied_out is apply_to - map_out in one rounded subtraction (include/mpsfr.h).  Against the reference its bound
    is therefore the map's and the two subtractions' own roundings: fl(a - m) - fl(a - m') = (m' - m) + (a - m) d -
    (a - m') d' with |d|, |d'| <= eps, to first order |m - m'| + 2 eps |a - m'| (where the map is small beside
    apply_to, half an ulp of the difference is more than the whole bound of the map).  With `apply` given and both
    planes asked for, applied_out is also held to the call's own map_out, bit for bit."""
    assert _same(got['mesh'], ref['mesh'].reshape(got['mesh'].shape)), tag
    assert _same(got['head'], ref['head'].reshape(got['head'].shape)), tag
    if apply is not None and got.get('map') is not None and got.get('applied') is not None:
        with np.errstate(invalid='ignore'):
            own = np.asarray(apply, dtype=np.float64).reshape(got['map'].shape) - got['map']
        fin = np.isfinite(own)
        assert np.array_equal(np.isnan(got['applied']), np.isnan(own)) and _same(got['applied'][fin], own[fin]), tag
    worst = 0.0
    for k, bk in (('map', 'map_bound'), ('rms', 'rms_bound'), ('applied', 'map_bound')):
        if got.get(k) is None or ref.get(k) is None:
            continue
        nan = np.isnan(ref[k])
        assert np.array_equal(np.isnan(got[k]), nan), (tag, k)
        fin = np.isfinite(ref[k])
        assert _same(got[k][~nan & ~fin], ref[k][~nan & ~fin]), (tag, k)
        err, bnd = np.abs(got[k][fin] - ref[k][fin]), ref[bk][fin]
        if k == 'applied':
            bnd = bnd + 2.0 * B.EPS * np.abs(ref[k][fin])
        some = err > 0
        ratio = float(np.max(err[some] / bnd[some])) if some.any() else 0.0
        print('%s %s: worst error / bound %.3f' % (tag, k, ratio))
        assert np.all(err <= bnd), (tag, k, ratio)
        worst = max(worst, ratio)
    return worst


# ---- 1. parity on the scene
@pytest.mark.parametrize('max_clip', [0, 5])
@pytest.mark.parametrize('filter', [1, 3, 5])
@pytest.mark.parametrize('box', [8, 16, 33, 64])
@pytest.mark.parametrize('usevar', [True, False])
@pytest.mark.parametrize('prec', PRECS)
def test_parity_with_numpy_on_the_scene(ctx, prec, usevar, box, filter, max_clip):
    s = B.scene()
    ref = B.scene_reference(usevar, box, filter, max_clip)
    got = raw_back(ctx, s['image'], s['var'] if usevar else None, s['apply'], box=box, filter=filter, max_clip=max_clip)
    worst = assert_parity(got, ref, 'scene var=%d box=%d filter=%d clip=%d' % (usevar, box, filter, max_clip), s['apply'])
    record_margin('background', map_error_over_bound=worst)


# ---- 2. shapes and cell contents
def _shape_cases():
    rng = np.random.default_rng(41)
    cases = {}
    for name, shape, box in (('1x1', (1, 1), 8), ('1x200', (1, 200), 16), ('200x1', (200, 1), 16), ('7x9', (7, 9), 8),
                             ('64x64', (64, 64), 64), ('128x130', (128, 130), 64), ('33x65b8', (33, 65), 8),
                             ('33x65b32', (33, 65), 32)):
        cases[name] = (rng.normal(size=shape) + 3.0, None, dict(box=box))
    one = np.full((16, 24), np.nan)
    one[3, 4] = 2.5                                                      # a cell with exactly 1 valid pixel
    one[9, 1], one[12, 7] = -1.0, 4.0                                    # ... with exactly 2
    one[:8, 8:16] = rng.normal(size=(8, 8))
    cases['one and two valid'] = (one, None, dict(box=8, min_frac=1.0 / 64))
    cases['4096 equal'] = (np.full((64, 128), 7.0), None, dict(box=64))
    cases['three values'] = (rng.choice([1.0, 2.0, 2.5], size=(32, 64)), None, dict(box=32))
    cases['three values, kappa 1'] = (rng.choice([1.0, 2.0, 2.5], size=(32, 64), p=[0.5, 0.3, 0.2]), None,
                                      dict(box=32, kappa=1.0, max_clip=16))
    wide = rng.choice([-1.0, 1.0], size=(40, 72)) * 10.0 ** rng.uniform(-300, 300, size=(40, 72))
    cases['1e-300 .. 1e300'] = (wide, None, dict(box=16))
    bad = rng.normal(size=(40, 72))
    bad[rng.uniform(size=bad.shape) < 0.2] = np.nan
    bad[rng.uniform(size=bad.shape) < 0.1] = np.inf
    bad[rng.uniform(size=bad.shape) < 0.1] = -np.inf
    cases['inf and NaN pixels'] = (bad, None, dict(box=16))
    var = np.ones((40, 72))
    var[16:32, 32:48] = 0.0
    cases['a tile masked by var'] = (rng.normal(size=(40, 72)), var, dict(box=16, filter=1))
    cases['all NaN'] = (np.full((40, 72), np.nan), None, dict(box=16))
    return cases


CASES = _shape_cases()


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('prec', PRECS)
def test_shapes_and_cells_where_the_kernel_can_go_wrong(ctx, prec, name):
    image, var, par = CASES[name]
    ref = B.background(image, var, apply_to=image, **par)
    got = raw_back(ctx, image, var, image, **par)
    assert_parity(got, ref, name, image)
    if name == 'all NaN':
        assert np.all(got['head'] == [2.0, 0.0, 15.0, 0.0]) and np.all(np.isnan(got['map'])) and np.all(np.isnan(got['rms']))
        assert np.all(np.isnan(got['mesh'][..., :4])) and np.all(got['mesh'][..., 4:7] == 0) and np.all(got['mesh'][..., 7] == 1)
    if name == '4096 equal':
        assert np.all(got['mesh'][..., 0] == 7.0) and np.all(got['mesh'][..., 1] == 0.0) and np.all(got['mesh'][..., 4] == 4096)
        assert np.all(got['mesh'][..., 7] == B.FLAT)
    if name == 'one and two valid':
        m = got['mesh'][0]
        assert m[0, 0, 2] == 2.5 and m[0, 0, 5] == 1 and m[1, 0, 2] == 1.5 and m[1, 0, 3] == 1.4826 * 2.5 and m[1, 0, 5] == 2


@pytest.mark.parametrize('name', K.NAMES)
@pytest.mark.parametrize('prec', PRECS)
def test_parity_on_the_case_table(ctx, prec, name):
    """The cases of background_cases.py: wide rows, more than 256 cells, the ring search, ties, the sort sizes, long and
    one-sided clipping, min_frac at equality, the rms clamp.  That a case reaches its path is its certificate on the
    reference (test_background_cases_host.py, and once more here); the comparison is the one of the scene."""
    d, ref = K.inputs(name), K.reference(name)
    failed = [claim for claim, holds in K.certificate(name) if not holds]
    assert not failed, failed
    image, var, apply, par, family = d['image'], d['var'], d['apply'], d['par'], K.family(name)
    got = raw_back(ctx, image, var, apply, **par)
    worst = assert_parity(got, ref, name, apply)
    if family == 'clamp':
        below = K.clamped_pixels(ref)
        assert below.any() and np.all(got['rms'][below] == 0.0)
    if family == 'wide':
        # one plane at a time: the level and the rms branch of the fill of sE each on their own, past the first block
        alone = raw_back(ctx, image, var, None, want=('rms',), **par)
        assert alone['map'] is None and alone['applied'] is None and _same(alone['rms'], got['rms'])
        worst = max(worst, assert_parity(alone, ref, name + ', rms_out alone'))
        alone = raw_back(ctx, image, var, apply, want=(), **par)
        assert alone['map'] is None and alone['rms'] is None and _same(alone['applied'], got['applied'])
        worst = max(worst, assert_parity(alone, ref, name + ', applied_out alone'))
    if image.ndim == 3 and family == 'cells':
        for layer in range(len(image)):
            one = raw_back(ctx, image[layer], None, apply[layer], **par)
            for k in OUTS:
                assert _same(got[k][layer], one[k][0] if k in ('mesh', 'head') else one[k]), (layer, k)
        assert _equal(device_back(ctx, image, None, apply, **par), got)
    print('%s (%s): worst error / bound %.3f' % (name, family, worst))
    record_margin('background', map_error_over_bound=worst, **{'map_error_over_bound_' + family: worst})


@pytest.mark.parametrize('prec', PRECS)
def test_more_layers_than_a_grid_dimension(ctx, prec):
    """70 000 layers of one pixel: the layer is a grid dimension of 65 535 at most, so the call launches twice.  A
    cell of one pixel is its pixel with MAD 0; a NaN pixel is a dead layer."""
    nl = 70000
    cube = np.arange(nl, dtype=np.float64).reshape(nl, 1, 1) - 3.25
    dead = np.array([0, 65534, 65535, 65536, nl - 1])
    cube[dead] = np.nan
    got = raw_back(ctx, cube, None, cube)
    want = np.tile([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, float(B.FLAT)], (nl, 1))
    want[:, 0] = want[:, 2] = cube[:, 0, 0]
    want[dead] = [np.nan, np.nan, np.nan, np.nan, 0.0, 0.0, 0.0, float(B.FILLED)]
    head = np.tile([0.0, 1.0, 0.0, 0.0], (nl, 1))
    head[dead] = [2.0, 0.0, 1.0, 0.0]
    assert _same(got['mesh'].reshape(nl, 8), want) and _same(got['head'], head)
    live = np.ones(nl, dtype=bool)
    live[dead] = False
    # one cell: every tap is its level, and the weights of an axis sum to 1 within 4 roundings
    assert np.all(np.abs(got['map'][live] - cube[live]) <= 16 * B.EPS * np.abs(cube[live])) and np.all(got['rms'][live] == 0.0)
    assert np.all(np.isnan(got['map'][dead])) and np.all(np.isnan(got['rms'][dead])) and np.all(np.isnan(got['applied'][dead]))
    assert np.all(np.abs(got['applied'][live]) <= 16 * B.EPS * np.abs(cube[live]))


# ---- 3. invariances
def _to_dev(torch, a):
    return torch.from_numpy(np.array(a, order='C')).to(torch.device('cuda:0'))


def device_back(ctx, image, var=None, apply_to=None, want=('map', 'rms'), fill=None, in_place=False, **par):
    """The device form into prefilled buffers (SENT, or the byte `fill`) with canaries; the outputs as raw_back's."""
    import torch
    p = dict(B.DEFAULTS)
    p.update(par)
    image = np.ascontiguousarray(image, dtype=np.float64)
    cube = image.reshape((-1,) + image.shape[-2:])
    nl, ny, nx = cube.shape
    size, (my, mx) = _sizes(nl, ny, nx, p['box'])
    want = set(want) | {'mesh', 'head'} | ({'applied'} if apply_to is not None else set())
    dev = torch.device('cuda:0')
    tim = _to_dev(torch, cube)
    tva = None if var is None else _to_dev(torch, var)
    tap = None if apply_to is None else _to_dev(torch, apply_to)
    buf = {}
    for k in OUTS:
        if fill is None:
            buf[k] = torch.full((size[k] + CAN,), SENT, dtype=torch.float64, device=dev)
        else:
            buf[k] = torch.full(((size[k] + CAN) * 8,), fill, dtype=torch.uint8, device=dev).view(torch.float64)
    if in_place:
        buf['applied'][:size['applied']] = tap.reshape(-1)
        tap = buf['applied']
    torch.cuda.synchronize()
    ptr = {k: (buf[k].data_ptr() if k in want else None) for k in OUTS}
    ctx.frame_background_device(nl, ny, nx, tim.data_ptr(), ptr['mesh'], ptr['head'],
                                var_ptr=None if tva is None else tva.data_ptr(), map_ptr=ptr['map'], rms_ptr=ptr['rms'],
                                apply_to_ptr=None if tap is None else tap.data_ptr(), applied_ptr=ptr['applied'], **p)
    ctx.sync()
    host = {k: buf[k].cpu().numpy() for k in OUTS}
    sent = np.full(1, SENT) if fill is None else np.frombuffer(bytes([fill]) * 8, dtype=np.float64)
    out = {}
    for k in OUTS:
        assert host[k][size[k]:].tobytes() == np.repeat(sent, CAN).tobytes(), k
        if k not in want:
            assert host[k].tobytes() == np.repeat(sent, size[k] + CAN).tobytes(), k
        out[k] = host[k][:size[k]] if k in want else None
    out['mesh'], out['head'] = out['mesh'].reshape(nl, my, mx, 8), out['head'].reshape(nl, 4)
    for k in ('map', 'rms', 'applied'):
        out[k] = None if out[k] is None else out[k].reshape(image.shape)
    return out


def _equal(a, b, keys=OUTS):
    return all((a[k] is None and b[k] is None) or _same(a[k], b[k]) for k in keys)


_BASE = {}


def _base(api, prec, usevar=True):
    """The scene through the host-pointer call with the default parameters, once per precision."""
    if (prec, usevar) not in _BASE:
        s = B.scene()
        _BASE[prec, usevar] = raw_back(_ctx(api, prec), s['image'], s['var'] if usevar else None, s['apply'])
    return _BASE[prec, usevar]


@pytest.mark.parametrize('usevar', [True, False])
@pytest.mark.parametrize('prec', PRECS)
def test_device_pointers_equal_host_pointers(api, ctx, prec, usevar):
    s = B.scene()
    var = s['var'] if usevar else None
    base = _base(api, prec, usevar)
    assert _equal(device_back(ctx, s['image'], var, s['apply']), base)
    assert _equal(device_back(ctx, s['image'], var, s['apply'], in_place=True), base)


def test_mixed_equals_f64(api):
    for usevar in (True, False):
        assert _equal(_base(api, 'mixed', usevar), _base(api, 'f64', usevar))


@pytest.mark.parametrize('prec', PRECS)
def test_a_second_call_other_work_and_the_optional_outputs(api, ctx, prec):
    import find_ref as F
    s = B.scene()
    base = _base(api, prec)
    assert _equal(raw_back(ctx, s['image'], s['var'], s['apply']), base)
    f = F.scene()
    ctx.find_stars(f['image'], f['psf'], var=f['var'])
    raw_back(ctx, s['image'][:50, :70], None, box=8, filter=5, kappa=2.0)
    assert _equal(raw_back(ctx, s['image'], s['var'], s['apply']), base)
    for want, apply in (((), None), (('map',), None), (('rms',), None), ((), s['apply']), (('map', 'rms'), None)):
        got = raw_back(ctx, s['image'], s['var'], apply, want=want)
        for k in OUTS:
            assert got[k] is None or _same(got[k], base[k]), (want, k)


@pytest.mark.parametrize('prec', PRECS)
def test_a_layer_of_a_cube_is_the_call_on_that_layer(ctx, prec):
    s = B.scene()
    rng = np.random.default_rng(9)
    cube = np.stack([s['image'], s['image'][::-1], np.full(B.FRAME, np.nan), s['image'] * 3.0, rng.normal(size=B.FRAME)])
    var = np.stack([s['var']] * 5)
    apply = np.stack([s['apply']] * 5)
    got = raw_back(ctx, cube, var, apply, box=16)
    assert list(got['head'][:, 0]) == [1.0, 1.0, 2.0, 1.0, 1.0]
    for layer in range(5):
        one = raw_back(ctx, cube[layer], var[layer], apply[layer], box=16)
        for k in OUTS:
            assert _same(got[k][layer], one[k][0] if k in ('mesh', 'head') else one[k]), (layer, k)
    assert _equal(device_back(ctx, cube, var, apply, box=16), got)


@pytest.mark.parametrize('box', [8, 33])
@pytest.mark.parametrize('prec', PRECS)
def test_permutation_negation_and_scaling(ctx, prec, box):
    s = B.scene()
    base = raw_back(ctx, s['image'], s['var'], box=box)
    perm = raw_back(ctx, B.permute_cells(s['image'], box, np.random.default_rng(3)),
                    B.permute_cells(s['var'], box, np.random.default_rng(3)), box=box)
    assert _same(perm['mesh'][..., 2:], base['mesh'][..., 2:])
    assert _same(perm['mesh'], base['mesh']) and _same(perm['head'], base['head'])
    neg = raw_back(ctx, -s['image'], s['var'], box=box)
    assert np.array_equal(neg['mesh'][..., [0, 2]], -base['mesh'][..., [0, 2]], equal_nan=True)      # (NaN: invalid cells)
    assert np.isfinite(base['mesh'][..., 0]).all() and np.isnan(base['mesh'][..., 2]).any()
    assert _same(neg['mesh'][..., [1, 3, 4, 5, 6, 7]], base['mesh'][..., [1, 3, 4, 5, 6, 7]]) and _same(neg['head'], base['head'])
    big = raw_back(ctx, s['image'] * 2048.0, s['var'], box=box)
    assert _same(big['mesh'][..., :4], base['mesh'][..., :4] * 2048.0) and _same(big['mesh'][..., 4:], base['mesh'][..., 4:])


@pytest.mark.parametrize('prec', PRECS)
def test_the_scene_moved_inside_a_nan_frame(ctx, prec):
    s = B.scene()
    box = 16
    base = raw_back(ctx, s['image'], s['var'], box=box, filter=1)
    ny, nx = B.FRAME
    oy, ox = 2 * box, 3 * box
    frame, var = np.full((ny + oy + 5, nx + ox + 20), np.nan), np.ones((ny + oy + 5, nx + ox + 20))
    frame[oy:oy + ny, ox:ox + nx], var[oy:oy + ny, ox:ox + nx] = s['image'], s['var']
    got = raw_back(ctx, frame, var, box=box, filter=1)
    my, mx = base['mesh'].shape[1:3]
    moved, want = got['mesh'][0, 2:2 + my, 3:3 + mx, 2:], base['mesh'][0, :, :, 2:]
    # (a partial cell of the scene is a whole cell of the larger frame: another npix, so another validity rule)
    full = np.zeros((my, mx), dtype=bool)
    full[:ny // box, :nx // box] = True
    assert full.sum() == 54 and _same(moved[full], want[full])


# ---- 4. call history and writes
@pytest.mark.parametrize('prec', PRECS)
def test_checked_call_after_predecessor_equals_fresh(api, prec):
    import find_ref as F
    s = B.scene()
    fresh = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision=prec)
    base = raw_back(fresh, s['image'], s['var'], s['apply'])
    fresh.close()
    ctx = _ctx(api, prec)
    rng = np.random.default_rng(17)
    f = F.scene()
    wild = rng.normal(size=(120, 200))
    wild[::3] = np.nan
    wild[1::3] = np.inf
    pred = {'L': lambda: raw_back(ctx, rng.normal(size=(3, 200, 310)), box=64, filter=5),
            'S': lambda: raw_back(ctx, rng.normal(size=(9, 11)), box=8, filter=1),
            'X': lambda: ctx.find_stars(f['image'], f['psf'], var=f['var']),
            'N': lambda: raw_back(ctx, wild, wild, wild, box=8),
            'F': lambda: raw_back(ctx, s['image'], expect_rc=-1, box=7)}
    for name, call in pred.items():
        call()
        assert _equal(raw_back(ctx, s['image'], s['var'], s['apply']), base), name


@pytest.mark.parametrize('prec', PRECS)
def test_device_form_writes_every_documented_element_and_nothing_else(api, ctx, prec):
    s = B.scene()
    base = _base(api, prec)
    got = device_back(ctx, s['image'], s['var'], s['apply'], fill=0xA5)     # (the canaries are checked in device_back)
    assert _equal(got, base)
    bare = device_back(ctx, s['image'], s['var'], None, want=(), fill=0xA5)
    assert _same(bare['mesh'], base['mesh']) and _same(bare['head'], base['head'])
    dead = device_back(ctx, np.full((2, 20, 30), np.nan), None, np.zeros((2, 20, 30)), fill=0xA5, box=8)
    assert all(np.all(np.isnan(dead[k])) for k in ('map', 'rms', 'applied')) and np.all(dead['head'] == [2, 0, 12, 0])


def test_bad_arguments_are_refused_and_leave_the_outputs(api):
    ctx = _ctx(api, 'mixed')
    image = np.random.default_rng(6).normal(size=(2, 50, 70))
    cases = [dict(nl=0), dict(nl=-1), dict(ny=0), dict(nx=0), dict(ny=16385), dict(nx=16385), dict(nl=1 << 14, ny=64, nx=65),
             dict(nl=1 << 27, ny=1, nx=1), dict(box=7), dict(box=65), dict(box=0), dict(box=-8), dict(filter=0),
             dict(filter=2), dict(filter=4), dict(filter=7), dict(filter=-1), dict(kappa=np.nan), dict(kappa=np.inf),
             dict(kappa=0.999), dict(kappa=100.5), dict(kappa=-3.0), dict(max_clip=-1), dict(max_clip=17),
             dict(min_frac=0.0), dict(min_frac=-0.5), dict(min_frac=1.0001), dict(min_frac=np.nan), dict(min_frac=np.inf),
             dict(image=None), dict(mesh=None), dict(head=None), dict(apply=None), dict(applied=None)]
    for kw in cases:
        raw_back(ctx, image, np.ones_like(image), image, expect_rc=-1, override=kw)
        assert b'frame_background' in ctx.lib.mpsfr_last_error(), kw
    raw_back(ctx, image, None, None, expect_rc=-1, override=dict(applied=np.zeros(image.size)))
    raw_back(ctx, image, None, image, expect_rc=-1, override=dict(applied=image))         # applied_out == image
    # the bounds themselves are legal
    for kw in (dict(box=8), dict(box=64), dict(kappa=1.0), dict(kappa=100.0), dict(max_clip=0), dict(max_clip=16),
               dict(min_frac=1.0), dict(min_frac=1e-300)):
        assert raw_back(ctx, image, None, image, **kw)['rc'] == 0


# ---- 5. the chain on device buffers
TOL, MAX_ITER = 1e-10, 100


@pytest.mark.parametrize('prec', PRECS)
def test_the_chain_on_device_buffers(api, ctx, prec):
    """fit -> background of the residual -> subtract -> fit, queued on device buffers without a synchronisation, against
    the same chain on host pointers bit for bit and, stage by stage, against the references on the inputs the chain
    itself handed on: the fluxes within frame_fit_ref's solver bounds, the mesh bit for bit."""
    import torch
    import frame_fit_ref as R
    s = B.sky_scene()
    frame, psf, origin, shift, index, n = s['image'], s['psf'], s['origin'], s['shift'], s['index'], s['n']
    ny, nx = frame.shape
    par = {k: v for k, v in B.SKY_PAR.items() if k != 'passes'}
    fitkw = dict(shift=shift, psf_index=index, radius=B.SKY_RADIUS, max_iter=MAX_ITER, tol=TOL)
    # host pointers
    rows0, head0, resid = ctx.fit_frame_psf(frame, psf, origin, return_residual=True, **fitkw)
    bmap, _, mesh, bhead, applied = ctx.frame_background(resid, apply_to=frame, return_rms=False, **par)
    rows1, head1 = ctx.fit_frame_psf(applied, psf, origin, **fitkw)
    # device buffers
    dev = torch.device('cuda:0')
    tfr, tps, tor, tsh, tix = (_to_dev(torch, a) for a in (frame, psf, origin, shift, index))
    trow, thead = torch.empty((n, 8), dtype=torch.float64, device=dev), torch.empty(8, dtype=torch.float64, device=dev)
    tres, tnext = torch.empty_like(tfr), torch.empty_like(tfr)
    my, mx = B.mesh_shape(ny, nx, par['box'])
    tmesh, tbh = torch.empty((my, mx, 8), dtype=torch.float64, device=dev), torch.empty(4, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    kw = dict(shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr(), radius=B.SKY_RADIUS, max_iter=MAX_ITER, tol=TOL)
    ctx.fit_frame_psf_device(ny, nx, tfr.data_ptr(), n, 1, tps.data_ptr(), tor.data_ptr(), trow.data_ptr(), thead.data_ptr(),
                             resid_ptr=tres.data_ptr(), **kw)
    ctx.frame_background_device(1, ny, nx, tres.data_ptr(), tmesh.data_ptr(), tbh.data_ptr(), apply_to_ptr=tfr.data_ptr(),
                                applied_ptr=tnext.data_ptr(), **par)
    ctx.fit_frame_psf_device(ny, nx, tnext.data_ptr(), n, 1, tps.data_ptr(), tor.data_ptr(), trow.data_ptr(),
                             thead.data_ptr(), **kw)
    ctx.sync()
    assert _same(tnext.cpu().numpy(), applied) and _same(tmesh.cpu().numpy(), mesh) and _same(tbh.cpu().numpy(), bhead)
    assert _same(trow.cpu().numpy(), rows1) and _same(thead.cpu().numpy(), head1)
    # the references, stage by stage
    for image, rows, head in ((frame, rows0, head0), (applied, rows1, head1)):
        ref = R.solve(image, None, psf, index, origin, shift, B.SKY_RADIUS, True)
        b = R.bounds(ref, TOL, MAX_ITER)
        err = np.abs(rows[:, 0] - ref['F']) * np.sqrt(ref['dg'][:n])
        print('flux error / bound %.3g' % (err.max() / b['y']))
        assert head[7] == 0 and np.all(rows[:, 7] == 0) and np.all(err <= b['y'])
    want = B.background(resid, apply_to=frame, **par)
    assert _same(mesh, want['mesh'][0]) and _same(bhead, want['head'][0])
    assert np.all(np.abs(applied - want['applied']) <= want['map_bound'])
    # ... and what the loop is for: one pass of it already beats the constant by far
    def rms(F):
        return float(np.sqrt(np.mean((F - s['flux']) ** 2)))
    print('rms flux error: constant b %.2f, after one background pass %.2f' % (rms(rows0[:, 0]), rms(rows1[:, 0])))
    assert rms(rows1[:, 0]) < 0.1 * rms(rows0[:, 0])


@pytest.mark.parametrize('prec', PRECS)
def test_fit_crowded_stars_with_sky_meets_the_reference_loop(api, prec):
    """psfrec.fit_crowded_stars(sky=...) on the scene of the host test: the same two assertions as on the references."""
    s = B.sky_scene()
    kw = dict(psf_index=s['index'], radius=B.SKY_RADIUS, pixscale=api.grid_pixscale(128), precision=prec)

    def rms(fit):
        return float(np.sqrt(np.mean((np.asarray(fit['scale']) - s['flux']) ** 2)))
    flat = rms(api.fit_crowded_stars(s['flat'], s['psf'], s['pos'], **kw)[0])
    const = rms(api.fit_crowded_stars(s['image'], s['psf'], s['pos'], **kw)[0])
    fit, origin, sky = api.fit_crowded_stars(s['image'], s['psf'], s['pos'], sky=dict(B.SKY_PAR), return_sky=True, **kw)
    print('rms flux error: flat %.3f, constant b %.3f, sky loop %.3f (%.3f x flat)' % (flat, const, rms(fit), rms(fit) / flat))
    assert rms(fit) < const and rms(fit) <= 1.5 * flat and fit.meta['sky_passes'] == B.SKY_PAR['passes']
    assert np.sqrt(np.mean((sky - s['sky']) ** 2)) < 0.2
    record_margin('background', sky_loop_over_flat=rms(fit) / flat)


# ---- 6. profiling
def test_timed_under_the_profiling_id_of_the_fit(api):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    s = B.scene()
    ctx.set_option('profile', 1)
    ctx.profile_reset()
    ctx.frame_background(s['image'], s['var'])
    prof = ctx.profile()
    assert prof['fit'][1] == 1 and prof['fit'][0] > 0
    assert all(v[1] == 0 for k, v in prof.items() if k != 'fit'), prof
    ctx.close()
