"""GPU: crowded-field photometry of cubes (mpsfr_fit_cube_psf; cube_fit.hip).

The contract is bit equality: layer l of the cube call -- rows, head, residual -- is what mpsfr_fit_frame_psf returns on
the contiguous inputs of that layer, whatever layer_batch is, in both precision modes, on host and device pointers.
1. bit equality on the shared cube of cube_fit_cases.py (5 layers; batches of 0, 1, 2 and 5), with and without var, the
   background, layer_shift and scale0.
2. the per-layer stop: the iteration counts differ between layers; the NaN layer and the masked star.
3. independent of the frame call: a layer with a non-zero layer_shift against the NumPy yardstick within its bounds.
4. reproducibility, mixed = f64, device = host pointers, and the small shapes (one layer, one star on a 1 x 2 frame, a
   star across a tile corner, a tile list longer than 256).
5. the device form's range rule per layer; max_iter = 1.
6. refusals: every MPSFR_E_INVALID, outputs untouched; the profiling id.
"""
import ctypes as C

import numpy as np
import pytest

import cube_fit_cases as K
import frame_fit_ref as F
from conftest import record_margin

pytestmark = pytest.mark.gpu

PRECS = ['mixed', 'f64']
NS = 40
TOL, MAX_ITER = 1e-10, 100
EPS = F.EPS


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
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _cube_fit(ctx, c, with_var=True, with_layer_shift=True, scale0=None, **kw):
    return ctx.fit_cube_psf(c['cube'], c['psf'], c['origin'], var=c['var'] if with_var else None, shift=c['shift'],
                            layer_shift=c['layer_shift'] if with_layer_shift else None, psf_index=c['index'],
                            scale0=scale0, return_residual=True, **kw)


def _frames(ctx, c, with_var=True, with_layer_shift=True, scale0=None, **kw):
    """The loop a user writes without the cube call: fit_frame_psf on the contiguous inputs of every layer."""
    out = []
    for l in range(c['cube'].shape[0]):
        use = with_layer_shift and c['layer_shift'] is not None
        image, psf, origin, a = K.layer_call(c, l, with_var, use, scale0)
        out.append(ctx.fit_frame_psf(image, psf, origin, return_residual=True, **a, **kw))
    return [np.stack([o[i] for o in out]) for i in range(3)]


_LOOP = {}


def _loop(ctx, prec, with_var=True, background=True, with_layer_shift=True, start=False):
    """The frame calls of the shared cube, once per case and precision."""
    key = (prec, with_var, background, with_layer_shift, start)
    if key not in _LOOP:
        c = K.cube()
        _LOOP[key] = _frames(ctx, c, with_var, with_layer_shift, _start(c) if start else None, background=background)
    return _LOOP[key]


def _start(c):
    """A start per layer and star: three quarters of the truth."""
    return 0.75 * c['flux']


def _equal(got, want, tag):
    for name, g, w in zip(('rows', 'head', 'residual'), got, want):
        assert g.shape == w.shape, (tag, name)
        for l in range(len(w)):
            assert _same(g[l], w[l]), (tag, name, 'layer %d' % l)


# ---- 1. bit equality
@pytest.mark.parametrize('with_var,background,with_layer_shift,start',
                         [(True, True, True, False), (False, True, True, False), (True, False, True, False),
                          (True, True, False, False), (True, True, True, True), (False, False, False, True)])
@pytest.mark.parametrize('prec', PRECS)
def test_layers_equal_the_frame_calls_bit_for_bit(ctx, prec, with_var, background, with_layer_shift, start):
    c = K.cube()
    want = _loop(ctx, prec, with_var, background, with_layer_shift, start)
    assert want[0].shape == (K.NL, c['n'], 8) and want[1].shape == (K.NL, 8) and want[2].shape == (K.NL,) + F.FRAME
    for batch in (0, 1, 2, 5):
        got = _cube_fit(ctx, c, with_var, with_layer_shift, _start(c) if start else None, background=background,
                        layer_batch=batch)
        _equal(got, want, 'batch %d' % batch)


# ---- 2. the per-layer stop and the masks
@pytest.mark.parametrize('prec', PRECS)
def test_iteration_counts_differ_between_layers(ctx, prec):
    rows, head, resid = _cube_fit(ctx, K.cube(), layer_batch=0)
    counts = head[K.FITTED, 4]
    print('cube fit %s: iterations per layer %s' % (prec, head[:, 4].astype(int).tolist()))
    assert np.all(head[K.FITTED, 7] == 0) and np.all(counts >= 2) and np.all(counts < MAX_ITER)
    assert len(set(counts)) > 1, counts
    print('the yardstick: %s' % [F.pcg(K.reference(l), TOL, MAX_ITER)[1] for l in K.FITTED])


@pytest.mark.parametrize('prec', PRECS)
def test_nan_layer_and_masked_star(ctx, prec):
    c = K.cube()
    rows, head, resid = _cube_fit(ctx, c, layer_batch=2)
    l = K.NAN_LAYER
    assert head[l, 7] == 2 and head[l, 6] == 0 and head[l, 4] == 0 and not head[l, :3].any()
    assert set(rows[l, :, 7]) == {1.0, 2.0} and rows[l, c['off'], 7] == 1 and not rows[l, :, :7].any()
    assert _same(resid[l], c['cube'][l]) and np.all(np.isnan(resid[l]))
    # the star whose disc is masked in one layer: left out there, fitted in every other fitted layer
    assert rows[K.MASK_LAYER, K.MASKED, 7] == 2 and not rows[K.MASK_LAYER, K.MASKED, :7].any()
    others = [m for m in K.FITTED if m != K.MASK_LAYER]
    assert np.all(rows[others, K.MASKED, 7] == 0) and np.all(rows[others, K.MASKED, 0] > 0)
    for m in K.FITTED:
        ref = K.reference(m)
        np.testing.assert_array_equal(rows[m, :, 7], ref['status'])
        assert (head[m, 3], head[m, 6], head[m, 7]) == (ref['nomega'], ref['nacc'], 0)
    # the other layers do not see the NaN layer: the same cube with that layer finite gives them the same bits
    d = dict(c, cube=c['cube'].copy())
    d['cube'][l] = c['cube'][0]
    r2, h2, d2 = _cube_fit(ctx, d, layer_batch=2)
    for m in K.FITTED:
        assert _same(r2[m], rows[m]) and _same(h2[m], head[m]) and _same(d2[m], resid[m]), m
    assert h2[l, 7] == 0


# ---- 3. independent of the frame call
@pytest.mark.parametrize('prec', PRECS)
def test_a_shifted_layer_agrees_with_numpy_within_the_bounds(ctx, prec):
    """Layer 2 (layer_shift (0.22, -0.14) px) against frame_fit_ref.solve at the summed shifts: y in the 2-norm, N_kk,
    the overlap and chi2 within frame_fit_ref.bounds, the quantities and bounds of the frame fit's own parity test."""
    c = K.cube()
    l = 2
    assert np.all(c['layer_shift'][l] != 0)
    ref = K.reference(l)
    b = F.bounds(ref, TOL, MAX_ITER)
    rows, head, resid = _cube_fit(ctx, c, max_iter=MAX_ITER, tol=TOL)
    rows, head = rows[l], head[l]
    acc = ref['acc']
    np.testing.assert_array_equal(rows[:, 7], ref['status'])
    np.testing.assert_array_equal(rows[:, 5], ref['ndisc'])
    assert (head[3], head[6], head[7]) == (ref['nomega'], ref['nacc'], 0) and 1 <= head[4] <= MAX_ITER
    x = np.concatenate([rows[acc, 0], [head[0]]])
    dg = ref['dg'][:len(acc)]
    ratios = dict(y=float(np.linalg.norm((x - ref['x']) * np.sqrt(ref['dg']))) / b['y'],
                  nkk=float(np.max(np.abs(rows[acc, 6] - ref['nkk'][acc]) / ref['nkk'][acc])) / b['nkk_rel'],
                  overlap=float(np.max(np.abs(rows[acc, 4] - ref['overlap'][acc]) / b['overlap'])),
                  chi2=abs(head[2] - ref['chi2']) / b['chi2'])
    print('cube fit %s layer %d: error / bound %s, %d iterations' %
          (prec, l, ', '.join('%s %.2e' % kv for kv in sorted(ratios.items())), head[4]))
    record_margin('cube_fit', **{'%s_%s' % (k, prec): v for k, v in ratios.items()})
    assert np.all(np.abs(rows[acc, 0] - ref['F'][acc]) <= b['y'] / np.sqrt(dg))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
    # the shift matters: the same layer fitted without its offset is another result
    plain = _cube_fit(ctx, c, with_layer_shift=False)[0][l]
    assert not _same(plain[acc, 0], rows[acc, 0])


# ---- 4. bits and small shapes
@pytest.mark.parametrize('prec', PRECS)
def test_same_call_twice_gives_the_same_bits(ctx, prec):
    a = _cube_fit(ctx, K.cube(), layer_batch=2)
    b = _cube_fit(ctx, K.cube(), layer_batch=2)
    _equal(b, a, 'twice')


def test_mixed_gives_the_bits_of_f64(api):
    a = _cube_fit(_ctx(api, 'mixed'), K.cube())
    b = _cube_fit(_ctx(api, 'f64'), K.cube())
    _equal(a, b, 'mixed against f64')


def _to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda:0'))


def _device_call(ctx, torch, c, shift, layer_shift, layer_batch, with_resid=True):
    """The device form on the cube dict c; returns (rows, head, residual) as host arrays."""
    nl, ny, nx = c['cube'].shape
    n = c['n']
    t = {k: _to_dev(torch, c[k]) for k in ('cube', 'var', 'psf', 'index', 'origin')}
    tshift, tls = _to_dev(torch, shift), None if layer_shift is None else _to_dev(torch, layer_shift)
    dev = t['psf'].device
    trow = torch.full((nl, n, 8), -1.0, dtype=torch.float64, device=dev)
    thead = torch.full((nl, 8), -1.0, dtype=torch.float64, device=dev)
    tres = torch.full((nl, ny, nx), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_cube_psf_device(nl, ny, nx, t['cube'].data_ptr(), n, c['psf'].shape[0], t['psf'].data_ptr(),
                            t['origin'].data_ptr(), trow.data_ptr(), thead.data_ptr(), var_ptr=t['var'].data_ptr(),
                            shift_ptr=tshift.data_ptr(), layer_shift_ptr=None if tls is None else tls.data_ptr(),
                            psf_index_ptr=t['index'].data_ptr(), resid_ptr=tres.data_ptr() if with_resid else None,
                            layer_batch=layer_batch)
    ctx.sync()
    return trow.cpu().numpy(), thead.cpu().numpy(), tres.cpu().numpy()


@pytest.mark.parametrize('prec', PRECS)
def test_device_pointers_give_the_bits_of_the_host_form(ctx, prec):
    import torch
    c = K.cube()
    want = _loop(ctx, prec)
    for batch in (0, 2):
        got = _device_call(ctx, torch, c, c['shift'], c['layer_shift'], batch)
        _equal(got, want, 'device, batch %d' % batch)
    # without the residual cube the rows and heads are the same bits, and the residual buffer is not touched
    rows, head, res = _device_call(ctx, torch, c, c['shift'], c['layer_shift'], 2, with_resid=False)
    assert _same(rows, want[0]) and _same(head, want[1]) and np.all(res == -1.0)


@pytest.mark.parametrize('prec', PRECS)
def test_one_layer_equals_the_frame_call(ctx, prec):
    c = K.cube()
    one = dict(c, cube=c['cube'][2:3], var=c['var'][2:3], psf=np.ascontiguousarray(c['psf'][:, 2:3]),
               layer_shift=c['layer_shift'][2:3])
    got = _cube_fit(ctx, one)
    want = _loop(ctx, prec)
    for g, w in zip(got, want):
        assert g.shape[0] == 1 and _same(g[0], w[2])


@pytest.mark.parametrize('prec', PRECS)
def test_one_star_on_a_one_by_two_frame(ctx, prec):
    psf = np.ascontiguousarray(np.broadcast_to(F.Y.models()[:1, None], (1, 3, NS, NS)))
    c = dict(cube=np.array([[[3.5, 2.5]], [[1.5, np.nan]], [[-2.0, 7.0]]]), var=None, psf=psf, index=None,
             origin=np.array([[-20, -20]], dtype=np.int32), shift=np.zeros((1, 2)),
             layer_shift=np.array([[0.0, 0.0], [0.0, 0.25], [0.0, 0.5]]), n=1)
    want = _frames(ctx, c, with_var=False, background=False, radius=1.0)
    for batch in (0, 1, 2):
        got = ctx.fit_cube_psf(c['cube'], psf, c['origin'], shift=c['shift'], layer_shift=c['layer_shift'],
                               background=False, radius=1.0, layer_batch=batch, return_residual=True)
        _equal(got, want, 'batch %d' % batch)
    rows, head, _ = want
    assert head[0, 7] == 0 and head[0, 3] == 2 and head[1, 7] == 2 and head[1, 3] == 1 and head[2, 7] == 0
    assert rows[0, 0, 7] == 0 and rows[1, 0, 7] == 2


@pytest.mark.parametrize('prec', PRECS)
def test_star_across_a_tile_corner(ctx, prec):
    rng = np.random.default_rng(4)
    base = F.Y.models()
    shape, nl = (33, 31), 2
    pos = np.array([[31.6, 29.8], [12.3, 8.9], [30.2, 3.1]])
    origin = (np.rint(pos) - NS // 2).astype(np.int32)
    shift = pos - (origin + NS // 2)
    index = np.array([0, 1, 3], dtype=np.int32)
    psf = np.stack([np.roll(base, l, axis=0) for l in range(nl)], axis=1)
    ls = np.array([[0.0, 0.0], [0.3, 0.4]])
    data, var = np.empty((nl,) + shape), np.empty((nl,) + shape)
    for l in range(nl):
        model, _, _ = F.Y.render(None, np.ascontiguousarray(psf[:, l]), index, origin, shift + ls[l],
                                 [900.0 + 100 * l, 400.0, 1500.0], shape=shape)
        var[l] = 1.0 + model / 4.0
        data[l] = model + 2.0 + rng.normal(size=shape) * np.sqrt(var[l])
        data[l][rng.uniform(size=shape) < 0.02] = np.nan
    c = dict(cube=data, var=var, psf=psf, index=index, origin=origin, shift=shift, layer_shift=ls, n=3)
    want = _frames(ctx, c)
    _equal(_cube_fit(ctx, c), want, 'corner')
    assert np.all(want[1][:, 7] == 0) and np.all(want[0][:, :, 7] == 0)
    assert np.array_equal(np.isnan(want[2]), np.isnan(data))


@pytest.mark.parametrize('prec', PRECS)
def test_tile_list_longer_than_the_sort_chunk(ctx, prec):
    c = K.lattice()
    assert K.longest_tile_list(c['origin'], c['cube'].shape[1:]) > 256 and c['cube'].shape[0] == 2
    want = _frames(ctx, c, radius=3.0, max_iter=30)
    for batch in (0, 1):
        got = _cube_fit(ctx, c, radius=3.0, max_iter=30, layer_batch=batch)
        _equal(got, want, 'lattice, batch %d' % batch)
    assert np.all(want[0][:, :, 7] == 0) and np.all(want[1][:, 6] == 289)


# ---- 5. the device form's range rule, the cap
@pytest.mark.parametrize('prec', PRECS)
def test_device_form_leaves_a_star_out_in_the_layer_where_its_shift_leaves_the_domain(ctx, prec):
    import torch
    c = K.cube()
    n = c['n']
    shift = c['shift'].copy()
    shift[[4, 9], 0] = 7.8                           # inside alone; beyond 8 px with the offset of layers 2 .. 4 (0.22 l)
    ls = c['layer_shift'].copy()
    out_of = [l for l in range(K.NL) if 7.8 + ls[l, 0] > 8.0]
    assert out_of == [2, 3, 4]
    rows, head, resid = _device_call(ctx, torch, c, shift, ls, 2)
    t = {k: _to_dev(torch, c[k]) for k in ('index', 'origin')}
    for l in range(K.NL):
        # the frame call in the device form on the contiguous layer at the summed shifts
        timg, tvar = _to_dev(torch, c['cube'][l]), _to_dev(torch, c['var'][l])
        tpsf, tsh = _to_dev(torch, c['psf'][:, l]), _to_dev(torch, shift + ls[l])
        trow = torch.full((n, 8), -1.0, dtype=torch.float64, device=timg.device)
        thead = torch.full((8,), -1.0, dtype=torch.float64, device=timg.device)
        tres = torch.full(F.FRAME, -1.0, dtype=torch.float64, device=timg.device)
        torch.cuda.synchronize()
        ctx.fit_frame_psf_device(F.FRAME[0], F.FRAME[1], timg.data_ptr(), n, 4, tpsf.data_ptr(), t['origin'].data_ptr(),
                                 trow.data_ptr(), thead.data_ptr(), var_ptr=tvar.data_ptr(), shift_ptr=tsh.data_ptr(),
                                 psf_index_ptr=t['index'].data_ptr(), resid_ptr=tres.data_ptr())
        ctx.sync()
        assert _same(rows[l], trow.cpu().numpy()) and _same(head[l], thead.cpu().numpy()), l
        assert _same(resid[l], tres.cpu().numpy()), l
        if l != K.NAN_LAYER:
            want = 2.0 if l in out_of else 0.0
            assert np.all(rows[l, [4, 9], 7] == want), l
            if l in out_of:
                assert not rows[l, [4, 9], :7].any()


@pytest.mark.parametrize('prec', PRECS)
def test_one_iteration_ends_with_status_one(ctx, prec):
    c = K.cube()
    rows, head, resid = _cube_fit(ctx, c, max_iter=1, layer_batch=2)
    assert np.all(head[K.FITTED, 7] == 1) and np.all(head[K.FITTED, 4] == 1) and head[K.NAN_LAYER, 7] == 2
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(head))
    for l in K.FITTED:
        acc = rows[l, :, 7] == 0
        assert acc.sum() == head[l, 6]
        image, psf, origin, a = K.layer_call(c, l)
        want = ctx.render_stars(psf, origin[acc], rows[l, acc, 0], shift=a['shift'][acc], psf_index=c['index'][acc],
                                image=image, subtract=True)
        assert _same(resid[l], want), l
    _equal((rows, head, resid), _frames(ctx, c, max_iter=1), 'one iteration')


# ---- 6. refusals and housekeeping
def _raw(ctx, c, **override):
    """The C call on host pointers with sentinel outputs; returns (rc, rows, head, resid)."""
    n = c['n']
    nl, ny, nx = c['cube'].shape
    a = dict(nl=nl, ny=ny, nx=nx, cube=c['cube'], var=c['var'], nstar=n, npsf=c['psf'].shape[0], psf=c['psf'],
             index=c['index'], origin=c['origin'], shift=c['shift'], layer_shift=c['layer_shift'], scale0=None,
             radius=8.0, flags=1, max_iter=100, tol=1e-10, layer_batch=0, rows=np.full((nl, n, 8), -7.0),
             head=np.full((nl, 8), -7.0), resid=np.full((nl, ny, nx), -7.0), on_device=0)
    a.update(override)

    def p(v):
        return None if v is None else C.c_void_p(np.ascontiguousarray(v).ctypes.data)
    keep = {k: np.ascontiguousarray(a[k]) if a[k] is not None else None
            for k in ('cube', 'var', 'psf', 'index', 'origin', 'shift', 'layer_shift', 'scale0')}
    rc = ctx.lib.mpsfr_fit_cube_psf(ctx._h, a['nl'], a['ny'], a['nx'], p(keep['cube']), p(keep['var']), a['nstar'],
                                    a['npsf'], p(keep['psf']), p(keep['index']), p(keep['origin']), p(keep['shift']),
                                    p(keep['layer_shift']), p(keep['scale0']), float(a['radius']), a['flags'],
                                    a['max_iter'], float(a['tol']), a['layer_batch'], p(a['rows']), p(a['head']),
                                    p(a['resid']), a['on_device'])
    return rc, a['rows'], a['head'], a['resid']


def test_bad_arguments_are_refused_and_leave_the_outputs(api):
    ctx = _ctx(api, 'mixed')
    c = K.cube()
    n, nl = c['n'], K.NL
    far, nan, inf = c['shift'].copy(), c['shift'].copy(), np.zeros((nl, n))
    far[2, 1], nan[5, 0], inf[3, 1] = 8.25, np.nan, np.inf
    bad_index, bad_origin, neg_index = c['index'].copy(), c['origin'].copy(), c['index'].copy()
    bad_index[4], bad_origin[0, 0], neg_index[0] = 4, (1 << 30) + 1, -1
    ls_nan, ls_inf, ls_far = c['layer_shift'].copy(), c['layer_shift'].copy(), c['layer_shift'].copy()
    ls_nan[1, 0], ls_inf[4, 1], ls_far[2, 0] = np.nan, -np.inf, 8.6          # (the shifts of the scene: within 0.5)
    edge = c['shift'].copy()
    edge[7, 1] = -7.9                                                        # legal alone; -8.18 in layer 4
    cases = [dict(nl=0), dict(nl=-1), dict(nl=4097), dict(layer_batch=-1), dict(layer_batch=-(1 << 31)),
             dict(ny=0), dict(nx=0), dict(ny=-1), dict(ny=16385), dict(nx=16385), dict(ny=8193, nx=8192),
             dict(nstar=0), dict(nstar=-1), dict(nstar=(1 << 20) + 1), dict(npsf=0), dict(npsf=-1),
             dict(cube=None), dict(psf=None), dict(origin=None), dict(rows=None), dict(head=None),
             dict(index=None),                                                    # npsf = 4 != nstar
             dict(radius=0.999), dict(radius=20.001), dict(radius=np.nan), dict(radius=np.inf), dict(radius=-8.0),
             dict(tol=0.0), dict(tol=1.0), dict(tol=-1e-10), dict(tol=np.nan), dict(tol=np.inf),
             dict(max_iter=0), dict(max_iter=-1), dict(max_iter=1001),
             dict(flags=2), dict(flags=4), dict(flags=3), dict(flags=-1),
             dict(index=bad_index), dict(index=neg_index), dict(shift=far), dict(shift=nan), dict(origin=bad_origin),
             dict(layer_shift=ls_nan), dict(layer_shift=ls_inf), dict(layer_shift=ls_far), dict(shift=edge),
             dict(shift=None, layer_shift=np.full((nl, 2), 8.5)),
             dict(scale0=inf), dict(scale0=np.full((nl, n), np.nan))]
    for kw in cases:
        rc, rows, head, resid = _raw(ctx, c, **kw)
        assert rc == -1, kw
        assert b'fit_cube_psf' in ctx.lib.mpsfr_last_error(), kw
        assert all(np.all(out == -7.0) for out in (rows, head, resid) if out is not None), kw
    # their neighbours are legal, and var, shift, layer_shift, scale0 and resid_out are optional
    for kw in (dict(radius=1.0), dict(radius=20.0), dict(tol=0.999), dict(tol=1e-300, max_iter=2), dict(max_iter=1),
               dict(flags=0), dict(var=None), dict(shift=None), dict(layer_shift=None), dict(scale0=np.zeros((nl, n))),
               dict(resid=None), dict(layer_batch=1), dict(layer_batch=nl + 1), dict(layer_batch=(1 << 31) - 1),
               dict(shift=None, layer_shift=np.full((nl, 2), 8.0)), dict(nl=1)):
        rc, rows, head, resid = _raw(ctx, c, **kw)
        m = kw.get('nl', nl)
        assert rc == 0 and np.all(head[:m, 7] != -7.0) and np.all(rows[:m, :, 7] != -7.0), kw
        assert head[0, 6] >= 1, kw


def test_timed_under_the_profiling_id_of_the_fit(api):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    assert ctx.lib.mpsfr_profile_count() == 16 and ctx.lib.mpsfr_version() == 102
    ctx.set_option('profile', 1)
    ctx.profile_reset()
    rows, head, resid = _cube_fit(ctx, K.cube(), layer_batch=5)
    prof = ctx.profile()
    assert head[0, 7] == 0 and prof['fit'][1] == 1 and prof['fit'][0] > 0
    assert all(v[1] == 0 for k, v in prof.items() if k != 'fit'), prof
    ctx.close()
