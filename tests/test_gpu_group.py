"""GPU: friends-of-friends grouping (mpsfr_group_stars), both precisions.  Every output is an integer or a single
rounding, so everything here is compared bit for bit (assert_array_equal) with the NumPy yardstick group_ref; there is
no tolerance in this file.

1. the shared scenes: the random field with every class, the exact link cases, the chains (one oversize group each,
   along a diagonal and along cell borders), pairs across cell borders and corners, the link across a whole cell at
   crit = 16, the wide chain, the edges of the frame.
2. one star, all fillers, fillers between stars, the finder's own rows at stride 8.
3. invariances: a permuted list (the same groups as sets, labels the permuted minima), the scene moved by (48, 80) in a
   larger frame (origins move by the offset, shifts keep their bits), host = device pointers, repeated calls and calls
   between other work of the context, mixed = f64.
4. max_groups of 1, n - 1, n and n + 5; every raw call checks canaries behind each buffer.
5. positions out of range in the device form, the refusals, profiling.
6. 65 536 stars on 2048 x 2048: many workgroups hook into the same components.
7. the chain find -> fit_found_stars -> subtract_stars on 40 rendered stars with pairs and triples.
"""
import ctypes as C

import numpy as np
import pytest

import find_ref as F
import group_ref as G

pytestmark = pytest.mark.gpu

PRECS = ['mixed', 'f64']
NS = 40
SENT, ISENT, CAN = -7.25, -77, 16
FILL = G.FILLER_ORIGIN


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


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def raw_group(ctx, pos, crit, shape, max_groups=None, tables=True, expect_rc=0, override=None):
    """mpsfr_group_stars on host pointers with canaries behind every output.  Returns a dict: rc, label, groups
    (max_groups, 8), origin, shift (max_groups * 8, as written) and counts; after a refusal it asserts that every output
    is untouched."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    nstar, stride = pos.shape
    mg = nstar if max_groups is None else max_groups
    cap = max(mg, 1) if mg <= 1 << 22 else 1
    label = np.full(nstar + CAN, ISENT, dtype=np.int32)
    groups = np.full(cap * 8 + CAN, ISENT, dtype=np.int32)
    origin = np.full(cap * 2 + CAN, ISENT, dtype=np.int32)
    shift = np.full(cap * 8 + CAN, SENT)
    counts = np.full(6 + CAN, ISENT, dtype=np.int32)
    a = dict(ny=shape[0], nx=shape[1], nstar=nstar, pos=pos, stride=stride, crit=crit, max_groups=mg, label=label,
             groups=groups, origin=origin if tables else None, shift=shift if tables else None, counts=counts)
    a.update(override or {})
    rc = ctx.lib.mpsfr_group_stars(ctx._h, a['ny'], a['nx'], a['nstar'], _ptr(a['pos']), a['stride'], a['crit'],
                                   a['max_groups'], _ptr(a['label']), _ptr(a['groups']), _ptr(a['origin']),
                                   _ptr(a['shift']), _ptr(a['counts']), 0)
    assert rc == expect_rc, (rc, ctx.lib.mpsfr_last_error())
    assert np.all(label[nstar:] == ISENT) and np.all(groups[cap * 8:] == ISENT) and np.all(origin[cap * 2:] == ISENT)
    assert np.all(shift[cap * 8:] == SENT) and np.all(counts[6:] == ISENT)
    if rc != 0:
        assert np.all(label == ISENT) and np.all(groups == ISENT) and np.all(origin == ISENT)
        assert np.all(shift == SENT) and np.all(counts == ISENT)
    if not tables:
        assert np.all(origin == ISENT) and np.all(shift == SENT)
    return dict(rc=rc, label=label[:nstar], groups=groups[:cap * 8].reshape(cap, 8),
                origin=origin[:cap * 2].reshape(cap, 2), shift=shift[:cap * 8], counts=counts[:6])


def _to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda:0'))


def device_group(ctx, pos, crit, shape, max_groups=None, tables=True):
    import torch
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    nstar, stride = pos.shape
    mg = nstar if max_groups is None else max_groups
    dev = torch.device('cuda:0')
    tpos = _to_dev(torch, pos)
    tlab = torch.full((nstar + CAN,), ISENT, dtype=torch.int32, device=dev)
    tgrp = torch.full((mg * 8 + CAN,), ISENT, dtype=torch.int32, device=dev)
    tor = torch.full((mg * 2 + CAN,), ISENT, dtype=torch.int32, device=dev)
    tsh = torch.full((mg * 8 + CAN,), SENT, dtype=torch.float64, device=dev)
    tct = torch.full((6 + CAN,), ISENT, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.group_stars_device(shape[0], shape[1], nstar, tpos.data_ptr(), stride, crit, mg, tlab.data_ptr(), tgrp.data_ptr(),
                           tct.data_ptr(), origin_ptr=tor.data_ptr() if tables else None,
                           shift_ptr=tsh.data_ptr() if tables else None)
    ctx.sync()
    label, groups, origin, shift, counts = (t.cpu().numpy() for t in (tlab, tgrp, tor, tsh, tct))
    assert np.all(label[nstar:] == ISENT) and np.all(groups[mg * 8:] == ISENT) and np.all(origin[mg * 2:] == ISENT)
    assert np.all(shift[mg * 8:] == SENT) and np.all(counts[6:] == ISENT)
    if not tables:
        assert np.all(origin == ISENT) and np.all(shift == SENT)
    return dict(label=label[:nstar], groups=groups[:mg * 8].reshape(mg, 8), origin=origin[:mg * 2].reshape(mg, 2),
                shift=shift[:mg * 8], counts=counts[:6])


def assert_reference(got, ref, max_groups, tables=True):
    groups, origin, shift = G.buffers(ref, max_groups)
    np.testing.assert_array_equal(got['counts'], ref['counts'])
    np.testing.assert_array_equal(got['label'], ref['label'])
    np.testing.assert_array_equal(got['groups'], groups)
    if tables:
        np.testing.assert_array_equal(got['origin'], origin)
        assert got['shift'].tobytes() == shift.tobytes()                    # the bits, the sign of a zero included


def assert_same(a, b):
    for key in ('label', 'groups', 'origin', 'shift', 'counts'):
        assert a[key].tobytes() == b[key].tobytes(), key


# ---- 1. the scenes
@pytest.mark.parametrize('name', list(G.scenes()))
@pytest.mark.parametrize('prec', PRECS)
def test_scene_equals_the_reference(ctx, prec, name):
    pos, crit, shape, ref = G.scene_reference(name)
    got = raw_group(ctx, pos, crit, shape)
    assert_reference(got, ref, len(pos))
    n = int(ref['counts'][0])
    label, groups, origin, shift, counts = ctx.group_stars(pos, crit, shape)
    np.testing.assert_array_equal(groups, ref['groups'])
    np.testing.assert_array_equal(origin, ref['origin'])
    np.testing.assert_array_equal(shift, ref['shift'])
    assert groups.shape == (n, 8) and label.tobytes() == ref['label'].tobytes()


# ---- 2. small lists, fillers, the finder's rows
@pytest.mark.parametrize('prec', PRECS)
def test_one_star_and_fillers(ctx, prec):
    for p in ([[3.25, 4.5]], [[-1.0, 7.0]], [[9.0, 7.0]]):
        got = raw_group(ctx, p, 2.5, (9, 7), max_groups=3)
        assert_reference(got, G.group(np.array(p), 2.5, (9, 7)), 3)
        assert list(got['counts']) == [1, 1, 0, 0, 0, 0] and list(got['groups'][0]) == [1, 0, 0, 0, 0, -1, -1, -1]
    nan = np.full((5, 2), np.nan)
    nan[1, 0], nan[3, 1] = 2.0, 3.0                                    # NaN in either coordinate is a filler
    got = raw_group(ctx, nan, 2.5, (9, 7))
    assert list(got['label']) == [-1] * 5 and list(got['counts']) == [0] * 6
    assert np.all(got['groups'][:, :4] == 0) and np.all(got['groups'][:, 4:] == -1) and np.all(got['origin'] == FILL)
    assert not got['shift'].any()
    pos, crit, shape, _ = G.scene_reference('field')
    mixed = np.full((2 * len(pos) + 3, 2), np.nan)
    mixed[1:-2:2] = pos
    ref = G.group(mixed, crit, shape)
    assert list(ref['counts']) == list(G.scene_reference('field')[3]['counts'])
    assert_reference(raw_group(ctx, mixed, crit, shape), ref, len(mixed))


@pytest.mark.parametrize('prec', PRECS)
def test_the_finders_rows_at_stride_8(api, ctx, prec):
    s = F.scene()
    rows, origin, n = ctx.find_stars(s['image'], s['psf'], var=s['var'], half=3, sep=3, threshold=5.0, max_stars=128)
    full = rows.base
    assert full.shape == (128, api.NFIND) and 2 < n < 128 and np.all(np.isnan(full[n:]))
    for crit in (10.0, 16.0):
        ref = G.group(full, crit, F.FRAME)
        assert np.all(ref['label'][n:] == -1) and (crit < 16.0 or ref['counts'][0] < n)   # at 16 something is linked
        assert_reference(raw_group(ctx, full, crit, F.FRAME), ref, 128)
        assert_reference(device_group(ctx, full, crit, F.FRAME, max_groups=20), ref, 20)


# ---- 3. invariances
@pytest.mark.parametrize('prec', PRECS)
def test_a_permuted_list_gives_the_same_groups(ctx, prec):
    pos, crit, shape, ref = G.scene_reference('field')
    perm = np.random.default_rng(8).permutation(len(pos))
    got = raw_group(ctx, pos[perm], crit, shape)
    inv = np.argsort(perm)
    first = np.full(len(pos), len(pos))
    np.minimum.at(first, ref['label'], inv)
    np.testing.assert_array_equal(got['label'][inv], first[ref['label']])      # labels: the permuted minima
    np.testing.assert_array_equal(got['counts'], ref['counts'])
    sets = {frozenset(np.flatnonzero(ref['label'] == lab)) for lab in np.unique(ref['label'])}
    assert {frozenset(perm[np.flatnonzero(got['label'] == lab)]) for lab in np.unique(got['label'])} == sets
    assert_reference(got, G.group(pos[perm], crit, shape), len(pos))


@pytest.mark.parametrize('prec', PRECS)
def test_the_scene_moved_inside_a_larger_frame(ctx, prec):
    pos, crit, shape, _ = G.scene_reference('field')
    pos = np.round(pos * 2.0 ** 20) / 2.0 ** 20            # on a grid of 2^-20 pixels, adding an integer offset is exact
    off = np.array([48.0, 80.0])
    base = raw_group(ctx, pos, crit, shape)
    assert_reference(base, G.group(pos, crit, shape), len(pos))
    got = raw_group(ctx, pos + off, crit, (shape[0] + 100, shape[1] + 170))
    assert np.array_equal((pos + off) - off, pos)
    for key in ('label', 'groups', 'counts', 'shift'):
        assert got[key].tobytes() == base[key].tobytes(), key
    n = int(base['counts'][0])
    small = base['groups'][:n, 0] <= 4
    np.testing.assert_array_equal(got['origin'][:n][small], base['origin'][:n][small] + off.astype(np.int32))
    assert np.all(got['origin'][:n][~small] == FILL) and np.all(got['origin'][n:] == FILL)


@pytest.mark.parametrize('name', ['field', 'chains'])
@pytest.mark.parametrize('prec', PRECS)
def test_device_pointers_equal_host_pointers(ctx, prec, name):
    pos, crit, shape, ref = G.scene_reference(name)
    host = raw_group(ctx, pos, crit, shape)
    got = device_group(ctx, pos, crit, shape)
    assert_same(got, host)
    bare = device_group(ctx, pos, crit, shape, tables=False)
    assert bare['label'].tobytes() == host['label'].tobytes() and bare['groups'].tobytes() == host['groups'].tobytes()
    bare = raw_group(ctx, pos, crit, shape, tables=False)
    assert bare['groups'].tobytes() == host['groups'].tobytes() and bare['counts'].tobytes() == host['counts'].tobytes()


def test_mixed_equals_f64(api):
    pos, crit, shape, _ = G.scene_reference('field')
    assert_same(raw_group(_ctx(api, 'mixed'), pos, crit, shape), raw_group(_ctx(api, 'f64'), pos, crit, shape))


@pytest.mark.parametrize('prec', PRECS)
def test_a_call_does_not_depend_on_the_calls_before_it(ctx, prec):
    import render_ref as Y
    pos, crit, shape, ref = G.scene_reference('field')
    base = raw_group(ctx, pos, crit, shape)
    for _ in range(3):
        assert_same(raw_group(ctx, pos, crit, shape), base)
    # other shapes and sizes of the same call, the finder and the renderer on the same context in between
    c = G.scene_reference('chains')
    assert_reference(raw_group(ctx, c[0], c[1], c[2], max_groups=2), c[3], 2)
    s = F.scene()
    ctx.find_stars(s['image'], s['psf'], var=s['var'])
    assert_same(raw_group(ctx, pos, crit, shape), base)
    r = Y.scene()
    ctx.render_stars(r['psf'], r['origin'], r['scale'], shift=r['shift'], psf_index=r['index'], image=r['image'])
    raw_group(ctx, pos[:7], 16.0, (1000, 300))
    assert_same(raw_group(ctx, pos, crit, shape), base)
    assert_reference(base, ref, len(pos))


# ---- 4. max_groups
@pytest.mark.parametrize('name', ['field', 'borders'])
@pytest.mark.parametrize('prec', PRECS)
def test_max_groups_below_at_and_above_the_count(ctx, prec, name):
    pos, crit, shape, ref = G.scene_reference(name)
    n = int(ref['counts'][0])
    off = np.concatenate([[0], np.cumsum(ref['counts'][1:])])
    for mg in (1, n - 1, n, n + 5, int(off[1]) + 1, int(off[2]) - 1):
        if mg >= 1:
            assert_reference(raw_group(ctx, pos, crit, shape, max_groups=mg), ref, mg)
    assert_reference(device_group(ctx, pos, crit, shape, max_groups=n + 5), ref, n + 5)
    # filler rows are legal for the frame calls: an all-NaN stamp
    got = raw_group(ctx, pos, crit, shape, max_groups=n + 5)
    assert np.all(np.isnan(ctx.cut_stamps(np.zeros(shape), got['origin'][n:])))


# ---- 5. out of range, refusals, profiling
@pytest.mark.parametrize('prec', PRECS)
def test_positions_out_of_range_in_the_device_form(ctx, prec):
    pos, crit, shape, _ = G.scene_reference('edges')
    ny, nx = shape
    bad = np.array([[np.nextafter(-1.0, -2.0), 3.0], [3.0, np.nextafter(float(nx), 1e9)], [np.inf, 3.0], [3.0, -np.inf],
                    [np.nan, np.inf], [1e300, 1e300], [float(ny) + 1.0, 2.0]])
    mixed = np.concatenate([bad[:3], pos, bad[3:]])
    ref = G.group(mixed, crit, shape, device=True)
    assert list(ref['label'][:3]) == [-2, -2, -2] and list(ref['label'][-4:]) == [-2, -1, -2, -2]
    assert_reference(device_group(ctx, mixed, crit, shape), ref, len(mixed))
    raw_group(ctx, mixed, crit, shape, expect_rc=-1)                      # the host form refuses them
    for k in (0, 1, 2, 3, 5, 6):
        raw_group(ctx, np.concatenate([pos, bad[k:k + 1]]), crit, shape, expect_rc=-1)
    assert raw_group(ctx, np.concatenate([pos, bad[4:5]]), crit, shape)['label'][-1] == -1


def test_bad_arguments_are_refused_and_leave_the_outputs(api):
    ctx = _ctx(api, 'mixed')
    pos, crit, shape, _ = G.scene_reference('edges')
    cases = [dict(ny=0), dict(nx=0), dict(ny=-1), dict(ny=16385), dict(nx=16385), dict(ny=8193, nx=8192),
             dict(nstar=0), dict(nstar=-1), dict(nstar=(1 << 24) + 1), dict(stride=1), dict(stride=0), dict(stride=-2),
             dict(crit=0.0), dict(crit=-2.5), dict(crit=np.nan), dict(crit=np.inf), dict(crit=-np.inf),
             dict(crit=float(np.nextafter(16.0, 17.0))), dict(max_groups=0), dict(max_groups=-1),
             dict(pos=None), dict(label=None), dict(groups=None), dict(counts=None), dict(origin=None), dict(shift=None)]
    for kw in cases:
        raw_group(ctx, pos, crit, shape, expect_rc=-1, override=kw)
        assert b'group_stars' in ctx.lib.mpsfr_last_error(), kw
    # their neighbours are legal
    assert raw_group(ctx, pos, 16.0, shape)['rc'] == 0 and raw_group(ctx, pos, 5e-324, shape)['rc'] == 0
    assert raw_group(ctx, pos, crit, shape, max_groups=1)['rc'] == 0
    assert raw_group(ctx, pos, crit, shape, tables=False)['rc'] == 0


def test_timed_under_the_profiling_id_of_the_fit(api):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    pos, crit, shape, ref = G.scene_reference('field')
    assert ctx.lib.mpsfr_profile_count() == 16 and ctx.lib.mpsfr_version() == 102
    ctx.set_option('profile', 1)
    ctx.profile_reset()
    counts = ctx.group_stars(pos, crit, shape)[4]
    prof = ctx.profile()
    assert list(counts) == list(ref['counts']) and prof['fit'][1] == 1 and prof['fit'][0] > 0
    ctx.group_stars(pos, 16.0, shape, max_groups=3)
    prof = ctx.profile()
    assert prof['fit'][1] == 2
    assert all(v[1] == 0 for k, v in prof.items() if k != 'fit'), prof
    ctx.close()


# ---- 6. a large field
def test_large_field_equals_the_reference(api):
    pos, crit, shape, ref = G.large_field()
    assert ref['counts'][5] > 50 and ref['groups'][:, 0].max() > 6
    ctx = _ctx(api, 'mixed')
    assert_reference(raw_group(ctx, pos, crit, shape), ref, len(pos))
    assert_reference(device_group(ctx, pos, crit, shape, max_groups=int(ref['counts'][0])), ref, int(ref['counts'][0]))


# ---- 7. the chain: find -> group, cut and fit -> subtract
@pytest.mark.parametrize('prec', PRECS)
def test_find_fit_found_stars_subtract(api, ctx, prec, monkeypatch):
    monkeypatch.setattr(api.psfrec, 'get_context', lambda *a, **k: ctx)
    pos, flux, blend = G.blend_field()
    psf = F.model()
    index = np.zeros(len(pos), dtype=np.int32)
    frame = ctx.render_stars(psf[None], (np.rint(pos) - NS // 2).astype(np.int32), flux, shift=pos - np.rint(pos),
                             psf_index=index, image=G.blend_background())
    var = np.ones_like(frame)
    ps = 0.2
    found = api.find_stars(frame, psf, var, pixscale=ps, **G.BLEND_FIND)
    assert len(found) == 40
    fp = np.asarray(found['position'])
    near = np.argmin(((fp[:, None] - pos[None]) ** 2).sum(-1), axis=1)
    assert sorted(near) == list(range(40))
    fit, origin = api.fit_found_stars(frame, psf, found, var=var, crit=G.BLEND_CRIT, pixscale=ps)
    assert len(fit) == 40 and origin.shape == (23, 2) and not np.any(fit['crowded'])
    np.testing.assert_array_equal(fit['nsrc'], blend[near])
    assert np.all(np.asarray(fit['status']) == 0)
    where = origin[np.asarray(fit['group'])] + NS // 2 + np.asarray(fit['shift']) / ps
    assert np.abs(where - pos[near]).max() < 0.5
    blended = blend[near] > 1
    z = np.abs(np.asarray(fit['flux']) - flux[near]) / np.asarray(fit['err_flux'])
    print('chain %s: worst flux error of a blended star %.2f of its error, of a single %.2f' %
          (prec, z[blended].max(), z[~blended].max()))
    assert blended.sum() == 30 and np.all(z[blended] < 5.0)
    residual, status = api.subtract_stars(frame, psf[None], origin, fit, psf_index=np.zeros(23, dtype=np.int32),
                                          pixscale=ps)
    assert np.all(status == 0)
    assert len(api.find_stars(residual, psf, var, pixscale=ps, **G.BLEND_FIND)) == 0
    # the same stars one by one: a blended star's flux takes in its neighbours
    stamps, vstamps, o1 = api.cut_star_stamps(frame, fp, var, pixscale=ps)
    one = api.fit_stars_with_psf(stamps, psf[None], var=vstamps, psf_index=index, shift=found['shift'], pixscale=ps)
    z1 = np.abs(np.asarray(one['flux']) - flux[near]) / np.asarray(one['err_flux'])
    print('chain %s: fitted alone, %d of %d blended stars miss by more than 5 of their errors' %
          (prec, int(np.sum(z1[blended] > 5.0)), int(blended.sum())))
    assert np.sum(z1[blended] > 5.0) >= 15
