"""Host: friends-of-friends grouping (mpsfr_group_stars) without a GPU.

1. the yardstick (group_ref) against answers written out by hand: the exact link cases, pairs across cell borders and
   corners, the link across a whole cell at crit = 16, the wide chain, the edges of the frame; the class conditions of the
   random field; candidate pairs from the grid equal all pairs; the layout of shift_out at the pitch of each class.
2. what Context.group_stars and its device form hand to C, against the recording stub of test_render_host.py, and what
   the host form makes of the answer (a stub that answers with the reference's tables): rows cut at the count, the
   shifts one group per row, truncation at max_groups.
3. every refusal, before any library call.
4. psfrec.group_stars and psfrec.fit_found_stars against the answering stub: input order restored, the `group` column
   indexes `origin`, crowded rows at status 2, one cut and one fit call per class that occurs.
5. the constants against the header, the export.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import group_ref as G
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec
from test_render_host import DEV, HANDLE, StubLib, make_ctx

NS = 40
FILL = G.FILLER_ORIGIN


# ---- 1. the yardstick
def _rows(ref):
    return [tuple(r) for r in ref['groups'].tolist()]


def test_exact_link_cases():
    _, _, _, ref = G.scene_reference('exact5')
    # 3-4-5 at crit 5: d2 = 25 = c2, linked; two stars at one position: linked
    assert list(ref['label']) == [0, 0, 2, 2] and list(ref['counts']) == [2, 0, 2, 0, 0, 0]
    assert _rows(ref) == [(2, 0, 0, 0, 0, 1, -1, -1), (2, 0, 2, 0, 2, 3, -1, -1)]
    # centre of (10, 10), (13, 14) is (11.5, 12): floor(12.0) = 12, floor(12.5) = 12 -> origin (-8, -8)
    assert ref['origin'].tolist() == [[-8, -8], [20, 20]]
    assert ref['shift'][0, :2].tolist() == [[-2.0, -2.0], [1.0, 2.0]] and not ref['shift'][1].any()
    _, crit, _, ref = G.scene_reference('exact5-')
    assert crit < 5.0 and crit * crit < 25.0
    assert list(ref['label']) == [0, 1, 2, 2] and list(ref['counts']) == [3, 2, 1, 0, 0, 0]
    assert _rows(ref) == [(1, 0, 0, 0, 0, -1, -1, -1), (1, 0, 1, 0, 1, -1, -1, -1), (2, 0, 2, 0, 2, 3, -1, -1)]
    assert ref['origin'].tolist() == [[-10, -10], [-7, -6], [20, 20]]


def test_pairs_across_borders_and_corners():
    pos, crit, shape, ref = G.scene_reference('borders')
    n = len(G.BORDER_PAIRS)
    want = np.repeat(np.arange(0, 2 * n, 2), 2)
    want[-1] = 2 * n - 1                                         # the last pair is 2.5 apart: two singles
    assert list(ref['label']) == list(want) and list(ref['counts']) == [n + 1, 2, n - 1, 0, 0, 0]
    assert _rows(ref)[:2] == [(1, 0, 2 * n - 2, 0, 2 * n - 2, -1, -1, -1), (1, 0, 2 * n - 1, 0, 2 * n - 1, -1, -1, -1)]
    assert _rows(ref)[2:] == [(2, 0, 2 * k, 0, 2 * k, 2 * k + 1, -1, -1) for k in range(n - 1)]
    # the pair (15.999..., 90), (16, 90): c = 16.0 after rounding, origin 16 - 20
    assert ref['origin'][3].tolist() == [-4, 70]
    assert ref['shift'][3, :2].tolist() == [[G.BELOW16 - 16.0, 0.0], [0.0, 0.0]]


def test_link_across_a_whole_cell_at_the_largest_crit():
    pos, crit, shape, ref = G.scene_reference('far')
    assert 32.0 - G.BELOW16 == 16.0 and 33.0 - G.BELOW17 > 16.0
    assert list(ref['label']) == [0, 0, 2, 3] and list(ref['counts']) == [3, 2, 1, 0, 0, 0]
    # (the pair is as wide as a group can be: its first member lies just beyond 8 pixels from the centre)
    assert _rows(ref)[2] == (2, G.WIDE, 0, 0, 0, 1, -1, -1) and ref['origin'][2].tolist() == [4, 180]


def test_wide_chain_and_edges():
    _, _, _, ref = G.scene_reference('wide')
    assert list(ref['label']) == [0, 0, 0, 0] and _rows(ref) == [(4, G.WIDE, 0, 0, 0, 1, 2, 3)]
    # c = 58.85 -> floor(59.35) = 59; the first star lies 9 pixels from it
    assert ref['origin'].tolist() == [[30, 39]] and ref['shift'][0, 0].tolist() == [0.0, -9.0]
    assert abs(ref['shift'][0, 3, 1] - 8.7) < 1e-12
    pos, _, (ny, nx), ref = G.scene_reference('edges')
    assert list(ref['label']) == [0, 0, 2, 2, 4, 5, 5, 7] and list(ref['counts']) == [5, 2, 3, 0, 0, 0]
    # (-1, -1) with (0.5, 0): c = (-0.25, -0.5) -> floor(0.25) = 0, floor(0.0) = 0
    assert ref['origin'][2].tolist() == [-20, -20] and ref['shift'][2, 0].tolist() == [-1.0, -1.0]
    with pytest.raises(ValueError):
        G.group(np.array([[-1.0000001, 0.0]]), 2.0, (10, 10))
    out = G.group(np.array([[-1.0000001, 0.0], [np.inf, 2.0], [np.nan, np.inf], [3.0, 3.0], [3.0, 10.000001]]), 2.0,
                  (10, 10), device=True)
    assert list(out['label']) == [-2, -2, -1, 3, -2] and list(out['counts']) == [1, 1, 0, 0, 0, 0]


def test_chains_are_one_oversize_group_each():
    pos, crit, shape, ref = G.scene_reference('chains')
    assert list(ref['counts']) == [3, 0, 0, 0, 0, 3]
    assert sorted(ref['groups'][:, 0].tolist()) == [200, 200, 400]
    assert np.all(ref['groups'][:, 1] == G.OVERSIZE) and np.all(ref['origin'] == FILL) and not ref['shift'].any()
    for row in ref['groups']:
        members = np.flatnonzero(ref['label'] == row[2])
        assert list(row[4:]) == list(members[:4]) and row[2] == members[0]
    # the diagonal crosses many 16-pixel cells; the others run along the cell borders themselves
    big = pos[ref['label'] == ref['groups'][np.argmax(ref['groups'][:, 0]), 2]]
    assert len(np.unique(np.floor(big / 16.0), axis=0)) > 40
    assert np.count_nonzero(pos[:, 0] == 16.0) == 200 and np.count_nonzero(pos[:, 1] == 32.0) == 200


def test_field_has_every_class_and_grid_pairs_are_all_pairs():
    pos, crit, shape, ref = G.scene_reference('field')
    G.check_field_classes(ref)
    assert np.all(ref['groups'][:, 0] == np.bincount(ref['label'])[ref['groups'][:, 2]])
    klass = np.minimum(ref['groups'][:, 0], 5)
    assert np.all(np.diff(klass) >= 0)
    for k in range(1, 6):
        assert np.all(np.diff(ref['groups'][klass == k, 2]) > 0)
    other = G.group(pos, crit, shape, pairs='grid')
    for key in ref:
        np.testing.assert_array_equal(other[key], ref[key])
    # a permutation gives the same groups as sets
    perm = np.random.default_rng(2).permutation(len(pos))
    moved = G.group(pos[perm], crit, shape)
    inv = np.argsort(perm)
    first = np.full(len(pos), len(pos))
    np.minimum.at(first, ref['label'], inv)                      # smallest new index of every old group
    assert np.array_equal(moved['label'][inv], first[ref['label']])


def test_shift_buffer_has_the_pitch_of_each_class():
    _, _, _, ref = G.scene_reference('field')
    c = ref['counts']
    off = np.concatenate([[0], np.cumsum(c[1:])])
    for mg in (int(c[0]), int(off[2]) + 3, 5):
        groups, origin, shift = G.buffers(ref, mg)
        assert groups.shape == (mg, 8) and origin.shape == (mg, 2) and shift.shape == (mg * 8,)
        for k in range(1, 5):
            n = min(int(off[k]), mg) - min(int(off[k - 1]), mg)
            if n > 0:
                lo = int(off[k - 1])
                block = shift[8 * lo:8 * lo + 2 * k * n].reshape(n, k, 2)
                np.testing.assert_array_equal(block, ref['shift'][lo:lo + n, :k])
                assert not shift[8 * lo + 2 * k * n:8 * min(int(off[k]), mg)].any()
        np.testing.assert_array_equal(_lib.group_shift_rows(shift, c), ref['shift'][:mg])
    assert list(_lib.group_offsets(c)) == list(off)


# ---- 2. what reaches C, and what the host form makes of the answer
def _array(ptr, n, ctype, dtype):
    return np.frombuffer((ctype * n).from_address(ptr.value), dtype=dtype)


class TableLib(StubLib):
    """The recording stub, whose mpsfr_group_stars answers with the reference's tables for the positions it is handed,
    and whose fits answer F = 1000 dp + dq of every source's start shift with status 0."""

    def mpsfr_group_stars(self, *a):
        self.calls.append(('mpsfr_group_stars', a))
        _, ny, nx, nstar, pos, stride, crit, max_groups, label, groups, origin, shift, count, on_device = a
        p = _array(pos, nstar * stride, C.c_double, np.float64).reshape(nstar, stride)
        ref = G.group(p, crit, (ny, nx))
        g, o, s = G.buffers(ref, max_groups)
        _array(label, nstar, C.c_int32, np.int32)[:] = ref['label']
        _array(groups, max_groups * 8, C.c_int32, np.int32)[:] = g.ravel()
        _array(count, 6, C.c_int32, np.int32)[:] = ref['counts']
        if origin is not None:
            _array(origin, max_groups * 2, C.c_int32, np.int32)[:] = o.ravel()
            _array(shift, max_groups * 8, C.c_double, np.float64)[:] = s
        return 0

    def mpsfr_fit_stamps_psf(self, *a):
        self.calls.append(('mpsfr_fit_stamps_psf', a))
        n = a[1]
        sh = _array(a[7], 2 * n, C.c_double, np.float64).reshape(n, 2)
        out = _array(a[9], n * _lib.NFIT_PSF, C.c_double, np.float64).reshape(n, _lib.NFIT_PSF)
        out[:] = 0.0
        out[:, 0] = 1000.0 * sh[:, 0] + sh[:, 1]
        out[:, 1:3] = sh
        out[:, 11] = 1600
        return 0

    def mpsfr_fit_groups_psf(self, *a):
        self.calls.append(('mpsfr_fit_groups_psf', a))
        n, K = a[1], a[2]
        sh = _array(a[8], 2 * n * K, C.c_double, np.float64).reshape(n, K, 2)
        out = _array(a[10], n * _lib.NFIT_GROUP, C.c_double, np.float64).reshape(n, _lib.NFIT_GROUP)
        out[:] = 0.0
        out[:, 5], out[:, 6] = 1600, K
        for k in range(K):
            out[:, 8 + 8 * k] = 1000.0 * sh[:, k, 0] + sh[:, k, 1]
            out[:, 9 + 8 * k:11 + 8 * k] = sh[:, k]
        out[:, 40:46] = 0.5
        return 0


def table_ctx():
    ctx = make_ctx()
    ctx.lib = TableLib()
    return ctx


@pytest.fixture
def ctx():
    c = make_ctx()
    yield c
    c._h = None


def test_group_stars_host_form():
    ctx = table_ctx()
    pos, crit, shape, ref = G.scene_reference('field')
    wide = np.concatenate([pos, np.full((len(pos), 6), 7.0)], axis=1)                   # stride 8, as the finder's rows
    label, groups, origin, shift, counts = ctx.group_stars(wide, crit, shape)
    name, a = ctx.lib.calls[0]
    assert name == 'mpsfr_group_stars' and len(ctx.lib.calls) == 1 and a[0].value == HANDLE
    assert (a[1], a[2], a[3], a[5], a[6], a[7], a[13]) == (200, 200, 1500, 8, 2.5, 1500, 0)
    assert all(isinstance(v, int) and not isinstance(v, bool) for v in (a[1], a[2], a[3], a[5], a[7]))
    assert isinstance(a[6], float)
    n = int(ref['counts'][0])
    assert label.dtype == groups.dtype == origin.dtype == counts.dtype == np.int32 and shift.dtype == np.float64
    assert groups.shape == (n, 8) and origin.shape == (n, 2) and shift.shape == (n, 4, 2) and counts.shape == (6,)
    assert a[8].value == label.ctypes.data and a[9].value == groups.ctypes.data and a[10].value == origin.ctypes.data
    assert groups.base.shape == (1500, 8) and origin.base.shape == (1500, 2)
    for got, key in ((label, 'label'), (groups, 'groups'), (origin, 'origin'), (shift, 'shift'), (counts, 'counts')):
        np.testing.assert_array_equal(got, ref[key])
    ctx.lib.calls.clear()
    label, groups, origin, shift, counts = ctx.group_stars(pos.tolist(), np.float32(2.5), shape, max_groups=800)
    assert ctx.lib.calls[0][1][7] == 800 and ctx.lib.calls[0][1][5] == 2
    assert groups.shape == (800, 8) and origin.shape == (800, 2) and shift.shape == (800, 4, 2)
    np.testing.assert_array_equal(groups, ref['groups'][:800])
    np.testing.assert_array_equal(shift, ref['shift'][:800])
    np.testing.assert_array_equal(counts, ref['counts'])
    ctx._h = None


def test_group_stars_device_form(ctx):
    assert ctx.group_stars_device(97, 150, 4096, DEV['rows'], 8, 2.5, 512, DEV['index'], DEV['out'], DEV['scale']) is None
    name, a = ctx.lib.calls[0]
    assert name == 'mpsfr_group_stars' and len(a) == 14 and a[0].value == HANDLE
    assert (a[1], a[2], a[3], a[5], a[6], a[7], a[13]) == (97, 150, 4096, 8, 2.5, 512, 1)
    assert (a[4].value, a[8].value, a[9].value, a[12].value) == (DEV['rows'], DEV['index'], DEV['out'], DEV['scale'])
    assert a[10] is None and a[11] is None
    ctx.lib.calls.clear()
    ctx.group_stars_device(97, 150, 1, DEV['rows'], 2, 16, 1, DEV['index'], DEV['out'], DEV['scale'],
                           origin_ptr=DEV['origin'], shift_ptr=DEV['shift'])
    a = ctx.lib.calls[0][1]
    assert (a[3], a[5], a[6], a[7]) == (1, 2, 16.0, 1) and (a[10].value, a[11].value) == (DEV['origin'], DEV['shift'])


# ---- 3. the refusals
def test_group_stars_refuses(ctx):
    pos = np.array([[1.0, 2.0], [3.0, 4.0], [np.nan, 0.0]])
    base = dict(pos=pos, crit=2.5, shape=(10, 12), max_groups=None)
    bad = [dict(pos=pos[0]), dict(pos=pos[:, :1]), dict(pos=np.zeros((0, 2))), dict(pos='p'), dict(pos=pos[None]),
           dict(pos=[[1.0, 12.5]]), dict(pos=[[10.5, 1.0]]), dict(pos=[[-1.5, 1.0]]), dict(pos=[[1.0, -1.01]]),
           dict(pos=[[np.inf, 1.0]]), dict(pos=[[1.0, -np.inf]]),
           dict(crit=0), dict(crit=-1.0), dict(crit=16.000001), dict(crit=np.nan), dict(crit=np.inf), dict(crit='2'),
           dict(crit=None), dict(crit=True),
           dict(shape=(10,)), dict(shape=10), dict(shape=(0, 12)), dict(shape=(10, 16385)), dict(shape=(10.0, 12)),
           dict(shape=(8193, 8193)),
           dict(max_groups=0), dict(max_groups=-3), dict(max_groups=2.0), dict(max_groups=True)]
    for kw in bad:
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError):
            ctx.group_stars(args['pos'], args['crit'], args['shape'], max_groups=args['max_groups'])
    ok = (97, 150, 10, 1, 2, 2.5, 10, 1, 1, 1)
    for k, v in [(0, 0), (1, 16385), (0, 97.0), (2, 0), (2, 2 ** 24 + 1), (2, 1.0), (3, 0), (3, None), (4, 1), (4, 2.0),
                 (5, 0.0), (5, -1.0), (5, 16.5), (5, np.nan), (5, np.inf), (6, 0), (6, 1.5), (7, 0), (8, 0), (9, None)]:
        a = list(ok)
        a[k] = v
        with pytest.raises(ValueError):
            ctx.group_stars_device(*a)
    for kw in (dict(origin_ptr=1), dict(shift_ptr=1)):
        with pytest.raises(ValueError):
            ctx.group_stars_device(*ok, **kw)
    assert ctx.lib.calls == []
    ctx.group_stars([[-1.0, 12.0], [10.0, -1.0]], 16, (10, 12), max_groups=1)       # the bounds themselves are legal
    ctx.group_stars_device(16384, 4096, 2 ** 24, 1, 2, 16.0, 1, 1, 1, 1)
    assert len(ctx.lib.calls) == 2


def test_psfrec_group_and_fit_refuse(monkeypatch):
    ctx = make_ctx()
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: ctx)
    for args, kw in (((np.zeros(3), 2.5), {}), (('p', 2.5), {}), ((np.zeros((3, 3)), 2.5), {}),
                     ((np.zeros((2, 2)), 0.0), {}), ((np.zeros((2, 2)), 17.0), {}),
                     ((np.zeros((2, 2)), 2.5), dict(pixscale=0.0)), ((np.full((2, 2), 5.0), 2.5), dict(shape=(4, 4)))):
        with pytest.raises(ValueError):
            psfrec.group_stars(*args, **kw)
    image, psf, found = np.zeros((30, 30)), np.zeros((NS, NS)), np.array([[3.0, 4.0], [5.0, 6.0]])
    for kw in (dict(crit=0.0), dict(crit=20.0), dict(crit=2.5, fit_back=1), dict(crit=2.5, mode='loose'),
               dict(crit=2.5, pixscale=-1.0), dict(crit=2.5, var=np.zeros((3, 3)))):
        with pytest.raises(ValueError):
            psfrec.fit_found_stars(image, psf, found, **kw)
    for bad in (np.array([[3.0, np.nan]]), np.array([[3.0, 31.0]]), np.zeros(2)):
        with pytest.raises(ValueError):
            psfrec.fit_found_stars(image, psf, bad, crit=2.5)
    with pytest.raises(ValueError):
        psfrec.fit_found_stars(image, np.zeros((3, NS, NS)), found, crit=2.5)
    with pytest.raises(TypeError):
        psfrec.fit_found_stars(image, psf, found)                                      # crit has no default
    assert ctx.lib.calls == []
    ctx._h = None


# ---- 4. psfrec against the answering stub
def _answering(monkeypatch):
    ctx = table_ctx()
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: ctx)
    return ctx


def test_psfrec_group_stars_tables(monkeypatch):
    ctx = _answering(monkeypatch)
    pos, crit, shape, ref = G.scene_reference('field')
    pos = pos.copy()
    pos[7] = np.nan
    ref = G.group(pos, crit, shape)
    stars, groups = psfrec.group_stars({'position': pos}, crit, shape)
    assert len(ctx.lib.calls) == 1
    assert tuple(stars.colnames) == ('label', 'size', 'flags')
    assert tuple(groups.colnames) == ('label', 'size', 'members', 'origin', 'shift', 'flags')
    np.testing.assert_array_equal(stars['label'], ref['label'])
    size = np.bincount(ref['label'][ref['label'] >= 0], minlength=len(pos))
    assert stars['label'][7] == -1 and stars['size'][7] == 0 and stars['flags'][7] == 0
    keep = ref['label'] >= 0
    np.testing.assert_array_equal(np.asarray(stars['size'])[keep], size[ref['label'][keep]])
    np.testing.assert_array_equal(np.asarray(stars['flags'])[keep] != 0, size[ref['label'][keep]] > 4)
    np.testing.assert_array_equal(groups['members'], ref['groups'][:, 4:])
    np.testing.assert_array_equal(groups['origin'], ref['origin'])
    np.testing.assert_array_equal(groups['shift'], ref['shift'])
    np.testing.assert_array_equal(groups['size'], ref['groups'][:, 0])
    assert np.asarray(groups['origin']).dtype == np.int32 and groups.meta['counts'] == ref['counts'].tolist()
    ctx.lib.calls.clear()
    psfrec.group_stars(pos, crit)                                  # shape=None: the smallest frame that holds them
    a = ctx.lib.calls[0][1]
    assert (a[1], a[2]) == tuple(int(np.ceil(v)) for v in np.nanmax(pos, axis=0))
    ctx._h = None


def crowd():
    """Singles, pairs, a triple, a quad, a chain of five (oversize) and a wide chain of four, at crit = 6, in an order
    that scatters every group over the list."""
    groups = [[(20.0, 20.0)], [(20.0, 60.0)], [(20.3, 100.0)],
              [(60.0, 20.0), (60.0, 24.5)], [(60.0, 60.0), (63.5, 62.0)],
              [(100.0, 20.0), (103.0, 23.0), (100.5, 26.0)],
              [(100.0, 60.0), (104.0, 60.0), (104.0, 64.0), (100.0, 64.0)],
              [(140.0, 20.0 + 5.0 * k) for k in range(5)],
              [(180.0, 50.0), (180.0, 55.9), (180.0, 61.8), (180.0, 67.7)]]
    pos = np.array([p for g in groups for p in g])
    perm = np.random.default_rng(4).permutation(len(pos))
    return pos[perm], 6.0, (200, 120)


def test_fit_found_stars_restores_input_order(monkeypatch):
    ctx = _answering(monkeypatch)
    pos, crit, shape = crowd()
    ref = G.group(pos, crit, shape)
    assert list(ref['counts']) == [9, 3, 2, 1, 2, 1] and ref['groups'][6, 1] == G.WIDE
    image = np.zeros(shape)
    psf = np.zeros((NS, NS))
    psf[20, 20] = 1.0
    fit, origin = psfrec.fit_found_stars(image, psf, {'position': pos}, crit=crit, pixscale=0.25)
    names = [c[0] for c in ctx.lib.calls]
    # one group call, then one cut and one fit per class that occurs (the wide quad leaves one quad to fit)
    assert names == ['mpsfr_group_stars', 'mpsfr_cut_stamps', 'mpsfr_fit_stamps_psf'] + \
        ['mpsfr_cut_stamps', 'mpsfr_fit_groups_psf'] * 3
    assert [c[1][5] for c in ctx.lib.calls if c[0] == 'mpsfr_cut_stamps'] == [3, 2, 1, 1]
    assert [(c[1][1], c[1][2]) for c in ctx.lib.calls if c[0] == 'mpsfr_fit_groups_psf'] == [(2, 2), (1, 3), (1, 4)]
    assert tuple(fit.colnames) == psfrec._FIT_COLS_GROUP + ('nsrc', 'label', 'crowded')
    assert len(fit) == len(pos) and origin.dtype == np.int32
    np.testing.assert_array_equal(origin, ref['origin'])
    np.testing.assert_array_equal(fit['label'], ref['label'])
    row = {int(r[2]): k for k, r in enumerate(ref['groups'])}
    grp = np.array([row[int(v)] for v in ref['label']])
    np.testing.assert_array_equal(fit['group'], grp)
    np.testing.assert_array_equal(fit['nsrc'], ref['groups'][grp, 0])
    crowded = ref['groups'][grp, 1] != 0
    assert crowded.sum() == 9
    np.testing.assert_array_equal(fit['crowded'], crowded)
    np.testing.assert_array_equal(np.asarray(fit['status'])[crowded], 2)
    np.testing.assert_array_equal(np.asarray(fit['status'])[~crowded], 0)
    assert np.all(np.isnan(np.asarray(fit['scale'])[crowded])) and np.all(np.asarray(fit['npix'])[crowded] == 0)
    # every fitted star got the answer to ITS start shift: position minus the centre pixel of its group's stamp
    start = pos - (ref['origin'][grp] + NS // 2)
    ok = ~crowded
    np.testing.assert_array_equal(np.asarray(fit['scale'])[ok], 1000.0 * start[ok, 0] + start[ok, 1])
    np.testing.assert_array_equal(np.asarray(fit['shift'])[ok], start[ok] * 0.25)
    for k in range(len(pos)):
        members = np.flatnonzero(ref['label'] == ref['label'][k])
        assert fit['source'][k] == list(members).index(k)
    assert np.all(np.asarray(fit['max_corr'])[ok & (ref['groups'][grp, 0] > 1)] == 0.5)
    assert np.all(np.asarray(fit['max_corr'])[ok & (ref['groups'][grp, 0] == 1)] == 0.0)
    # the table is what subtract_stars takes: its group column indexes origin
    assert np.asarray(fit['group']).max() == len(origin) - 1 and np.asarray(fit['group']).min() == 0
    ctx._h = None


def test_fit_found_stars_modes(monkeypatch):
    ctx = _answering(monkeypatch)
    pos, crit, shape = crowd()
    var = np.ones(shape)
    psfrec.fit_found_stars(np.zeros(shape), np.eye(NS), pos, var=var, crit=crit, fit_back=False, mode='fixed')
    flags = {c[0]: c[1] for c in ctx.lib.calls}
    assert flags['mpsfr_fit_stamps_psf'][8] == _lib.FIT_FIXED_SHIFT
    assert flags['mpsfr_fit_groups_psf'][9] == _lib.FIT_FIXED_SHIFT
    assert flags['mpsfr_cut_stamps'][4] is not None and flags['mpsfr_fit_groups_psf'][4] is not None
    ctx._h = None


# ---- 5. constants and exports
def test_exports_and_header_constants():
    assert 'mpsfr_group_stars' in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    for name, val in (('NGROUP', _lib.NGROUP), ('GROUP_OVERSIZE', _lib.GROUP_OVERSIZE), ('GROUP_WIDE', _lib.GROUP_WIDE)):
        assert int(re.search(r'#define MPSFR_%s\s+(\d+)' % name, hdr).group(1)) == val, name
    assert float(re.search(r'#define MPSFR_GROUP_MAX_CRIT\s+([\d.]+)', hdr).group(1)) == _lib.GROUP_MAX_CRIT
    assert (_lib.NGROUP, _lib.GROUP_MAX_CRIT, _lib.GROUP_OVERSIZE, _lib.GROUP_WIDE) == (8, 16.0, 1, 2)
    assert _lib.GROUP_MAX_CRIT == 2 * _lib.FIT_PSF_MAX_SHIFT and _lib.GROUP_FILLER_ORIGIN == FILL
    assert (G.NGROUP, G.OVERSIZE, G.WIDE, G.MAX_GROUP, G.MAX_SHIFT) == \
        (_lib.NGROUP, _lib.GROUP_OVERSIZE, _lib.GROUP_WIDE, _lib.MAX_GROUP, _lib.FIT_PSF_MAX_SHIFT)
    import muse_psfr_amd
    for name in ('group_stars', 'fit_found_stars', 'NGROUP', 'GROUP_MAX_CRIT', 'GROUP_OVERSIZE', 'GROUP_WIDE'):
        assert hasattr(muse_psfr_amd, name), name
    src = open(os.path.join(ROOT, 'muse_psfr_amd', 'csrc', 'group.hip')).read()
    assert int(re.search(r'constexpr int kCell = (\d+);', src).group(1)) > _lib.GROUP_MAX_CRIT
    assert 'group.hip' in __import__('muse_psfr_amd._build', fromlist=['SOURCES']).SOURCES


# ---- 6. the scene of the GPU chain test, checked on the CPU against the NumPy yardsticks of find, render and the fits
def _cut(frame, o):
    ny, nx = frame.shape
    out = np.full((NS, NS), np.nan)
    ys, xs = slice(max(o[0], 0), min(o[0] + NS, ny)), slice(max(o[1], 0), min(o[1] + NS, nx))
    out[ys.start - o[0]:ys.stop - o[0], xs.start - o[1]:xs.stop - o[1]] = frame[ys, xs]
    return out


def test_blend_scene_has_margin_on_the_cpu():
    """What test_gpu_group.py asserts of the chain, on the yardsticks alone: all 40 stars are found, the groups are the
    blends, every blended flux lies within 5 of its errors (measured: 2.3) and every single-star fit of a blended star
    misses by more than that (30 of 30) -- neither bound is marginal at this noise."""
    import find_ref as F
    import psf_fit_ref as PF
    import psf_group_ref as PG
    import render_ref as Y
    pos, flux, blend = G.blend_field()
    assert len(pos) == 40 and sorted(np.bincount(blend)[1:] // np.arange(1, 4)) == [4, 9, 10]
    psf = F.model()
    origin = (np.rint(pos) - NS // 2).astype(np.int32)
    frame = Y.render(G.blend_background(), psf[None], np.zeros(40, dtype=np.int32), origin, pos - np.rint(pos), flux)[0]
    found = F.find(frame, np.ones_like(frame), psf, **G.BLEND_FIND)
    assert found['count'] == 40
    fp = found['rows'][:40, :2]
    near = np.argmin(((fp[:, None] - pos[None]) ** 2).sum(-1), axis=1)
    assert sorted(near) == list(range(40))
    g = G.group(fp, G.BLEND_CRIT, frame.shape)
    assert list(g['counts']) == [23, 10, 9, 4, 0, 0] and not g['groups'][:, 1].any()
    worst, misses, blended = 0.0, 0, 0
    for row in range(10, 23):
        n = g['groups'][row, 0]
        members = g['groups'][row, 4:4 + n]
        assert np.all(blend[near[members]] == n)
        st = _cut(frame, g['origin'][row])
        fit = PG.fit(st, np.ones_like(st), psf, g['shift'][row, :n], True, 'free')
        worst = max(worst, float(np.max(np.abs(fit['F'] - flux[near[members]]) / fit['err_F'])))
        for m in members:
            o = (np.rint(fp[m]) - NS // 2).astype(int)
            st = _cut(frame, o)
            one = PF.fit(st, np.ones_like(st), psf, True, shift=fp[m] - np.rint(fp[m]))
            blended += 1
            misses += abs(one['x'][0] - flux[near[m]]) > 5 * one['err'][0]
    print('blend scene: worst flux error %.2f sigma, %d of %d single fits miss' % (worst, misses, blended))
    assert worst < 3.0 and blended == 30 and misses == 30
