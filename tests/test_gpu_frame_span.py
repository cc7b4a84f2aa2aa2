"""GPU: the frame and cube calls beyond one workgroup's span of work, both precisions (the scenes and the facts that make
them cross their constants: frame_span_cases.py, asserted in test_frame_span_host.py; the table: DESIGN.md section 8).

1. padded lists -- any star list inside 2101 rows, the live stars on both sides of every trip of 1024: render_stars and
   fit_frame_psf against the unpadded calls and yardsticks; fit_frame_psf_free and fit_cube_psf_free under the checks of
   section 1 of their own GPU test files with the yardsticks of the unpadded scenes; fit_cube_psf layer by layer
   against fit_frame_psf on the same padded list.
2. the live lattice -- 1023, 1024 and 1089 stars (nu = 1024, 1025, 1090 with the background, 1089 without) against
   frame_fit_ref.solve_sparse within frame_fit_ref.bounds at tol 1e-10 and max_iter 100; fit_frame_psf_free with
   max_outer = 0 under section 4's contract of test_gpu_frame_free.py; two layers through fit_cube_psf bit for bit.
   Out of scope: a converged free yardstick at 3 x 1089 unknowns (its dense solves do not fit a test).
3. the long frame 257 x 16384 -- 1028 partials, 4608 tiles: fit_frame_psf, render_stars and find_stars.
4. the tile-count frames 1024 x 1024 and 1312 x 800 (1024 and 1025 tiles): render_stars and fit_frame_psf.
5. the finder frames -- 1024 and 1028 segments, max_stars inside chunk 1, more than 8192 peaks.
6. the deep cube -- 1025 layers: fit_cube_psf at layer_batch 0, 1024 and 1025 against three frame calls;
   fit_cube_psf_free with max_outer = 0 (k_cf_step's loops over the layers) against the joint held solve.
   Out of scope: the converged parity of fit_cube_psf_free on the deep cube (the dense joint yardstick of
   cube_free_ref over 1025 layers is gigabytes, with one star too).
Every bound is frame_fit_ref.bounds, find_ref.row_bounds / stat_bounds, the renderer's 1e-13 S, or bit equality.  Worst
error / bound ratios go to record_margin('frame_span', ...).
"""
import numpy as np
import pytest

import cube_fit_cases as K
import cube_free_cases as Q
import cube_free_ref as R
import find_ref as FR
import frame_fit_ref as F
import frame_free_ref as G
import frame_span_cases as S
import render_ref as Y
from conftest import record_margin
from test_gpu_cube_free import _check_layer
from test_gpu_find import assert_parity, raw_find
from test_gpu_frame_fit import _check_against
from test_gpu_frame_free import _check_closing

pytestmark = pytest.mark.gpu

PRECS = ['mixed', 'f64']
NS = 40
TOL, MAX_ITER = 1e-10, 100
FREE_TOL = 1e-12                       # of the free calls' parity runs (test_gpu_frame_free.py, test_gpu_cube_free.py)
PARITY = 1e-13                         # the renderer's per-pixel bound in units of S
EPS = F.EPS


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
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _fit(ctx, s, radius, background=True, **kw):
    return ctx.fit_frame_psf(s['image'], s['psf'], s['origin'], var=s['var'], shift=s['shift'], psf_index=s['index'],
                             radius=radius, background=background, max_iter=MAX_ITER, tol=TOL, **kw)


def _render(ctx, s, **kw):
    return ctx.render_stars(s['psf'], s['origin'], s['scale'], shift=s['shift'], psf_index=s['index'], image=s['image'],
                            **kw)


def _record(tag, ratios):
    print('frame span %s: error / bound %s' % (tag, ', '.join('%s %.2e' % kv for kv in sorted(ratios.items()))))
    record_margin('frame_span', **{'%s_%s' % (k, tag): v for k, v in ratios.items()})


def _fillers(places):
    return np.setdiff1d(np.arange(S.TOTAL), places)


FILLER_ROW = [0, 0, 0, 0, 0, 0, 0, 1]


# ---- 1. padded lists
@pytest.mark.parametrize('subtract', [False, True])
@pytest.mark.parametrize('prec', PRECS)
def test_padded_render_equals_the_unpadded_call_bit_for_bit(ctx, prec, subtract):
    s = Y.scene()
    p, places = S.pad_scene(s, ('origin', 'shift', 'scale', 'index'), 1)
    want, wrows = _render(ctx, s, subtract=subtract, return_status=True)
    got, rows = _render(ctx, p, subtract=subtract, return_status=True)
    assert rows.shape == (S.TOTAL, 4)
    assert _same(got, want) and _same(rows[places], wrows)          # the sum at a pixel runs in star-index order
    fill = _fillers(places)
    assert np.all(rows[fill, 0] == 1) and not rows[fill, 1:].any()
    # and the unpadded call is the yardstick's (test_gpu_render.py), so the padded one is
    ref, npix, Sm = Y.scene_reference(subtract)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan) and np.max(np.abs(got - ref)[~nan] / Sm[~nan]) <= PARITY


@pytest.mark.parametrize('prec', PRECS)
def test_padded_frame_fit(ctx, prec):
    s = F.scene()
    p, places = S.pad_scene(s, ('origin', 'shift', 'index'), 2)
    ref = F.scene_reference(True, True, 8.0)
    b = F.bounds(ref, TOL, MAX_ITER)
    rows, head, resid = _fit(ctx, p, 8.0, return_residual=True)
    assert rows.shape == (S.TOTAL, 8)
    _record('padded_fit_%s' % prec, _check_against(rows[places], head, ref, b))
    fill = _fillers(places)
    assert np.all(rows[fill] == np.array(FILLER_ROW, dtype=float))
    r0, h0 = _fit(ctx, s, 8.0)
    assert head[3] == h0[3] and head[6] == h0[6] and _same(rows[places][:, [5, 7]], r0[:, [5, 7]])
    acc = np.flatnonzero(rows[:, 7] == 0)
    assert np.array_equal(acc, places[ref['acc']])
    want = ctx.render_stars(p['psf'], p['origin'][acc], rows[acc, 0], shift=p['shift'][acc], psf_index=p['index'][acc],
                            image=p['image'], subtract=True)
    assert _same(resid, want)


_FREE_RULE = {}


@pytest.mark.parametrize('prec', PRECS)
def test_padded_frame_free_follows_the_unpadded_yardsticks(ctx, prec):
    """Section 1 of test_gpu_frame_free.py (var, background, radius 8) on the padded displaced scene: its checks on the
    live rows against the converged yardstick and the rule of the unpadded scene, and the fillers left out."""
    s0 = G.displaced_scene(False)
    s, places = S.pad_scene(s0, ('origin', 'shift', 'index'), 4)
    conv = G.scene_converged(True, True, 8.0, False, max_outer=10)
    pr, acc, fi = conv['problem'], conv['problem'].acc, conv['last']['free_idx']
    assert conv['rho'] < 0.5 and len(fi) == len(acc)
    pos_tol = G.parity_pos_tol(conv, FREE_TOL, MAX_ITER)
    bound, _ = G.position_bounds(conv, pos_tol, FREE_TOL, MAX_ITER)
    steps = np.array(conv['steps'])
    assert not np.any(np.abs(steps - pos_tol) <= 0.1 * pos_tol)
    nouter = int(np.argmax(steps <= pos_tol)) + 1
    rows, shifts, head = ctx.fit_frame_psf_free(s['image'], s['psf'], s['origin'], var=s['var'], shift=s['shift'],
                                                psf_index=s['index'], radius=8.0, background=True, max_iter=MAX_ITER,
                                                tol=FREE_TOL, max_outer=10, pos_tol=pos_tol)
    assert rows.shape == (S.TOTAL, 16) and shifts.shape == (S.TOTAL, 2) and head.shape == (12,)
    fill = _fillers(places)
    assert np.all(rows[fill, 7] == 1) and _same(shifts[fill], s['shift'][fill]) and _same(rows[fill, 8:10], s['shift'][fill])
    assert not rows[fill, :7].any() and not rows[fill, 10:].any()
    rows, shifts = rows[places], shifts[places]
    np.testing.assert_array_equal(rows[:, 7], conv['status'])
    np.testing.assert_array_equal(rows[:, 5], pr.base['ndisc'])
    assert (head[3], head[6], head[7], head[8], head[10]) == (pr.nomega, pr.nacc, 0, nouter, len(acc))
    assert head[9] <= pos_tol
    if 'rule' not in _FREE_RULE:
        _FREE_RULE['rule'] = G.refine(s0['image'], s0['var'], s0['psf'], s0['index'], s0['origin'], s0['shift'], 8.0, True,
                                      max_outer=10, pos_tol=pos_tol)
    rule = _FREE_RULE['rule']
    assert rule['nouter'] == nouter and rule['posok']
    np.testing.assert_array_equal(rows[acc, 15], rule['nfree'][acc])
    np.testing.assert_array_equal(rows[acc, 14], rule['flags'][acc])
    out = np.setdiff1d(np.arange(s0['n']), acc)
    assert len(out) >= 2 and _same(shifts[out], s0['shift'][out]) and _same(rows[out, 8:10], s0['shift'][out])
    assert not rows[out, :7].any() and not rows[out, 10:].any()
    assert _same(rows[:, 8:10], shifts) and _same(rows[acc, 12:14], shifts[acc] - s0['shift'][acc])
    err = np.abs(shifts[acc][fi] - conv['shift'][acc][fi])
    ratios = dict(position=float(np.max(err / bound)))
    ref = pr.held(shifts, int(np.sum(rule['nfree'] > 0)))
    ratios.update(_check_closing(rows, head, ref, F.bounds(ref, FREE_TOL, MAX_ITER), acc))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
    _record('padded_free_%s' % prec, ratios)


_CUBE_RULE = {}


@pytest.mark.parametrize('prec', PRECS)
def test_padded_cube_free_follows_the_unpadded_yardsticks(ctx, prec):
    """Section 1 of test_gpu_cube_free.py (var, background, radius 8) on the padded cube of cube_free_cases."""
    c0 = Q.cube(False)
    pad, places = S.pad({k: c0[k] for k in ('origin', 'shift', 'index')}, F.FRAME, 4, S.TOTAL, 5)
    c = dict(c0, n=S.TOTAL, **pad)
    n, nl = c0['n'], Q.NL
    conv = Q.cube_converged(True, True, 8.0, False, max_outer=10)
    cp, free = conv['problem'], conv['last']['free']
    assert conv['rho'] < 0.5 and cp.live == [0, 1, 2]
    pos_tol = R.parity_pos_tol(conv, FREE_TOL, MAX_ITER)
    bound, _ = R.position_bounds(conv, pos_tol, FREE_TOL, MAX_ITER)
    steps = np.array(conv['steps'])
    assert not np.any(np.abs(steps - pos_tol) <= 0.1 * pos_tol)
    nouter = int(np.argmax(steps <= pos_tol)) + 1
    rows, pos, shifts, head, call = ctx.fit_cube_psf_free(c['cube'], c['psf'], c['origin'], var=c['var'], shift=c['shift'],
                                                          layer_shift=c['layer_shift'], psf_index=c['index'], radius=8.0,
                                                          background=True, max_iter=MAX_ITER, tol=FREE_TOL, max_outer=10,
                                                          pos_tol=pos_tol)
    assert rows.shape == (nl, S.TOTAL, 8) and pos.shape == (S.TOTAL, 8) and shifts.shape == (S.TOTAL, 2)
    assert head.shape == (nl, 8) and call.shape == (8,)
    fill = _fillers(places)
    assert np.all(rows[:, fill, 7] == 1) and not rows[:, fill, :7].any() and not pos[fill, 2:].any()
    assert _same(shifts[fill], c['shift'][fill]) and _same(pos[fill, :2], c['shift'][fill])
    rows, pos, shifts = np.ascontiguousarray(rows[:, places]), pos[places], shifts[places]
    if 'rule' not in _CUBE_RULE:
        _CUBE_RULE['rule'] = Q.run(c0, True, True, 8.0, max_outer=10, pos_tol=pos_tol)
    rule = _CUBE_RULE['rule']
    assert rule['nouter'] == nouter and rule['posok']
    for l in range(nl):
        pr = cp.layers[l]
        np.testing.assert_array_equal(rows[l, :, 7], pr.base['status'])
        np.testing.assert_array_equal(rows[l, :, 5], pr.base['ndisc'])
        assert (head[l, 3], head[l, 6], head[l, 7]) == (pr.nomega, pr.nacc, 0)
    assert (call[2], call[4], call[6]) == (nouter, len(free), 0) and call[3] <= pos_tol and call[7] <= FREE_TOL
    assert call[1] == sum(p.nomega - p.nacc - 1 for p in cp.layers) - 2 * len(free)
    assert abs(call[0] - head[:, 2].sum()) <= 4 * EPS * call[0] and np.all(head[:, 4] == head[0, 4])
    np.testing.assert_array_equal(pos[:, 7], rule['nfree'])
    np.testing.assert_array_equal(pos[:, 6], rule['flags'])
    assert rows[Q.MASK_LAYER, Q.MASKED, 7] == 2 and list(conv['carried'][:, Q.MASKED]) == [True, False, True]
    assert pos[Q.MASKED, 7] == nouter and np.all(pos[Q.MASKED, 2:4] > 0)
    out = np.flatnonzero(~cp.seen)
    assert len(out) >= 2 and _same(shifts[out], c0['shift'][out]) and not pos[out, 2:].any() and not rows[:, out, :7].any()
    assert _same(pos[:, :2], shifts) and _same(pos[cp.seen, 4:6], shifts[cp.seen] - c0['shift'][cp.seen])
    ratios = dict(position=float(np.max(np.abs(shifts[free] - conv['shift'][free]) / bound)))
    for l in range(nl):
        ref = cp.layers[l].held(shifts + c0['layer_shift'][l])
        for k, v in _check_layer(rows[l], head[l], ref, F.bounds(ref, FREE_TOL, MAX_ITER), cp.layers[l].acc).items():
            ratios[k] = max(ratios.get(k, 0.0), v)
    for k, v in ratios.items():
        assert v < 1.0, (k, v)
    _record('padded_cube_free_%s' % prec, ratios)


@pytest.mark.parametrize('prec', PRECS)
def test_padded_cube_fit_equals_the_frame_calls_on_the_padded_list(ctx, prec):
    c0 = K.cube()
    pad, places = S.pad({k: c0[k] for k in ('origin', 'shift', 'index')}, F.FRAME, 4, S.TOTAL, 3)
    c = dict(c0, n=S.TOTAL, **pad)
    rows, head, resid = ctx.fit_cube_psf(c['cube'], c['psf'], c['origin'], var=c['var'], shift=c['shift'],
                                         layer_shift=c['layer_shift'], psf_index=c['index'], layer_batch=2,
                                         return_residual=True)
    assert rows.shape == (K.NL, S.TOTAL, 8)
    fill = _fillers(places)
    for l in range(K.NL):
        image, psf, origin, a = K.layer_call(c, l)
        want = ctx.fit_frame_psf(image, psf, origin, return_residual=True, **a)
        assert _same(rows[l], want[0]) and _same(head[l], want[1]) and _same(resid[l], want[2]), l
        assert np.all(rows[l, fill] == np.array(FILLER_ROW, dtype=float)), l
        if l != K.NAN_LAYER:
            np.testing.assert_array_equal(rows[l, places, 7], K.reference(l)['status'])
            assert (head[l, 3], head[l, 6], head[l, 7]) == (K.reference(l)['nomega'], K.reference(l)['nacc'], 0)


# ---- 2. the live lattice
@pytest.mark.parametrize('case', sorted(S.LATTICE_CASES))
@pytest.mark.parametrize('prec', PRECS)
def test_lattice_against_the_sparse_yardstick(ctx, prec, case):
    s, ref = S.lattice_reference(case)
    b = F.bounds(ref, TOL, MAX_ITER)
    rows, head = _fit(ctx, s, S.LATTICE_RADIUS, background=S.LATTICE_CASES[case][1])
    assert rows.shape == (s['n'], 8)
    ratios = _check_against(rows, head, ref, b)
    print('%d iterations' % head[4])
    _record('lattice_%s_%s' % (case, prec), ratios)


@pytest.mark.parametrize('prec', PRECS)
def test_lattice_free_without_outer_steps_is_the_solve_at_the_start(ctx, prec):
    """Section 4's contract of test_gpu_frame_free.py (check_no_outer_step) on the 1089 stars, against solve_sparse."""
    s, ref = S.lattice_reference('1089_back')
    b = F.bounds(ref, TOL, MAX_ITER)
    rows, shifts, head = ctx.fit_frame_psf_free(s['image'], s['psf'], s['origin'], var=s['var'], shift=s['shift'],
                                                psf_index=s['index'], radius=S.LATTICE_RADIUS, background=True,
                                                max_outer=0, max_iter=MAX_ITER, tol=TOL)
    acc = ref['acc']
    np.testing.assert_array_equal(rows[:, 7], ref['status'])
    np.testing.assert_array_equal(rows[:, 5], ref['ndisc'])
    assert (head[3], head[6], head[7]) == (ref['nomega'], ref['nacc'], 0) and 1 <= head[4] <= MAX_ITER and head[5] <= TOL
    x = np.concatenate([rows[acc, 0], [head[0]]])
    ratios = dict(y=float(np.linalg.norm((x - ref['x']) * np.sqrt(ref['dg']))) / b['y'],
                  nkk=float(np.max(np.abs(rows[acc, 6] - ref['nkk'][acc]) / ref['nkk'][acc])) / b['nkk_rel'],
                  overlap=float(np.max(np.abs(rows[acc, 4] - ref['overlap'][acc]) / b['overlap'])),
                  chi2=abs(head[2] - ref['chi2']) / b['chi2'])
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
    rel = b['chi2'] / ref['chi2'] + b['nkk_rel'] + 8 * EPS
    np.testing.assert_allclose(rows[acc, 1], ref['err'][acc], rtol=rel)
    assert _same(shifts, s['shift']) and _same(rows[:, 8:10], s['shift']) and not rows[:, 10:].any()
    assert list(head[8:11]) == [0, 0, 0] and head[11] == head[4]
    _record('lattice_free0_%s' % prec, ratios)


@pytest.mark.parametrize('prec', PRECS)
def test_lattice_layers_through_the_cube_call_equal_the_frame_calls(ctx, prec):
    s = S.live_lattice()
    psf = np.stack([s['psf'], np.roll(s['psf'], 1, axis=0)], axis=1)
    cube = np.stack([s['image'], 2.0 * s['image'][::-1, ::-1] + 1.0])
    var = np.stack([s['var'], 4.0 * s['var'][::-1, ::-1]])
    ls = np.array([[0.0, 0.0], [0.13, -0.21]])
    for batch in (0, 1):
        rows, head, resid = ctx.fit_cube_psf(cube, psf, s['origin'], var=var, shift=s['shift'], layer_shift=ls,
                                             psf_index=s['index'], radius=S.LATTICE_RADIUS, max_iter=MAX_ITER, tol=TOL,
                                             layer_batch=batch, return_residual=True)
        for l in range(2):
            want = ctx.fit_frame_psf(np.ascontiguousarray(cube[l]), np.ascontiguousarray(psf[:, l]), s['origin'],
                                     var=np.ascontiguousarray(var[l]), shift=s['shift'] + ls[l], psf_index=s['index'],
                                     radius=S.LATTICE_RADIUS, max_iter=MAX_ITER, tol=TOL, return_residual=True)
            assert _same(rows[l], want[0]) and _same(head[l], want[1]) and _same(resid[l], want[2]), (batch, l)
            assert head[l, 6] == 1089 and head[l, 7] in (0, 1)
    assert head[0, 7] == 0


# ---- 3 and 4. the long frame and the tile-count frames
def _wide_scene(name):
    if name == 'long':
        s = S.long_frame()
        return s, s, S.LONG_RADIUS
    return S.tile_frame(name), S.tile_render_scene(name), S.TILE_RADIUS


WIDE = ['long'] + sorted(S.TILE_FRAMES)


@pytest.mark.parametrize('name', WIDE)
@pytest.mark.parametrize('prec', PRECS)
def test_wide_frame_fit_against_the_sparse_yardstick(ctx, prec, name):
    s, _, radius = _wide_scene(name)
    ref = S.fit_reference(name, s, radius)
    b = F.bounds(ref, TOL, MAX_ITER)
    rows, head, resid = _fit(ctx, s, radius, return_residual=True)
    _record('%s_%s' % (name, prec), _check_against(rows, head, ref, b))
    assert np.array_equal(np.isnan(resid), np.isnan(s['image']))
    inside = S.footprints(s['image'].shape, s['origin'])
    assert _same(resid[~inside], s['image'][~inside])


@pytest.mark.parametrize('name', WIDE)
@pytest.mark.parametrize('prec', PRECS)
def test_wide_frame_render_against_the_yardstick(ctx, prec, name):
    _, s, _ = _wide_scene(name)
    inside = S.footprints(s['image'].shape, s['origin'])
    nan = np.isnan(s['image'])
    for subtract in (False, True) if name != 'long' else (False,):
        want, npix, Sm = S.render_reference(name, s, subtract)
        got, rows = _render(ctx, s, subtract=subtract, return_status=True)
        assert np.array_equal(np.isnan(got), nan)                              # NaN stays NaN and poisons nothing
        worst = float(np.max(np.abs(got - want)[~nan] / Sm[~nan]))
        record_margin('frame_span', **{'render_%s_%s_%s' % (name, prec, 'sub' if subtract else 'add'): worst / PARITY})
        assert worst <= PARITY
        assert _same(got[~inside], s['image'][~inside])                        # outside every footprint: image_in's bits
        assert np.array_equal(rows[:, 1], npix) and np.all(rows[:, 0] == 0) and np.all(npix > 0)


@pytest.mark.parametrize('prec', PRECS)
def test_long_frame_find_against_the_yardstick(ctx, prec):
    s = S.long_frame()
    ref = S.find_reference('long', s, **S.LONG_FIND)
    got = raw_find(ctx, s['image'], s['psf'][0], s['var'], max_stars=64, want_map=False, **S.LONG_FIND)
    worst = assert_parity(got, ref, 'long frame', with_map=False)
    record_margin('frame_span', **{'find_long_%s' % prec: worst})


# ---- 5. the finder frames
@pytest.mark.parametrize('name', sorted(S.FINDER_FRAMES))
@pytest.mark.parametrize('prec', PRECS)
def test_finder_frames_full_parity(ctx, prec, name):
    s = S.finder_frame(name)
    ref = S.find_reference(name, s, **S.FINDER)
    got = raw_find(ctx, s['image'], s['psf'], s['var'], max_stars=256, **S.FINDER)
    worst = assert_parity(got, ref, name)
    record_margin('frame_span', **{'find_%s_%s' % (name, prec): worst})


@pytest.mark.parametrize('prec', PRECS)
def test_max_stars_cutting_inside_the_second_chunk(ctx, prec):
    name = '257x128'
    s = S.finder_frame(name)
    ref = S.find_reference(name, s, **S.FINDER)
    segs = np.array([S.segment(S.FINDER_FRAMES[name], i) for i in ref['index']])
    cap = int(np.count_nonzero(segs < S.SEGS)) + 1
    assert cap < ref['count']
    full = raw_find(ctx, s['image'], s['psf'], s['var'], max_stars=256, **S.FINDER)
    got = raw_find(ctx, s['image'], s['psf'], s['var'], max_stars=cap, **S.FINDER)          # (canaries: raw_find)
    assert got['count'] == ref['count'] == full['count'] and len(got['rows']) == cap
    assert _same(got['rows'], full['rows'][:cap]) and np.array_equal(got['origin'], full['origin'][:cap])
    assert np.array_equal(got['origin'], ref['origin'][:cap])                        # the first max_stars in pixel order
    bound = FR.row_bounds(ref)[:cap]
    assert np.all(np.abs(got['rows'][:, :5] - ref['rows'][:cap, :5]) <= bound[:, :5])
    assert S.segment(S.FINDER_FRAMES[name], ref['index'][cap - 1]) >= S.SEGS


@pytest.mark.parametrize('prec', PRECS)
def test_more_peaks_than_the_rows_kernel_has_blocks(ctx, prec):
    s = S.noise_frame()
    ref = S.find_reference('noise', s, **S.NOISE_FIND)
    assert ref['count'] > S.ROWBLOCKS
    got = raw_find(ctx, s['image'], s['psf'], s['var'], max_stars=1 << 14, **S.NOISE_FIND)
    worst = assert_parity(got, ref, 'noise frame')
    record_margin('frame_span', **{'find_noise_%s' % prec: worst})


# ---- 6. the deep cube
@pytest.mark.parametrize('prec', PRECS)
def test_deep_cube_layers_equal_the_frame_calls(ctx, prec):
    c = S.deep_cube()
    nl = S.DEEP_NL
    want = {}
    for l in (0, S.STEP - 1, S.STEP):
        image, psf, origin, a = K.layer_call(c, l)
        want[l] = ctx.fit_frame_psf(image, psf, origin, radius=S.DEEP_RADIUS, return_residual=True, **a)
    for batch in (0, S.STEP, S.STEP + 1):
        rows, head, resid = ctx.fit_cube_psf(c['cube'], c['psf'], c['origin'], var=c['var'], shift=c['shift'],
                                             layer_shift=c['layer_shift'], psf_index=c['index'], radius=S.DEEP_RADIUS,
                                             layer_batch=batch, return_residual=True)
        assert rows.shape == (nl, 2, 8) and head.shape == (nl, 8)
        for l, w in want.items():
            assert _same(rows[l], w[0]) and _same(head[l], w[1]) and _same(resid[l], w[2]), (batch, l)
        # the NaN layer as section 2 of test_gpu_cube_fit.py states it; every other layer is fitted
        l = S.DEEP_NAN_LAYER
        assert head[l, 7] == 2 and head[l, 6] == 0 and head[l, 4] == 0 and not head[l, :3].any()
        assert set(rows[l, :, 7]) == {2.0} and not rows[l, :, :7].any()
        assert np.all(np.isnan(resid[l])) and np.array_equal(np.isnan(resid), np.isnan(c['cube']))
        assert np.all(head[:l, 7] == 0) and np.all(head[:l, 6] == 2) and np.all(rows[:l, :, 7] == 0)
        assert np.all(head[:l, 4] >= 1) and np.all(np.isfinite(rows)) and np.all(np.isfinite(head))
    # and layer 1023 is the yardstick's: the bit equality above ties the cube call to a checked frame call
    l = S.STEP - 1
    ref = F.solve(c['cube'][l], c['var'][l], np.ascontiguousarray(c['psf'][:, l]), c['index'], c['origin'],
                  c['shift'] + c['layer_shift'][l], S.DEEP_RADIUS, True)
    _record('deep_%s' % prec, _check_against(want[l][0], want[l][1], ref, F.bounds(ref, TOL, MAX_ITER)))


@pytest.mark.parametrize('prec', PRECS)
def test_deep_cube_free_without_outer_steps_is_the_held_solve(ctx, prec):
    """k_cf_step's loops over 1025 layers.  With max_outer = 0 the call is its opening solve with the positions held:
    one least-squares problem over all live layers with one stop test, so the scaled solution over ALL layers'
    unknowns is held to frame_fit_ref.bounds of the joint system (frame_span_cases.deep_joint_reference), the
    integer columns to the per-layer yardsticks.  (Not the converged parity of section 1 of test_gpu_cube_free.py:
    see the module docstring.)"""
    c = S.deep_cube()
    joint = S.deep_joint_reference()
    b = F.bounds(joint, TOL, MAX_ITER)
    rows, pos, shifts, head, call = ctx.fit_cube_psf_free(c['cube'], c['psf'], c['origin'], var=c['var'],
                                                          shift=c['shift'], layer_shift=c['layer_shift'],
                                                          psf_index=c['index'], radius=S.DEEP_RADIUS, background=True,
                                                          max_iter=MAX_ITER, tol=TOL, max_outer=0)
    assert rows.shape == (S.DEEP_NL, 2, 8) and head.shape == (S.DEEP_NL, 8) and call.shape == (8,)
    x = []
    for l, ref in zip(joint['live'], joint['layers']):
        np.testing.assert_array_equal(rows[l, :, 7], ref['status'])
        np.testing.assert_array_equal(rows[l, :, 5], ref['ndisc'])
        assert (head[l, 3], head[l, 6], head[l, 7]) == (ref['nomega'], ref['nacc'], 0), l
        x += [rows[l, 0, 0], rows[l, 1, 0], head[l, 0]]
    ratio = float(np.linalg.norm((np.array(x) - joint['x']) * np.sqrt(joint['dg']))) / b['y']
    _record('deep_free0_%s' % prec, dict(y=ratio))
    assert ratio <= 1.0
    l = S.DEEP_NAN_LAYER
    assert head[l, 7] == 2 and head[l, 6] == 0 and not head[l, :3].any() and not rows[l, :, :7].any()
    assert set(rows[l, :, 7]) == {2.0}
    # the positions stay, nobody was free, one iteration count for all layers
    assert _same(shifts, c['shift']) and _same(pos[:, :2], c['shift']) and not pos[:, 2:].any()
    assert list(call[2:5]) == [0, 0, 0] and call[6] == 0 and call[7] <= TOL
    live = joint['live']
    assert np.all(head[live, 4] == head[0, 4]) and 1 <= head[0, 4] <= MAX_ITER
    assert abs(call[0] - head[live, 2].sum()) <= (len(live) + 4) * EPS * call[0]
    assert call[1] == sum(r['nomega'] - r['nacc'] - 1 for r in joint['layers'])
