"""Host: every condition the GPU tests of test_gpu_frame_span.py rest on, asserted on the references alone.

1. the blocking constants frame_span_cases names are the ones in the sources.
2. the crossing facts of every scene: the live places of pad(), nu = 1024 and 1025 of the lattice's sub-lists, more than
   1024 partials with disc pixels beyond partial 1024, the tile counts and `per`, the segment counts and the planted
   peaks' segments, more than 8192 peaks, more than 1024 layers.
3. solve_sparse equals solve on frame_fit_ref.scene() and on the 289-star lattice within a tenth of bounds()['y'], the
   statuses and integer columns identical.
4. the live lattice: bounds()['y'] / |y*| <= 1e-6, so that the parity check can fail; the textbook iteration stays
   within MAX_ITER.
5. the finder frames: the discrete answers of find_ref are unambiguous at the accuracy of stat_bounds / row_bounds, the
   rule of test_find_host.py, with no peak left out.
"""
import os
import re

import numpy as np
import pytest

import find_ref as FR
import frame_fit_ref as F
import frame_span_cases as S
import render_ref as Y
from conftest import ROOT

TOL, MAX_ITER = 1e-10, 100


def _src(name):
    return open(os.path.join(ROOT, 'muse_psfr_amd', 'csrc', name)).read()


# ---- 1. the constants
def test_the_constants_are_those_of_the_sources():
    fit, render, find = _src('frame_fit_impl.h'), _src('render.hip'), _src('find.hip')
    assert int(re.search(r'constexpr int kStepThreads = (\d+);', fit).group(1)) == S.STEP
    assert int(re.search(r'constexpr int kChunk = (\d+);', fit).group(1)) == S.CHUNK
    assert int(re.search(r'constexpr int kScanThreads = (\d+);', render).group(1)) == S.SCAN
    m = re.search(r'constexpr int kChunkThreads = (\d+), kThreadSegs = (\d+), kChunkSegs = kChunkThreads \* kThreadSegs;',
                  find)
    assert int(m.group(1)) * int(m.group(2)) == S.SEGS and int(m.group(2)) == 4
    assert int(re.search(r'kRowBlocks = (\d+);', find).group(1)) == S.ROWBLOCKS
    assert int(re.search(r'constexpr int kTile = (\d+);', find).group(1)) == S.TILE == Y.TILE
    for name in ('frame_free.hip', 'cube_free.hip'):
        assert 'kStepThreads' in _src(name)
    assert int(re.search(r'#define MPSFR_MAX_IMAGE_SIDE\s+(\d+)', open(os.path.join(ROOT, 'include', 'mpsfr.h')).read())
               .group(1)) == S.LONG_FRAME[1]


# ---- 2. the crossing facts
def _padded_cases():
    import cube_fit_cases as K
    r, f, c = Y.scene(), F.scene(), K.cube()
    return [('render', r, ('origin', 'shift', 'scale', 'index'), r['image'].shape, 1),
            ('frame', f, ('origin', 'shift', 'index'), f['image'].shape, 2),
            ('cube', dict(c, image=c['cube'][0]), ('origin', 'shift', 'index'), c['cube'].shape[1:], 3)]


def test_total_means_three_trips_and_no_round_number():
    assert -(-S.TOTAL // S.STEP) == 3 and all(S.TOTAL % m for m in (64, 256, 1024))
    assert {S.STEP - 1, S.STEP, S.STEP + 1, 2 * S.STEP - 1, 2 * S.STEP, S.TOTAL - 1, 0} <= set(S.PLACES)


@pytest.mark.parametrize('case', [0, 1, 2])
def test_pad_keeps_the_live_stars_in_order_on_both_sides_of_every_trip(case):
    name, s, names, shape, seed = _padded_cases()[case]
    p, places = S.pad_scene(s, names, seed)
    n = len(s['origin'])
    assert len(places) == n and np.all(np.diff(places) > 0) and set(S.PLACES) <= set(places.tolist())
    assert all(len(p[k]) == S.TOTAL for k in names) and p['n'] == S.TOTAL
    for k in names:
        assert np.array_equal(p[k][places], s[k]) and p[k].dtype == np.asarray(s[k]).dtype, k
    # every one of the three trips holds live rows (the third has only 53 places: the two fixed ones at least)
    assert all(np.count_nonzero((places // S.STEP) == t) >= 2 for t in range(3))
    assert len(places) == len(S.PLACES) or len(set(places.tolist()) - set(S.PLACES)) == n - len(S.PLACES)
    filler = np.setdiff1d(np.arange(S.TOTAL), places)
    assert np.all(S.off_frame(shape, p['origin'][filler]))
    assert np.all((p['index'][filler] >= 0) & (p['index'][filler] < len(s['psf']))) and len(set(p['index'][filler])) == 4
    assert len({tuple(o) for o in p['origin'][filler]}) > len(filler) // 2          # varied origins
    assert np.all(np.abs(p['origin']) <= F.MAX_ORIGIN) and np.all(np.abs(p['shift'][filler]) <= 0.5)


def test_the_fillers_are_status_one_in_the_yardstick():
    s = F.scene()
    p, places = S.pad_scene(s, ('origin', 'shift', 'index'), 2)
    ref = F.solve_sparse(p['image'], p['var'], p['psf'], p['index'], p['origin'], p['shift'], 8.0, True)
    base = F.scene_reference(True, True, 8.0)
    filler = np.setdiff1d(np.arange(S.TOTAL), places)
    assert np.all(ref['status'][filler] == 1) and np.array_equal(ref['status'][places], base['status'])
    assert np.array_equal(places[base['acc']], ref['acc']) and ref['nomega'] == base['nomega']
    assert np.array_equal(ref['omega'], base['omega'])
    # the constant is the only unknown of a trip of its own only with 1024 stars: here it is element 2101 of the third
    assert S.TOTAL // S.STEP == 2


def test_lattice_sublists_give_1024_and_1025_unknowns():
    for case, nu in (('1023_back', 1024), ('1024_back', 1025), ('1089_back', 1090), ('1089_noback', 1089)):
        s, ref = S.lattice_reference(case)
        m, back = S.LATTICE_CASES[case]
        assert s['n'] == m == ref['nacc'] and np.all(ref['status'] == 0) and ref['nacc'] + (1 if back else 0) == nu
    assert S.lattice_reference('1089_back')[1]['nomega'] == 29673
    # with 1024 stars and the background the constant is the only element of the second trip
    assert S.LATTICE_CASES['1024_back'] == (S.STEP, True)
    assert S.LATTICE_FRAME[0] % S.TILE and S.LATTICE_FRAME[1] % S.TILE


def test_long_frame_has_more_than_1024_partials_and_discs_beyond_them():
    s = S.long_frame()
    ny, nx = S.LONG_FRAME
    assert S.nchunk(S.LONG_FRAME) == 1028 > S.STEP and S.nchunk((ny - 1, nx)) == S.STEP     # 257 rows: the fewest
    assert 256 * nx == S.STEP * S.CHUNK                     # row 256 is the whole of what lies beyond partial 1023
    assert S.ntiles(S.LONG_FRAME) == 9 * 512 == 4608 and S.scan_per(4608) == 5
    ref = S.fit_reference('long', s, S.LONG_RADIUS)
    assert ref['nacc'] == s['n'] == 16 and np.all(ref['status'] == 0)
    ok = F.valid_pixels(s['image'], s['var'])
    beyond, across = 0, 0
    for k in range(s['n']):
        dk = F.disc(S.LONG_FRAME, F.centre(s['origin'][k], s['shift'][k]), S.LONG_RADIUS) & ok
        lin = np.flatnonzero(dk.ravel())
        beyond += int(np.any(lin >= S.STEP * S.CHUNK))
        rows = lin // nx
        across += int(any(len(set(lin[rows == r] // S.CHUNK)) > 1 for r in set(rows)))
    assert beyond >= 2 and across >= 3
    assert np.count_nonzero(ref['omega'].ravel()[S.STEP * S.CHUNK:]) > 50
    X, Yr = s['pos'][:, 1], s['pos'][:, 0]
    for near_x in (0, nx - 1):
        for near_y in (0, ny - 1):
            assert np.any((np.abs(X - near_x) < 3) & (np.abs(Yr - near_y) < 1.5)), (near_y, near_x)
    assert 0.005 < np.isnan(s['image']).mean() < 0.015
    b = F.bounds(ref, TOL, MAX_ITER)
    assert b['y'] / np.linalg.norm(ref['x'] * np.sqrt(ref['dg'])) <= 1e-6
    assert F.pcg(ref, TOL, MAX_ITER)[1] < MAX_ITER


@pytest.mark.parametrize('name', sorted(S.TILE_FRAMES))
def test_tile_frames_have_their_tile_counts_and_footprints(name):
    shape = S.TILE_FRAMES[name]
    nt = S.ntiles(shape)
    assert (nt, S.scan_per(nt)) == {'1024x1024': (1024, 1), '1312x800': (1025, 2)}[name]
    if name == '1312x800':
        assert (-(-shape[0] // S.TILE), -(-shape[1] // S.TILE)) == (41, 25)
        assert -(-nt // S.scan_per(nt)) == 513 <= S.SCAN // 2 + 1          # the upper half of the scan's threads idle
    s = S.tile_frame(name)
    assert s['n'] == 40
    for scene in (s, S.tile_render_scene(name)):
        met = set().union(*(S.tiles_of(shape, o) for o in scene['origin']))
        assert set(S.TILE_TARGETS[name]) <= met and nt - 1 in met and 0 in met
        assert np.all(np.abs(scene['shift']) <= F.MAX_SHIFT)
    ref = S.fit_reference(name, s, S.TILE_RADIUS)
    assert ref['nacc'] == 40
    b = F.bounds(ref, TOL, MAX_ITER)
    assert b['y'] / np.linalg.norm(ref['x'] * np.sqrt(ref['dg'])) <= 1e-6 and F.pcg(ref, TOL, MAX_ITER)[1] < MAX_ITER


def test_deep_cube_has_more_layers_than_the_step_kernel_has_threads():
    c = S.deep_cube()
    nl = c['cube'].shape[0]
    assert nl == S.DEEP_NL == 1025 > S.STEP and c['psf'].shape == (2, nl, 40, 40) and c['cube'].shape[1:] == (12, 12)
    assert np.all(np.isnan(c['cube'][S.DEEP_NAN_LAYER])) and S.DEEP_NAN_LAYER == S.STEP
    assert not np.isnan(c['cube'][:S.DEEP_NAN_LAYER]).any()
    assert len({tuple(v) for v in c['layer_shift']}) == nl                        # varies with the layer
    assert np.all(np.abs(c['shift'][None] + c['layer_shift'][:, None]) <= F.MAX_SHIFT)
    assert np.array_equal(c['psf'][:, 1], np.roll(Y.models(), 1, axis=0)[:2])
    for l in (0, S.STEP - 1):
        ref = F.solve(c['cube'][l], c['var'][l], np.ascontiguousarray(c['psf'][:, l]), c['index'], c['origin'],
                      c['shift'] + c['layer_shift'][l], S.DEEP_RADIUS, True)
        assert ref['nacc'] == 2 and ref['head_status'] == 0


# ---- 3. the sparse yardstick against the dense one
def _agree(dense, sparse):
    b = F.bounds(dense, TOL, MAX_ITER)
    for k in ('status', 'ndisc', 'acc', 'omega'):
        assert np.array_equal(dense[k], sparse[k]), k
    assert (dense['nomega'], dense['nacc'], dense['head_status']) == (sparse['nomega'], sparse['nacc'], sparse['head_status'])
    assert float(np.linalg.norm((dense['x'] - sparse['x']) * np.sqrt(dense['dg']))) <= 0.1 * b['y']
    assert set(dense) <= set(sparse)
    # every other column within the bound bounds() gives it (a tenth for F, as for y); N and |N| entry by entry within
    # the rounding of a sum of NTERM terms that are |N|'s
    acc, nacc = dense['acc'], dense['nacc']
    dg = dense['dg'][:nacc]
    assert np.all(np.abs(sparse['F'][acc] - dense['F'][acc]) <= 0.1 * b['y'] / np.sqrt(dg))
    assert np.all(np.abs(sparse['nkk'][acc] - dense['nkk'][acc]) <= b['nkk_rel'] * dense['nkk'][acc])
    assert np.all(np.abs(sparse['overlap'][acc] - dense['overlap'][acc]) <= b['overlap'])
    assert abs(sparse['chi2'] - dense['chi2']) <= b['chi2']
    rel = b['chi2'] / dense['chi2'] + b['nkk_rel'] + 8 * F.EPS
    np.testing.assert_allclose(sparse['err'][acc], dense['err'][acc], rtol=rel)
    assert abs(sparse['err_b'] - dense['err_b']) <= rel * dense['err_b']
    assert np.all(np.abs(sparse['N'] - dense['N']) <= b['nkk_rel'] * dense['Nabs'])
    assert np.all(np.abs(sparse['Nabs'] - dense['Nabs']) <= b['nkk_rel'] * dense['Nabs'])
    np.testing.assert_array_equal(np.asarray(sparse['A'].todense()), dense['A'])            # the same columns, bit for bit
    # the residual frame on Omega: the difference of the fluxes through |A|, and the rounding of a pixel's sum
    om = dense['omega']
    L = int(np.max(np.count_nonzero(dense['A'][:, :nacc], axis=1)))
    Sm = np.abs(dense['d']) + np.abs(dense['A']) @ np.abs(dense['x'])
    slack = np.abs(dense['A'][:, :nacc]) @ (0.1 * b['y'] / np.sqrt(dg)) + (L + 20) * F.EPS * Sm
    assert np.all(np.abs(sparse['resid'][om] - dense['resid'][om]) <= slack)
    assert np.array_equal(np.isnan(sparse['resid']), np.isnan(dense['resid']))
    # the bounds of the sparse result: the same three terms from the same matrices, and its own reference term
    bs = F.bounds(sparse, TOL, MAX_ITER)
    assert 0 < bs['terms'][3] < 0.1 * b['y']
    for got, want in zip(bs['terms'][:3], b['terms'][:3]):
        assert abs(got - want) <= 1e-6 * want                  # (lmin and |y*| of matrices that agree as above)
    assert bs['nkk_rel'] == b['nkk_rel'] and abs(bs['kappa'] - b['kappa']) <= 1e-6 * b['kappa']


@pytest.mark.parametrize('with_var,background,radius', [(True, True, 8.0), (False, False, 4.0), (True, False, 8.0)])
def test_solve_sparse_equals_solve_on_the_scene(with_var, background, radius):
    s = F.scene()
    sparse = F.solve_sparse(s['image'], s['var'] if with_var else None, s['psf'], s['index'], s['origin'], s['shift'],
                            radius, background)
    _agree(F.scene_reference(with_var, background, radius), sparse)
    assert set(sparse['status']) == {0, 1, 2}


def test_solve_sparse_equals_solve_on_the_289_star_lattice():
    from test_gpu_frame_fit import lattice
    s = lattice()
    args = (s['image'], s['var'], s['psf'], s['index'], s['origin'], s['shift'], 5.0, True)
    _agree(F.solve(*args), F.solve_sparse(*args))


def test_solve_sparse_answers_nothing_fitted_like_solve():
    psf = Y.models()[:1]
    image = np.array([[3.5]])
    a = F.solve(image, None, psf, None, np.array([[-20, -20]]), None, 8.0, True)
    b = F.solve_sparse(image, None, psf, None, np.array([[-20, -20]]), None, 8.0, True)
    assert a['head_status'] == b['head_status'] == 2 and np.array_equal(a['status'], b['status']) and b['nomega'] == 1


# ---- 4. the bounds on the live lattice can fail
@pytest.mark.parametrize('case', sorted(S.LATTICE_CASES))
def test_lattice_bounds_are_tight_and_the_iteration_fits(case):
    s, ref = S.lattice_reference(case)
    b = F.bounds(ref, TOL, MAX_ITER)
    ynorm = float(np.linalg.norm(ref['x'] * np.sqrt(ref['dg'])))
    assert b['y'] / ynorm <= 1e-6
    x, steps, rel = F.pcg(ref, TOL, MAX_ITER)
    assert steps < MAX_ITER and rel <= TOL
    assert float(np.linalg.norm((x - ref['x']) * np.sqrt(ref['dg']))) <= b['y']
    if case == '1089_back':                                               # (every star and the sky modelled)
        z = (ref['F'] - s['flux']) / ref['sigma']
        assert np.abs(z).max() < 6.0                                      # the yardstick finds the truth within its errors


# ---- 5. the finder frames
def unambiguous(ref, sep, thr):
    """The discrete answers of a find_ref result cannot differ in a run whose T lies within stat_bounds of the
    reference's: no finite T within its bound of the threshold, no candidate within the two bounds of any finite T of
    its square, every curvature further from zero than its bound (row_bounds' dcurv) or flagged for a neighbour that is
    not finite, den away from 0 where the window is valid.  Every candidate pixel is compared: none is left out."""
    T = ref['map']
    ny, nx = T.shape
    fin = np.isfinite(T)
    dT = FR.stat_bounds(ref)[0]
    assert np.all(np.isfinite(dT[fin]))
    assert np.all(np.abs(T[fin] - thr) > dT[fin])
    cand = fin & (np.nan_to_num(T, nan=-np.inf) >= thr)
    Tp = np.pad(T, sep, constant_values=np.nan)
    Ep = np.pad(np.where(fin, dT, 0.0), sep, constant_values=0.0)
    compared = 0
    for dy in range(-sep, sep + 1):
        for dx in range(-sep, sep + 1):
            if dy == 0 and dx == 0:
                continue
            other = Tp[sep + dy:sep + dy + ny, sep + dx:sep + dx + nx]
            eo = Ep[sep + dy:sep + dy + ny, sep + dx:sep + dx + nx]
            both = cand & np.isfinite(other)
            assert np.all(np.abs(other[both] - T[both]) > dT[both] + eo[both]), (dy, dx)
            compared += int(both.sum())
    assert compared > 0 and cand.sum() >= ref['count']
    for row, i in zip(ref['rows'], ref['index']):
        Yp, Xp = divmod(int(i), nx)
        for bit, lo, hi in ((1, (Yp - 1, Xp), (Yp + 1, Xp)), (2, (Yp, Xp - 1), (Yp, Xp + 1))):
            inside = all(0 <= p[0] < ny and 0 <= p[1] < nx and np.isfinite(T[p]) for p in (lo, hi))
            if not inside:
                assert int(row[7]) & bit
                continue
            tm, t0, tp = T[lo], T[Yp, Xp], T[hi]
            dcurv = dT[lo] + 2 * dT[Yp, Xp] + dT[hi] + 4 * FR.EPS * (abs(tm) + 2 * abs(t0) + abs(tp))
            assert abs(tm - 2 * t0 + tp) > dcurv, (Yp, Xp, bit)
    den, ok = ref['den'], 2 * ref['nvalid'] > ref['K'].size
    assert np.all(den[ok] > 1e-6 * ref['S'][2][ok])


def _relative_rule(ref, sep, thr):
    """The rule of test_find_host.py as it stands there: 1e-9 relative, more than twenty times the bound of T."""
    T = ref['map']
    fin = np.isfinite(T)
    dT = FR.stat_bounds(ref)[0]
    assert np.all(dT[fin] < 0.05 * 1e-9 * np.maximum(np.abs(T[fin]), thr))
    assert np.all(np.abs(T[fin] - thr) > 1e-9 * np.maximum(np.abs(T[fin]), thr))
    ny, nx = T.shape
    index = np.arange(ny * nx).reshape(ny, nx)
    for i in np.flatnonzero(fin.ravel() & (np.nan_to_num(T.ravel(), nan=-np.inf) >= thr)):
        Yp, Xp = divmod(int(i), nx)
        sl = (slice(max(Yp - sep, 0), Yp + sep + 1), slice(max(Xp - sep, 0), Xp + sep + 1))
        others = np.isfinite(T[sl]) & (index[sl] != i)
        if others.any():
            assert np.min(np.abs(T[sl][others] - T[Yp, Xp])) > 1e-9 * abs(T[Yp, Xp]), (Yp, Xp)
    for row, i in zip(ref['rows'], ref['index']):
        Yp, Xp = divmod(int(i), nx)
        for bit, tm, tp in ((1, T[Yp - 1, Xp] if Yp else np.nan, T[Yp + 1, Xp] if Yp + 1 < ny else np.nan),
                            (2, T[Yp, Xp - 1] if Xp else np.nan, T[Yp, Xp + 1] if Xp + 1 < nx else np.nan)):
            if not int(row[7]) & bit:
                assert tm - 2 * T[Yp, Xp] + tp < -1e-3 * T[Yp, Xp], (Yp, Xp, bit)


@pytest.mark.parametrize('name', sorted(S.FINDER_FRAMES))
def test_finder_frames_cross_the_chunk_of_1024_segments(name):
    shape = S.FINDER_FRAMES[name]
    assert S.nseg(shape) == {'256x128': 1024, '257x128': 1028}[name]
    assert -(-S.nseg(shape) // S.SEGS) == {'256x128': 1, '257x128': 2}[name]
    s = S.finder_frame(name)
    assert s['image'].shape == shape
    ref = S.find_reference(name, s, **S.FINDER)
    segs = [S.segment(shape, i) for i in ref['index']]
    rows = ref['index'] // shape[1]
    assert S.SEGS - 1 in segs                               # the last segment of chunk 0: row 255, columns 96 .. 127
    assert {254, 255} <= set(rows.tolist()) and ref['count'] >= len(s['pos']) - 1
    if name == '257x128':
        assert S.SEGS in segs and 256 in rows               # the first segment of chunk 1, in its first thread
        assert S.nseg(shape) - S.SEGS == 4                  # four segments: one thread of chunk 1
        before = int(np.count_nonzero(np.array(segs) < S.SEGS))
        assert 0 < before < ref['count']                    # a max_stars of before + 1 cuts inside chunk 1
        assert ref['count'] - before >= 2
    unambiguous(ref, S.FINDER['sep'], S.FINDER['threshold'])
    _relative_rule(ref, S.FINDER['sep'], S.FINDER['threshold'])


def test_noise_frame_has_more_peaks_than_the_rows_kernel_has_blocks():
    s = S.noise_frame()
    ref = S.find_reference('noise', s, **S.NOISE_FIND)
    assert ref['count'] > S.ROWBLOCKS and ref['count'] == len(ref['rows']) == len(ref['index'])
    assert np.nanmin(ref['map']) > S.NOISE_FIND['threshold'] and np.all(s['var'] == 1.0)
    unambiguous(ref, S.NOISE_FIND['sep'], S.NOISE_FIND['threshold'])
    bound = FR.row_bounds(ref)
    assert np.all(np.isfinite(bound)) and np.all(np.isfinite(ref['rows'][:, :5]))


def test_long_frame_finder_answers_are_unambiguous():
    s = S.long_frame()
    ref = S.find_reference('long', s, **S.LONG_FIND)
    assert ref['count'] == s['n']                                            # every star and nothing else
    near = np.abs(ref['rows'][:, None, :2] - s['pos'][None]).max(axis=2).min(axis=1)
    assert near.max() < 1.0
    # three finder chunks of 1024 segments would do for 230 x 300; this frame has 257 x 512 segments: 129 chunks
    assert -(-S.nseg(S.LONG_FRAME) // S.SEGS) == 129
    unambiguous(ref, S.LONG_FIND['sep'], S.LONG_FIND['threshold'])
    _relative_rule(ref, S.LONG_FIND['sep'], S.LONG_FIND['threshold'])


def test_deep_cube_joint_bound_is_tight_and_the_iteration_fits():
    joint = S.deep_joint_reference()
    assert len(joint['live']) == S.STEP and len(joint['x']) == 3 * S.STEP and S.DEEP_NAN_LAYER not in joint['live']
    assert all(r['nacc'] == 2 and r['head_status'] == 0 for r in joint['layers'])
    b = F.bounds(joint, TOL, MAX_ITER)
    assert b['y'] / float(np.linalg.norm(joint['x'] * np.sqrt(joint['dg']))) <= 1e-6
    x, steps, rel = F.pcg(joint, TOL, MAX_ITER)
    assert steps < MAX_ITER and float(np.linalg.norm((x - joint['x']) * np.sqrt(joint['dg']))) <= b['y']
