"""CPU: the mpmath yardstick of the energy metrics (tests/metrics_mp_ref.py) and the hard cases (tests/metrics_cases.py)
that tests/test_gpu_metrics_edges.py runs on the kernel.

1. the yardstick against facts that do not depend on it, and against tests/metrics_ref.py where that one is good;
2. the cases hit what they claim: the cut counts 64, 128, beyond 128 and 156, none beyond the queue's 256;
3. a fp64 NumPy model of the kernel's arithmetic (tests/metrics_model.py: sweep, queue in chunks of 64, corner sum,
   maximum ladder) passes the classes (a) to (d) at the bounds the GPU test asserts;
4. the model with one deliberate mistake fails at the cases built for that mistake -- and only there where that can
   be said.  Two remarks on what such a mistake can show:
   * the sign of the near-corner terms AT x0 == 0 (or y0 == 0) cannot matter: that term is the area over a strip of
     width 0, quadrant_area(0, y) = 0 with angle 0.  The kernel takes -1 there; taking +1 gives the same bits
     (test_the_sign_at_x0_zero_is_immaterial).  The mistake that the corner, edge and pixel centres of class (c) do
     catch is the sign where x0 < 0, a pixel that holds the centre's row or column ('sx0');
   * `in` with < sends a pixel whose farthest corner lies on the circle (3-4-5, 5-12-13 from a corner centre) through
     the overlap formula, which returns x y = 1 for it: the energies agree to rounding, what differs is the number of
     queued pixels, which the model reports and the yardstick's exact count pins.
"""
import numpy as np
import pytest

import metrics_cases as Cs
import metrics_model as K
import metrics_mp_ref as Y
import metrics_ref as R

mp = Y.mp


def model_rows(c, edits=(), stamps=None):
    st = c['stamps'] if stamps is None else stamps
    rows, counts = [], []
    for k, s in enumerate(st):
        row, cnt = K.metrics(s, None if c['centers'] is None else c['centers'][k], c['radii'], c['boxes'], c['fracs'],
                             edits, center_max=Cs.CENTER_MAX)
        rows.append(row)
        counts.append(cnt)
    return np.array(rows), counts


def worst(m, keys=('flux', 'centroid', 'ee', 'sqe')):
    return {k: float(np.max(m[k])) if m[k].size else 0.0 for k in keys}


def within_bounds(c, m):
    b = Cs.BOUNDS[c['cls']]
    w = worst(m)
    return all(w[k] <= b[k] for k in w) and (not m['root'].size or float(np.max(m['root'])) <= Cs.ROOT_PROMISE)


# ---- 1. the yardstick
@pytest.mark.parametrize('cp,cq,r', [(19.5, 19.5, 0.3), (20.0, 20.0, 0.5), (19.3, 20.1, 13.0), (19.5, 19.5, 19.9),
                                     (19.6027, 19.3256, 19.3314)])
def test_areas_sum_to_the_disc(cp, cq, r):
    a = Y.overlap(cp, cq, r)
    assert all(0 <= x <= 1 for x in a.ravel())
    assert abs(mp.fsum(a.ravel()) - mp.pi * mp.mpf(r) ** 2) <= mp.mpf(10) ** -50


def test_known_areas_of_a_pixel_about_its_own_centre():
    for r in (0.1, 0.25, 0.5):
        a = Y.overlap(7.0, 8.0, r)
        assert abs(a[7, 8] - mp.pi * mp.mpf(r) ** 2) <= mp.mpf(10) ** -50 and mp.fsum(a.ravel()) == a[7, 8]
    for r in (Cs.SQH, 1.0):
        assert Y.overlap(7.0, 8.0, r)[7, 8] == 1                          # (the square of SQH rounds up to above 1/2)
    assert float(Cs.SQH) ** 2 >= 0.5
    # a chord: the circle of radius 0.6 about a pixel's centre leaves four corners outside
    want = mp.pi * mp.mpf(0.6) ** 2 - 4 * (mp.mpf(0.6) ** 2 * mp.acos(0.5 / mp.mpf(0.6))
                                           - 0.5 * mp.sqrt(mp.mpf(0.6) ** 2 - 0.25))
    assert abs(Y.overlap(20.0, 20.0, 0.6)[20, 20] - want) <= mp.mpf(10) ** -50


def test_lattice_corners_on_the_circle_are_decided_exactly():
    """From the corner centre (19.5, 19.5) the circle of radius 5 passes through the lattice points (+-3, +-4),
    (+-4, +-3), (+-5, 0), (0, +-5): the pixel inside such a point is whole, the pixel beyond it is empty."""
    c = Y.circle(19.5, 19.5, 5.0)
    for sp in (1, -1):
        for sq in (1, -1):
            for a, b in ((3, 4), (4, 3)):
                # relative cell [a - 1, a] x [b - 1, b] (far corner (a, b)) and [a, a + 1] x [b, b + 1] (near corner)
                pin = (19.5 + sp * (a - 0.5), 19.5 + sq * (b - 0.5))
                pout = (19.5 + sp * (a + 0.5), 19.5 + sq * (b + 0.5))
                assert c.whole[int(pin[0]), int(pin[1])] and not c.cut[int(pin[0]), int(pin[1])]
                assert not c.whole[int(pout[0]), int(pout[1])] and not c.cut[int(pout[0]), int(pout[1])]
    assert c.area(22, 23) == 1 and c.area(23, 24) == 0
    # radius 13 (5-12-13)
    c = Y.circle(19.5, 19.5, 13.0)
    assert c.whole[19 + 5, 19 + 12] and not c.cut[19 + 6, 19 + 13] and not c.whole[19 + 6, 19 + 13]
    # a circle tangent to grid lines from a pixel centre: r = 2.5 about (20, 20) touches the lines at 17.5 and 22.5
    c = Y.circle(20.0, 20.0, 2.5)
    assert not c.cut[17, 20] and not c.whole[17, 20] and c.cut[18, 20]


@pytest.mark.parametrize('cp,cq,r', [(19.3, 20.1, 0.3), (19.5, 19.5, 1.0), (19.3, 20.1, 13.0), (20.0, 20.0, 5.0),
                                     (19.6027, 19.3256, 19.3314), (18.1, 21.4, 2.5)])
def test_agrees_with_the_fp64_reference_near_the_stamp(cp, cq, r):
    """metrics_ref's own error: a difference of antiderivatives of magnitude r^2, each a few roundings -- 16 eps r^2
    (measured against this yardstick: 9.2e-14 at r = 13, 16 eps r^2 = 6e-13)."""
    a = Y.overlap(cp, cq, r)
    d = np.abs(np.array(a, dtype=float) - R.circle_overlap(cp, cq, r)).max()
    assert d <= 16 * 2.0 ** -52 * max(1.0, r * r), d


def test_energies_and_centroid_agree_with_the_fp64_reference():
    st = Cs.case_full()['stamps'][0]
    c = R.centroid(st)
    cy = Y.centroid(st)
    assert abs(float(cy[0]) - c[0]) <= 1e-13 and abs(float(cy[1]) - c[1]) <= 1e-13
    for r in (0.8, 7.3, 22.0):
        assert abs(float(Y.EE(st, c, r)) - R.EE(st, c, r)) <= 1e-12
    for s in (0.3, 3.7, 17.0, 55.0):
        assert abs(float(Y.SQE(st, c, s)) - R.SQE(st, c, s)) <= 1e-13
    assert abs(float(Y.r_max(c)) - R.r_max(c)) <= 1e-13
    assert Y.EE(st, c, 80.0) == 1 and Y.SQE(st, c, 80.0) == 1


# ---- 2. the cases hit what they claim
def test_cut_counts_of_class_a():
    seen = []
    for (cp, cq), r, n in Cs.CUT_COUNTS:
        assert int(Cs.cut_mask(cp, cq, r).sum()) == n, (cp, cq, r)          # the kernel's compares, in fp64
        assert Y.cut_count(cp, cq, r) == n, (cp, cq, r)                     # decided exactly
        seen.append(n)
    assert 64 in seen and 128 in seen and max(seen) == 156 and sum(n > 128 for n in seen) >= 4
    # the cases carry these radii, and the ring stamp is 1 on the 156 cut pixels of r = 19.9
    radii = {(tuple(c['centers'][0]), r) for c in Cs.cases_a() for r in c['radii']}
    assert radii == {(c, r) for c, r, _ in Cs.CUT_COUNTS}
    ring = Cs.stamps_a()[3]
    assert ring.sum() == 156.0 and set(np.unique(ring)) == {0.0, 1.0}
    assert all(s.sum() > 0.0 for s in Cs.stamps_a())


def test_no_case_exceeds_the_queue():
    most = 0
    for c in Cs.all_cases():
        if c['centers'] is None:
            continue
        for ce in {tuple(x) for x in c['centers']}:
            for r in c['radii']:
                most = max(most, int(Cs.cut_mask(ce[0], ce[1], r).sum()))
    assert most == 156 <= K.MQ


def test_the_cases_are_what_they_claim():
    pos = Cs.impulse_positions()
    assert len(pos) == 404 and {(i, j) for i in (0, 7, 8, 39) for j in range(40)} <= set(pos)
    assert {(i, j) for j in (0, 7, 8, 39) for i in range(40)} <= set(pos)
    lad = Cs.ladder_stamps()
    for s, g in zip(lad, Cs.LADDER):
        assert abs(Y.abs_ratio(s) / g - 1.0) <= 1e-3 and s.sum() > 0.0, g
    f = Cs.cases_f()
    assert f[0]['stamps'][0].min() < 0.0 < f[0]['stamps'][0].sum()
    ee = [float(Y.EE(f[0]['stamps'][0], (19.8, 19.4), r)) for r in (3.0, 6.0, 12.0, 28.0)]
    assert ee[1] > 1.0 and ee[1] > ee[2] > ee[3] >= 1.0 - 1e-12                 # not monotone
    two = f[1]['stamps'][0]
    assert all(Y.EE(two, (15.0, 12.0), r) == mp.mpf(1) / 2 for r in (Cs.SQH, 5.0, 9.0))   # flat at 1/2
    assert Y.EE(two, (15.0, 12.0), 11.0) == 1
    far = Cs.far_centers()
    assert [d for d, k, _ in far if k == 'row'] == Cs.G_DIST == [d for d, k, _ in far if k == 'diag']
    ok, refused = Cs.cases_g()
    assert np.all(Cs.in_range(ok['centers'])) and not np.any(Cs.in_range(refused['centers']))
    assert [19.5, -100.0] in ok['centers'].tolist() and [-71.5, -71.5] in ok['centers'].tolist()
    assert len(ok['stamps']) + len(refused['stamps']) == len(far)
    lim = Cs.limit_centers()
    assert np.all(Cs.in_range(lim)) and [-100.0, -100.0] in lim.tolist() and len(Cs.cases_g_single()) == 8
    assert all(len(c['fracs']) == 1 for c in Cs.cases_g_single())
    from muse_psfr_amd import _lib
    assert _lib.METRIC_CENTER_MAX == Cs.CENTER_MAX == K.K_CENTER_MAX
    _lib.metric_centers(ok['centers'], len(ok['centers']))
    for ce in refused['centers']:
        with pytest.raises(ValueError):
            _lib.metric_centers(ce[None, :], 1)
    assert len(Cs.case_full()['radii']) == len(Cs.case_full()['boxes']) == len(Cs.case_full()['fracs']) == 16
    for k, c in Cs.cases_e():
        f = c['stamps'].reshape(4, -1).sum(axis=1)
        assert np.all(np.isfinite(f)) and np.all(f > 2.0 ** -1000)


# ---- 3. the model of the kernel passes
_MODEL = {}


def model_measure(c):
    if c['name'] not in _MODEL:
        rows, counts = model_rows(c)
        _MODEL[c['name']] = (rows, counts, Cs.measure(c, rows))
    return _MODEL[c['name']]


ABC = Cs.cases_a() + Cs.cases_b() + Cs.cases_c() + [Cs.case_full()]


@pytest.mark.parametrize('c', ABC, ids=[c['name'] for c in ABC])
def test_the_model_passes(c):
    rows, counts, m = model_measure(c)
    assert np.all(rows[:, 6] == 0.0)
    for s, row in zip(c['stamps'], rows):
        assert (row[1], row[2], row[3]) == Cs.expected_peak(s)
    assert within_bounds(c, m), (worst(m), m['root'].max() if m['root'].size else None)
    if c['centers'] is not None:                                          # the queue counts are the exact counts
        for k, cnt in enumerate(counts):
            assert cnt == [Y.cut_count(c['centers'][k][0], c['centers'][k][1], r) for r in c['radii']]


def test_the_model_gives_the_known_values_of_an_impulse():
    c = Cs.cases_b()[2]
    rows = model_measure(c)[0]
    Cs.check_own_impulses(c, rows)


def test_the_model_finds_the_peaks_of_class_d():
    c, want = Cs.cases_d()
    rows, _ = model_rows(c)
    Cs.check_peaks(rows, want)


# ---- 4. the edited models fail where they should
def test_a_queue_stopped_at_128_fails_beyond_128():
    for c in Cs.cases_a():
        rows, _ = model_rows(c, ('queue128',))
        m = Cs.measure(c, rows)
        for j, r in enumerate(c['radii']):
            n = Y.cut_count(c['centers'][0][0], c['centers'][0][1], r)
            bad = m['ee'][:, j] > Cs.BOUNDS['a']['ee']
            # (the ring stamp is 0 on the cut pixels of every radius but its own, 19.9)
            hit = np.all(bad[:3]) and (bad[3] or r != 19.9)
            assert hit if n > 128 else not np.any(bad), (c['name'], r, n, m['ee'][:, j])


def test_a_queue_position_off_by_one_at_64_fails_beyond_64():
    for c in Cs.cases_a():
        rows, _ = model_rows(c, ('pos64',))
        m = Cs.measure(c, rows)
        for j, r in enumerate(c['radii']):
            n = Y.cut_count(c['centers'][0][0], c['centers'][0][1], r)
            bad = m['ee'][:, j] > Cs.BOUNDS['a']['ee']
            # (entry 63 is lost, entry 64 read from a stale slot: every stamp but one that is 0 on both pixels)
            assert bad.sum() >= 3 if n > 64 else not np.any(bad), (c['name'], r, n, m['ee'][:, j])


def test_a_wrong_sign_of_the_near_corner_terms_fails_on_the_centres_of_class_c():
    c = Cs.cases_c()[0]
    rows, _ = model_rows(c, ('sx0',))
    m = Cs.measure(c, rows)
    bad = m['ee'] > Cs.BOUNDS['c']['ee']
    # centres on an edge (19.5, 20) and on a pixel (20, 20): rows 2 .. 5; the corner centre has no pixel with x0 < 0
    assert not np.any(bad[:2]) and np.all(bad[2:].any(axis=1))
    j = c['radii'].index(0.3)                                             # the circle inside one pixel
    assert np.all(bad[4:, j])


def test_the_sign_at_x0_zero_is_immaterial():
    c = Cs.cases_c()[0]
    rows, _ = model_rows(c)
    rows1, _ = model_rows(c, ('sx_at_zero',))
    assert np.array_equal(rows, rows1)
    x0 = np.abs(np.arange(40.0)[None, :] - np.array(Cs.C_CENTERS)[:, 1:2]) - 0.5
    assert np.any(x0 == 0.0)                                              # (the class has pixels with x0 == 0)


def test_in_with_less_than_queues_the_pixels_with_a_corner_on_the_circle():
    c = Cs.cases_c()[0]
    rows, counts = model_rows(c, ('in_lt',))
    j5, j13 = c['radii'].index(5.0), c['radii'].index(13.0)
    exact = [Y.cut_count(19.5, 19.5, r) for r in c['radii']]
    # the 8 pixels whose farthest corner is (+-3, +-4), (+-4, +-3) or (+-5, +-12), (+-12, +-5)
    assert counts[0][j5] == exact[j5] + 8 and counts[0][j13] == exact[j13] + 8
    assert within_bounds(c, Cs.measure(c, rows))                          # (the energies do not see it)


def test_a_tie_rule_by_lane_and_swapped_slots_fail():
    c, want = Cs.cases_d()
    rows, _ = model_rows(c, ('tie_lane',))
    got = [(r[2], r[3]) for r in rows]
    assert got[2] == (8.0, 0.0) and got[2] != want[2][1:3]                # (7, 8) is in lane 56, (8, 0) in lane 0
    with pytest.raises(AssertionError):
        Cs.check_peaks(rows, want)
    b = Cs.cases_b()[0]                                                   # (the centre is beside the pixel)
    pos = Cs.impulse_positions()
    sub = [k for k, (i, j) in enumerate(pos) if i // 8 != j // 8][:40]
    bs = dict(b, stamps=b['stamps'][sub], centers=b['centers'][sub])
    rows, _ = model_rows(bs, ('slot_swap',))
    m = Cs.measure(bs, rows)
    assert np.all((m['ee'] > Cs.BOUNDS['b']['ee']).any(axis=1))
    assert all((r[2], r[3]) != pos[k] for r, k in zip(rows, sub))
