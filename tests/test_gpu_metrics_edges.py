"""GPU: k_stamp_metrics (mpsfr_stamp_metrics) on the hard inputs of tests/metrics_cases.py, both precision contexts,
against the mpmath yardstick tests/metrics_mp_ref.py (60 digits; tests/test_metrics_cases_host.py pins it).

Classes: (a) circles that cut 64, 128 and up to 156 pixels (the third pass over the queue); (b) single pixels at the
cell boundaries of the 8 x 8 lane map, with known values; (c) centres on a pixel corner, edge and centre with circles
through lattice corners and tangent to grid lines, boxes on pixel edges and centres, 16 + 16 + 16 parameters at once;
(d) ties of the peak; (e) amplitudes 2^+-30 .. 2^+-600; (f) stamps of mixed signs and a ladder of sum|I| / flux;
(g) centres up to the limit of 100 px, every fraction in one call and one fraction per call, and centres beyond it.

What is asserted
* flux, centroid, EE_k and SQE_k against the yardstick: per class the smaller of the project's 1e-10 and four times
  the worst error measured on an MI355X, rounded up to one digit (metrics_cases.BOUNDS), times sum|I| / |flux| of the
  stamp.  Measured value and bound go to record_margin('metrics_edges', ...) and profiles/metrics_margins.json.
* the known values of an impulse and the zeros of an aperture that does not reach the stamp: exactly (1e-15 where pi
  enters).  Peak, its position and the status: exactly.
* R_k: finite and inside [0, r_max] on every row; with status 0 the yardstick's |EE(R_k) - f_k| <= 1e-12, the number of
  include/mpsfr.h -- a condition, not a measurement.  A row with status 1 is not held to it; how many there are, and
  from which rung of the ladder on, is recorded.
* (e): every field but flux and peak bit for bit the row at 2^0, flux and peak scaled exactly.  The argument: a
  power of two scales every stamp value, hence every partial sum and every product with an area, without rounding
  (nothing leaves the normal range: the smallest product is an area of ~1e-17 times a pixel of ~1e-5 x 2^-600);
  iflux = 1 / flux scales by the inverse power exactly; EE = sum x iflux, the centroid sum_p / flux, the Newton step
  g / (d x iflux) and the start radius sqrt(f flux / (pi max(peak, flux / 1600))) are ratios of quantities that scale
  alike.  No step of the kernel squares a stamp value, so 2^+-600 stays clear of overflow: the whole range is
  scale-free.
* one case per class through device pointers: bit for bit the host form.
"""
import numpy as np
import pytest

import metrics_cases as Cs
from conftest import record_margin

pytestmark = pytest.mark.gpu

PRECS = ['mixed', 'f64']
HEAD = Cs.HEAD


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


def run(ctx, c):
    rows = ctx.stamp_metrics(c['stamps'], c['radii'], c['boxes'], c['fracs'], centers=c['centers'])
    assert rows.shape == (len(c['stamps']), HEAD + len(c['radii']) + len(c['boxes']) + len(c['fracs']))
    return rows


def run_device(ctx, c):
    import torch
    dev = torch.device('cuda:0')
    n = len(c['stamps'])
    ts = torch.from_numpy(c['stamps']).to(dev)
    tc = None if c['centers'] is None else torch.from_numpy(c['centers']).to(dev)
    to = torch.full((n, HEAD + len(c['radii']) + len(c['boxes']) + len(c['fracs'])), -1.0, dtype=torch.float64,
                    device=dev)
    torch.cuda.synchronize()
    ctx.stamp_metrics_device(n, ts.data_ptr(), to.data_ptr(), c['radii'], c['boxes'], c['fracs'],
                             centers_ptr=None if tc is None else tc.data_ptr())
    ctx.sync()
    return to.cpu().numpy()


def check_head(c, rows, status=(0.0,)):
    for k, (s, row) in enumerate(zip(c['stamps'], rows)):
        assert (row[1], row[2], row[3]) == Cs.expected_peak(s), (c['name'], k, row[:HEAD])
        assert row[6] in status and row[7] == 0.0, (c['name'], k, row[:HEAD])


def check_against_the_yardstick(c, rows, prec):
    """Measures, records and asserts the energies and the centroid; asserts the promise on the radii of the rows with
    status 0.  Returns the measurement."""
    m = Cs.measure(c, rows)
    cls, bound = c['cls'], Cs.BOUNDS[c['cls']]
    worst = {k: float(np.max(m[k])) if m[k].size else 0.0 for k in ('flux', 'centroid', 'ee', 'sqe')}
    print('metrics_edges %s %s: %s' % (c['name'], prec, worst))
    record_margin('metrics_edges', **{'%s_%s' % (cls, k): v for k, v in worst.items()})
    record_margin('metrics_edges', **{'%s_%s_bound' % (cls, k): bound[k] for k in worst})
    for k, v in worst.items():
        assert v <= bound[k], (c['name'], k, v, bound[k])
    nf = len(c['fracs'])
    if nf:
        ree = rows[:, rows.shape[1] - nf:]
        assert np.all(np.isfinite(ree)) and np.all(ree >= 0.0) and np.all(ree <= m['rmax'][:, None]), (c['name'], ree)
        ok = rows[:, 6] == 0.0
        root0 = float(np.max(m['root'][ok])) if np.any(ok) else 0.0
        print('metrics_edges %s %s: |EE(R) - f| %.3g over %d rows with status 0, %d rows with status 1'
              % (c['name'], prec, root0, ok.sum(), (~ok).sum()))
        record_margin('metrics_edges', **{'%s_root_status0' % cls: root0})
        assert root0 <= Cs.ROOT_PROMISE, (c['name'], m['root'], rows[:, 6])
    return m


# ---- (a) cut counts
@pytest.mark.parametrize('prec', PRECS)
def test_circles_that_cut_64_128_and_156_pixels(ctx, prec):
    for c in Cs.cases_a():
        rows = run(ctx, c)
        check_head(c, rows)
        check_against_the_yardstick(c, rows, prec)


# ---- (b) impulses
@pytest.mark.parametrize('prec', PRECS)
def test_impulses_at_the_cell_boundaries(ctx, prec):
    near, mid, _ = Cs.cases_b()
    for c in (near, mid):
        rows = run(ctx, c)
        check_head(c, rows)
        check_against_the_yardstick(c, rows, prec)


@pytest.mark.parametrize('prec', PRECS)
def test_impulses_about_their_own_centroid(ctx, prec):
    own = Cs.cases_b()[2]
    rows = run(ctx, own)
    Cs.check_own_impulses(own, rows)
    check_against_the_yardstick(own, rows, prec)


# ---- (c) exact geometry
@pytest.mark.parametrize('prec', PRECS)
def test_corner_edge_and_pixel_centres(ctx, prec):
    for c in Cs.cases_c():
        rows = run(ctx, c)
        check_head(c, rows)
        check_against_the_yardstick(c, rows, prec)
    # a constant stamp about the corner centre: a box with integer side holds s^2 pixels exactly
    c1 = Cs.cases_c()[0]
    rows = run(ctx, c1)
    sq = Cs.split(c1, rows[0])[1]
    assert np.all(np.abs(sq - np.array(c1['boxes']) ** 2 / 1600.0) <= 1e-15), sq


@pytest.mark.parametrize('prec', PRECS)
def test_sixteen_radii_boxes_and_fractions_at_once(ctx, prec):
    c = Cs.case_full()
    rows = run(ctx, c)
    check_head(c, rows)
    check_against_the_yardstick(c, rows, prec)
    # every third of the row is what a call with that third alone gives
    st = c['stamps']
    assert np.array_equal(ctx.stamp_metrics(st, c['radii'], (), ())[:, HEAD:], rows[:, HEAD:HEAD + 16])
    assert np.array_equal(ctx.stamp_metrics(st, (), c['boxes'], ())[:, HEAD:], rows[:, HEAD + 16:HEAD + 32])
    assert np.array_equal(ctx.stamp_metrics(st, (), (), c['fracs'])[:, HEAD:], rows[:, HEAD + 32:])


# ---- (d) peak ties
@pytest.mark.parametrize('prec', PRECS)
def test_peak_ties_and_refused_stamps(ctx, prec):
    c, want = Cs.cases_d()
    rows = run(ctx, c)
    Cs.check_peaks(rows, want)
    assert np.all(np.isnan(rows[5:, 4:6]))                                # (no centroid of a refused stamp)
    good = dict(c, stamps=c['stamps'][:5])
    check_against_the_yardstick(good, rows[:5], prec)


# ---- (e) amplitudes
@pytest.mark.parametrize('prec', PRECS)
def test_powers_of_two_scale_flux_and_peak_only(ctx, prec):
    base = {}
    for k, c in Cs.cases_e():
        rows = run(ctx, c)
        kind = c['name'].rsplit('_', 1)[0]
        if k == 0:
            base[kind] = rows
            assert np.all(rows[:, 6] == 0.0) and np.all(np.isfinite(rows))
            continue
        ref = base[kind]
        assert np.array_equal(rows[:, 2:], ref[:, 2:]), (c['name'], np.nonzero(rows[:, 2:] != ref[:, 2:]))
        assert np.array_equal(rows[:, :2], ref[:, :2] * 2.0 ** k), c['name']


# ---- (f) mixed signs
@pytest.mark.parametrize('prec', PRECS)
def test_stamps_of_mixed_signs(ctx, prec):
    signs, two, ladder = Cs.cases_f()
    nflag = 0
    for c in (signs, two):
        rows = run(ctx, c)
        check_head(c, rows, status=(0.0, 1.0))
        check_against_the_yardstick(c, rows, prec)
        nflag += int((rows[:, 6] == 1.0).sum())
    # two impulses, f = 1/2: EE is flat at 1/2 between sqrt(1/2) and the second pixel
    r_half = Cs.split(two, rows[0])[2][two['fracs'].index(0.5)]
    assert 0.7 <= r_half <= 9.5, r_half                  # (from where the circle holds the first pixel to within 2e-14)
    rows = run(ctx, ladder)
    check_head(ladder, rows, status=(0.0, 1.0))
    check_against_the_yardstick(ladder, rows, prec)
    flagged = [g for g, row in zip(Cs.LADDER, rows) if row[6] == 1.0]
    print('metrics_edges ladder %s: status 1 at the rungs %s; %d rows of the other stamps' % (prec, flagged, nflag))
    assert flagged, 'no rung of the ladder was flagged: lengthen it'          # (the flag has been seen)
    record_margin('metrics_edges', f_status1_rows=nflag + len(flagged), f_ladder_first_flagged_rung=min(flagged))


# ---- (g) far centres
def _reach(ce):
    """Distance from a centre to the stamp [-0.5, 39.5]^2 in the maximum norm and in the Euclidean norm."""
    dp = max(-0.5 - ce[0], ce[0] - 39.5, 0.0)
    dq = max(-0.5 - ce[1], ce[1] - 39.5, 0.0)
    return max(dp, dq), float(np.hypot(dp, dq))


@pytest.mark.parametrize('prec', PRECS)
def test_far_centres(ctx, prec):
    c, refused = Cs.cases_g()
    assert len(c['stamps']) >= 6 and len(refused['stamps']) >= 8
    rows = run(ctx, c)
    check_head(c, rows)                                                    # (within the limit nothing is flagged)
    m = check_against_the_yardstick(c, rows, prec)
    for ce, row, root in zip(c['centers'], rows, m['root']):
        print('metrics_edges far %s: (%g, %g)  |EE(R) - f| %s' % (prec, ce[0], ce[1], ' '.join('%.2g' % x for x in root)))
        dmax, deuc = _reach(ce)
        if deuc > 80.0:
            assert row[HEAD] == 0.0, (ce, row)
        if dmax >= 40.0:
            assert row[HEAD + 1] == 0.0, (ce, row)
    assert np.any(rows[:, HEAD] == 0.0) and np.any(rows[:, HEAD] > 0.0)
    # beyond the limit: refused by the Python layer, status 2 from the kernel
    with pytest.raises(ValueError):
        run(ctx, refused)
    rows = run_device(ctx, refused)
    assert np.all(rows[:, 6] == 2.0) and np.all(np.isnan(rows[:, HEAD:])), rows
    assert np.array_equal(rows[:, 4:6], refused['centers'])


@pytest.mark.parametrize('prec', PRECS)
def test_one_fraction_per_call_up_to_the_centre_limit(ctx, prec):
    """The promise on R_k where it is hardest inside the accepted range, refereed radius by radius: with one fraction
    per call no other fraction can flag the row.  Every row must come back with status 0 (the stamp is non-negative),
    and the worst error must leave the factor 4 to 1e-12 that the limit was chosen for."""
    worst = 0.0
    for c in Cs.cases_g_single():
        rows = run(ctx, c)
        check_head(c, rows)
        m = check_against_the_yardstick(c, rows, prec)
        worst = max(worst, float(np.max(m['root'])))
    print('metrics_edges single fractions %s: worst |EE(R) - f| %.3g' % (prec, worst))
    record_margin('metrics_edges', g_root_single_fraction=worst)
    assert 4.0 * worst <= Cs.ROOT_PROMISE, worst


# ---- device pointers
@pytest.mark.parametrize('prec', PRECS)
def test_device_pointers_bit_for_bit(ctx, prec):
    g = Cs.cases_g()[0]
    b = Cs.cases_b()[0]
    b = dict(b, stamps=b['stamps'][::5], centers=b['centers'][::5])
    for c in (Cs.cases_a()[1], b, Cs.cases_c()[0], Cs.cases_d()[0], Cs.cases_e()[-1][1], Cs.cases_f()[2], g):
        host, dev = run(ctx, c), run_device(ctx, c)
        assert host.tobytes() == dev.tobytes(), c['name']
