"""GPU: the work plan of the per-wavelength stage against its rules in float64 (tests/mf_plan_ref.py).

Every test makes one small call, fetches what the planning kernels read (`dphi0`, `tel`, `tlb`, `dlin` or the minima of
k_dmin, the host's thresholds `mf_par`) and what they wrote, and holds the latter

  (R) word for word to the rule evaluated in NumPy: the minima of k_dmin / k_vkeep exactly; the masks, k-step words,
      sweep bits, list lengths and the multiset of work items of k_mf_prep; `vkeep`, `order`, `thrf`;
  (G) to what include/mpsfr.h promises of the parts of the half plane a plan leaves out, from `dphi0` and `tel`
      alone, with no tolerance.

Two conditions leave something out of (R), both derived, not measured: a block whose bound lies
within one float32 ulp of a threshold it is compared with, and a (task, wavelength) whose mass / budget comes within
1e-4 of 1 at a step (float32 sums of at most 47 terms, v_exp_f32 and the float32 S give under 1e-5).  At most 0.1 % of
a case's blocks and one (task, wavelength) in twenty may be left out; a case above that fails.  `vkeep` likewise: a
pair whose sum comes within 1e-4 of thr_sum at its boundary line.

`thrf`: log2 of a float32 sum through v_log_f32 has no bound derived from the code.  Measured on an MI355X
(profiles/mf_plan_margins.json): |thrf - fp64| <= 3.52e-6 bits, one float32 ulp of the value; asserted 2e-5 (four
times, rounded up), under the condition of 1e-3 bits, which moves the mass the floor drops by less than 0.1 %.
"""
import numpy as np
import pytest

import mf_plan_ref as P
import stage_b_ref as R
from conftest import record_margin, H
from muse_psfr_amd.synthetic import grid_pixscale

pytestmark = pytest.mark.gpu

PRUNE_EPS, TIER_EPS = 1e-9, 4e-6                 # the library's defaults
THRF_TOL, THRF_CONDITION = 2e-5, 1e-3            # bits
NEAR = 1e-4

#        seeing  GL    L0    three LGS   (the rows of tests/test_gpu_stage_b.py)
ROWS = [(0.4, 0.95, 29.0, 0),        # sharp
        (1.6, 0.30, 9.0, 0),         # broad
        (0.6, 0.5, 15.0, 0),         # the rows with the coherent plateau just below the floor tier
        (0.5, 0.9, 20.0, 0),
        (0.3, 0.5, 29.0, 1),
        (0.9, 0.9, 11.0, 0),
        (0.4, 0.95, 29.0, 0),        # (= the first: two equal keys for k_task_order)
        (1.0, 0.7, 25.0, 0),
        (0.45, 0.93, 28.5, 1)]


def test_the_thrf_tolerance_is_inside_its_condition():
    assert THRF_TOL <= THRF_CONDITION


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _rows(ntask):
    rows = {1: ROWS[:1], 2: ROWS[:2], 3: ROWS[:3], 7: ROWS[:7], 9: ROWS}[ntask]
    return tuple(np.array([r[k] for r in rows]) for k in range(4))


def _wavelengths(dim, nl, scramble=False):
    if nl == 2:
        lb = R.wavelength_set(dim, grid_pixscale(dim), 3)[[0, 2]]
    else:
        lb = R.wavelength_set(dim, grid_pixscale(dim), nl)
    return lb[np.random.default_rng(nl).permutation(nl)] if scramble else lb


def _context(api, dim, opts=(), precision='mixed'):
    ctx = api.Context(dim=dim, pixscale=grid_pixscale(dim), precision=precision)
    ctx.set_option('streams', 1)                 # one lane, one chunk: debug_fetch hands out the whole call
    for k, v in opts:
        ctx.set_option(k, v)
    return ctx


def _fails(ctx, what):
    with pytest.raises(Exception):
        ctx.debug_fetch(what, (1,))


# ---- minima ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dim,npl,prec', [(128, 1, 'mixed'), (128, 2, 'mixed'), (512, 1, 'mixed'), (512, 2, 'mixed'),
                                          (128, 1, 'f64'), (128, 2, 'f64'), (512, 1, 'f64'), (512, 2, 'f64')])
def test_minima_equal_the_minima_of_the_stored_plane(api, dim, npl, prec):
    """k_dmin (`dline`, `dblk`) and the minimum over the directions of k_vkeep (`dminb`), exactly: a minimum rounds
    nothing (f64 mode: each value rounded down to float first).  stage_a = 0: the full-size transforms, after which
    k_dmin runs on every grid.  One direction in mixed mode is the thin-wave kernel, whose `dminb` are k_dmin's blocks."""
    ntask, ndir = 3, npl * npl
    h1, nks, nmt, _ = P.geometry(dim)
    ctx = _context(api, dim, (('stage_a', 0),), prec)
    try:
        ctx.reconstruct(_wavelengths(dim, 2), *_rows(ntask), H, npsflin=npl)
        d0 = ctx.debug_fetch('dphi0', (ntask, ndir, h1, dim))
        dline = ctx.debug_fetch('dline', (ntask, ndir, h1))
        dblk = ctx.debug_fetch('dblk', (ntask, ndir, nmt, nks))
        if prec == 'mixed':
            dminb = ctx.debug_fetch('dminb', (ntask, nmt, nks))
        else:
            _fails(ctx, 'dminb')
        _fails(ctx, 'dlin')
    finally:
        ctx.close()
    want_line, want_blk = P.plane_minima(d0, f64=prec == 'f64')
    bad = int((dline != want_line).sum()), int((dblk != want_blk).sum())
    print('minima dim %d ndir %d %s: %d lines, %d blocks compared; %d, %d differ' % (
        dim, ndir, prec, dline.size, dblk.size, bad[0], bad[1]))
    assert bad == (0, 0)
    if prec == 'mixed':
        assert np.array_equal(dminb, want_blk.min(axis=1))


# ---- k_mf_prep ---------------------------------------------------------------------------------------------------

def _fetch_plan(ctx, dim, ntask, nl, prune_eps):
    """Everything of the last call of the thin-wave kernel: (par, inputs, fetched plan)."""
    h1, nks, nmt, nsw = P.geometry(dim)
    par = P.parse_par(ctx.debug_fetch('mf_par', (9 + nl,)))
    ngr = par.ngr
    sched = ctx.debug_fetch('mf_sched', (64,))
    got = P.fetched_plan(ctx.debug_fetch('mf_own', (ntask, nl, nmt, 2)), ctx.debug_fetch('mf_uni', (ntask, ngr, nmt)),
                         ctx.debug_fetch('mf_ksum', (ntask, nl, nsw)), ctx.debug_fetch('mf_kuni', (ntask, ngr, nsw)),
                         ctx.debug_fetch('mf_gsw', (ntask, ngr)), sched,
                         ctx.debug_fetch('mf_items', (int(sched.sum()), 5)), nks)
    got['own'] = got['own'].reshape(ntask, nl, nmt, 2, nks)
    inp = dict(d0=ctx.debug_fetch('dphi0', (ntask, 1, h1, dim))[:, 0], tel=ctx.debug_fetch('tel', (h1, dim)),
               tlb=ctx.debug_fetch('tlb', (nmt, nks)), path='none')
    if prune_eps > 0:
        try:
            inp['dmin'] = P.block_minima_of_lines(ctx.debug_fetch('dlin', (ntask, 1, h1, nks))[:, 0])
            inp['path'] = 'dlin'
            _fails(ctx, 'dminb')
        except Exception:
            inp['dmin'] = ctx.debug_fetch('dminb', (ntask, nmt, nks))
            inp['path'] = 'dminb'
    else:
        inp['dmin'] = np.zeros((ntask, nmt, nks))
        _fails(ctx, 'dminb')
    for what in ('vkeep', 'thrf', 'order'):
        _fails(ctx, what)
    return par, inp, got


def _check_plan(label, dim, par, inp, got, prune_eps, tier_eps):
    """(R) and (G) of one call; -> the reference plan."""
    pl = P.peak_lines(dim)
    ref = P.plan(par, inp['dmin'], inp['tlb'], inp['d0'][:, :pl], inp['tel'][:pl], nopr=prune_eps == 0)
    found, st = P.compare_plan(ref, got, NEAR)
    print('mf_plan %-26s dim %4d %-5s tasks %d nl %2d per %d ngr %d: %d blocks, %d left out; %d (task, wavelength), %d '
          'left out; %d items in classes %s; %d findings' % (
              label, dim, inp['path'], got['own'].shape[0], par.c.size, par.per, par.ngr, st['blocks'], st['blocks_out'],
              st['pairs'], st['pairs_out'], len(got['items']), sorted({i[0] for i in got['items']}), len(found)))
    assert st['blocks_out'] <= 1e-3 * st['blocks'] and st['pairs_out'] * 20 <= st['pairs'], (label, st)
    assert not found, (label, len(found), found[:12])
    bad = P.guarantee_blocks(got['own'], ref['e'], par, inp['d0'], inp['tel'], prune_eps, tier_eps, nopr=prune_eps == 0)
    assert not bad, (label, bad[:6])
    return ref


def _run_plan(api, label, dim, ntask, nl, opts=(), scramble=False, path=None):
    o = dict(opts)
    prune_eps, tier_eps = o.get('prune_eps', PRUNE_EPS), o.get('tier_eps', TIER_EPS)
    ctx = _context(api, dim, opts)
    try:
        ctx.reconstruct(_wavelengths(dim, nl, scramble), *_rows(ntask), H)
        par, inp, got = _fetch_plan(ctx, dim, ntask, nl, prune_eps)
    finally:
        ctx.close()
    if path is not None:
        assert inp['path'] == path, (label, inp['path'])
    assert (par.per, par.ngr) == P.groups(nl)
    return _check_plan(label, dim, par, inp, got, prune_eps, tier_eps)


# The smallest shapes that reach each layout: 128^2 (nks 4, nmt 5, one sweep) and 256^2 on k_dmin's block minima, 512^2
# (three sweeps) and above on the line minima of stage A's series form; 1280^2 has nks 40, nmt 41, six sweeps and S over
# two lines; both minima paths on one grid (512^2 with stage_a 0, 128^2 with stage_a 2).  Tasks 1 / 7 / 9; wavelengths
# 1 / 6 / 7 / 13: one group, a full group, two ragged groups (4 + 3), three groups (5 + 5 + 3); one set scrambled.
SHAPES = [(128, 9, 13, (), False, 'dminb'), (256, 7, 7, (), False, 'dminb'), (512, 7, 6, (), False, 'dlin'),
          (512, 1, 1, (), False, 'dlin'), (1024, 1, 3, (), False, 'dlin'), (1280, 2, 3, (), False, 'dlin'),
          (512, 3, 7, (('stage_a', 0),), True, 'dminb'), (128, 3, 7, (('stage_a', 2),), False, 'dlin')]


@pytest.mark.parametrize('dim,ntask,nl,opts,scramble,path', SHAPES)
def test_plan_of_the_thin_wave_kernel(api, dim, ntask, nl, opts, scramble, path):
    ref = _run_plan(api, 'defaults', dim, ntask, nl, opts, scramble, path)
    h1, nks, nmt, nsw = P.geometry(dim)
    assert ref['own'].shape == (ntask, nl, nmt, 2, nks) and ref['kuni'].shape[2] == nsw
    if dim == 1280:
        assert (nks, nmt, nsw, P.peak_lines(dim)) == (40, 41, 6, 2)


@pytest.mark.parametrize('dim', [128, 256, 512])
def test_plan_under_every_option_and_down_the_ladder(api, dim):
    """The sharp, broad and plateau rows with seven wavelengths through one context: the defaults, prune_eps = 0 (every
    block full, every sweep filed), tier_eps = 0 (no tiers) and inf (the nominal thresholds), mf_mid_log2 at, above and
    below mf_floor_log2, and the ladder of tier_eps fixed in tests/test_mf_plan_ref.py.  Over the three grids every way
    through the budget pass occurs (the last grid asserts it)."""
    ntask, nl = 3, 7
    lb = _wavelengths(dim, nl)
    h1, nks, nmt, nsw = P.geometry(dim)
    variants = [('prune_eps 0', (('prune_eps', 0.0),)), ('tier_eps 0', (('tier_eps', 0.0),)),
                ('tier_eps inf', (('tier_eps', float('inf')),)), ('mid at the floor', (('mf_mid_log2', -29.01),)),
                ('mid above', (('mf_mid_log2', -10.0),)), ('mid below the floor', (('mf_mid_log2', -35.0),))]
    variants += [('tier_eps %g' % te, (('tier_eps', te),)) for te in P.LADDER]
    base = {'prune_eps': PRUNE_EPS, 'tier_eps': TIER_EPS, 'mf_mid_log2': -18.01}
    ctx = _context(api, dim)
    try:
        for label, opts in variants:
            o = dict(base, **dict(opts))
            for k, v in o.items():
                ctx.set_option(k, v)
            ctx.reconstruct(lb, *_rows(ntask), H)
            par, inp, got = _fetch_plan(ctx, dim, ntask, nl, o['prune_eps'])
            ref = _check_plan(label, dim, par, inp, got, o['prune_eps'], o['tier_eps'])
            SEEN.update(P.coverage(ref))
            CLASSES.update(i[0] for i in got['items'])
            if label == 'prune_eps 0':
                assert got['own'][:, :, :, 0].all() and not got['own'][:, :, :, 1].any()
                assert np.all(got['gsw'] == (1 << nsw) - 1) and len(got['items']) == ntask * par.ngr * nsw
            if label == 'tier_eps 0':
                assert not got['own'][:, :, :, 1].any() and np.all(ref['thr_keep'] == par.thr_eps)
            if label == 'tier_eps inf':
                assert np.all(ref['thr_keep'] == max(par.thr_eps, par.thr_floor)) and np.all(ref['thr_mid'] == par.thr_mid)
            if label in ('mid at the floor', 'mid below the floor'):
                assert not got['own'][:, :, :, 1].any()
    finally:
        ctx.close()
    DONE.add(dim)
    if DONE >= {128, 256, 512}:
        print('mf_plan classes seen:', sorted(SEEN), 'item classes', sorted(CLASSES))
        assert SEEN >= EVERY_CLASS, sorted(EVERY_CLASS - SEEN)
        assert len(CLASSES) >= 3


SEEN, CLASSES, DONE = set(), set(), set()
EVERY_CLASS = {'no lowering', 'keep lowered', 'clamp', 'mid lowered', 'no mid block', 'no tier block', 'one sweep',
               'several sweeps', 'sweep without work'}


# ---- k_vkeep, k_task_order ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('dim,npl,nl,scramble,opts', [
    (128, 1, 7, False, (('otf_mfma', 0),)), (128, 2, 6, True, (('otf_mfma', 0),)), (256, 1, 13, True, (('mf_kernel', 1),)),
    (256, 2, 7, False, ()), (512, 1, 7, True, (('otf_mfma', 0),)), (512, 1, 2, False, (('mf_kernel', 1),))])
def test_lines_kept_and_task_order(api, dim, npl, nl, scramble, opts):
    """`vkeep` of the FFT form and of the blocked matrix-core kernel (mf_kernel = 1; several directions always) against
    the rule, from the minima k_vkeep read; `order` the stated permutation of nine tasks, two of them with equal keys;
    (G) for the lines each wavelength drops."""
    ntask, ndir = 9, npl * npl
    h1, nks, nmt, _ = P.geometry(dim)
    lb = _wavelengths(dim, nl, scramble)
    mf = dict(opts).get('otf_mfma', 1) != 0
    ctx = _context(api, dim, opts)
    try:
        ctx.reconstruct(lb, *_rows(ntask), H, npsflin=npl)
        par = P.parse_par(ctx.debug_fetch('mf_par', (9 + nl,)))
        d0 = ctx.debug_fetch('dphi0', (ntask, ndir, h1, dim))
        tel = ctx.debug_fetch('tel', (h1, dim))
        dline = ctx.debug_fetch('dline', (ntask, ndir, h1))
        dblk = ctx.debug_fetch('dblk', (ntask, ndir, nmt, nks))
        got = ctx.debug_fetch('vkeep', (ntask, (nl + 1) // 2))
        if mf:
            dminb = ctx.debug_fetch('dminb', (ntask, nmt, nks))
            order = ctx.debug_fetch('order', (ntask,))
        else:
            _fails(ctx, 'dminb')
            _fails(ctx, 'order')
        _fails(ctx, 'mf_own')
    finally:
        ctx.close()
    share = (0.5 if mf else 1.0) * PRUNE_EPS
    assert float(par.thr_sum) == float(np.float32(share / (2.0 * dim * ndir)))
    want_line, want_blk = P.plane_minima(d0)
    # (the series form skips the pieces of a line outside the telescope's support: they hold 0 in `dphi0` and do not
    # enter a minimum -- tests/test_gpu_series_minima.py holds those minima; here they are what k_vkeep read)
    if dim >= 512 or (dim == 256 and ndir > 1):
        assert np.all(dline >= want_line) and np.all(dblk >= want_blk)
    else:
        assert np.array_equal(dline, want_line) and np.array_equal(dblk, want_blk)
    want, out = P.vkeep(par, dline, tel, NEAR)
    bad = P.compare_vkeep(want, out, got)
    print('vkeep dim %d ndir %d nl %d %s: %d pairs, %d left out, %d differ' % (dim, ndir, nl, dict(opts), out.size,
                                                                             out.sum(), len(bad)))
    assert out.sum() * 20 <= out.size
    assert not bad, (bad[:8], want[bad[0][0]], got[bad[0][0]])
    assert np.all(np.diff(got, axis=1) >= 0)
    assert not P.guarantee_lines(got.astype(int), par, d0, tel, share)
    if mf:
        assert np.array_equal(dminb, dblk.min(axis=1))
        assert np.array_equal(order, P.task_order(got))
        assert got[0, -1] == got[6, -1] and list(order).index(0) < list(order).index(6)


# ---- k_peak_floor ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dim,npl', [(256, 2), (256, 3), (512, 2)])
def test_floor_per_task(api, dim, npl):
    ntask, nl, ndir = 3, 7, npl * npl
    h1, nks, nmt, _ = P.geometry(dim)
    pl = P.peak_lines(dim)
    ctx = _context(api, dim)
    try:
        for te in (TIER_EPS, 1e-9):
            ctx.set_option('tier_eps', te)
            ctx.reconstruct(_wavelengths(dim, nl), *_rows(ntask), H, npsflin=npl)
            par = P.parse_par(ctx.debug_fetch('mf_par', (9 + nl,)))
            d0 = ctx.debug_fetch('dphi0', (ntask, ndir, h1, dim))
            tel = ctx.debug_fetch('tel', (h1, dim))
            thrf = ctx.debug_fetch('thrf', (ntask,))
            dminb = ctx.debug_fetch('dminb', (ntask, nmt, nks))
            tlb = ctx.debug_fetch('tlb', (nmt, nks))
            want = P.peak_floor(par, d0[:, :, :pl], tel[:pl], dim)
            err = np.abs(thrf - want).max()
            print('thrf dim %d ndir %d tier_eps %g: %s  fp64 %s  |diff| %.3e bits' % (dim, ndir, te, thrf, want, err))
            record_margin('mf_plan', thrf_bits=err)
            assert abs(float(par.c2min) / float(min(P.c2_of(c) for c in par.c)) - 1) < 2e-7
            assert err <= THRF_TOL, (dim, npl, te, err)
            assert not P.guarantee_floor(thrf, par, dminb, tlb, d0, tel, te)
        ctx.set_option('tier_eps', float('inf'))
        ctx.reconstruct(_wavelengths(dim, nl), *_rows(ntask), H, npsflin=npl)
        _fails(ctx, 'thrf')
    finally:
        ctx.close()
