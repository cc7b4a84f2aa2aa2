"""CPU: the NumPy rules of the per-wavelength stage's work plan (tests/mf_plan_ref.py) on the oracle's own planes.

The oracle's structure functions of three rows of tests/test_gpu_stage_b.py (sharp, broad, a coherent plateau just
below the floor tier) at 128^2 and 256^2 with four directions, rounded to fp32 as the library stores them; the
minima and the block maxima of the telescope OTF made in NumPy.  The four directions are four tasks for the rule of
k_mf_prep (one direction per stamp) and four directions of one task for k_vkeep / k_peak_floor.

 * the rule (R) satisfies the guarantee (G) on every row and every rung of the tier_eps ladder;
 * the yardstick shown to see: every mutation of the rule the comparison of tests/test_gpu_mf_plan.py is meant to
   catch is reported, at the blocks, words or items it moves and nowhere else;
 * the ladder of tier_eps the GPU test runs is fixed here (LADDER), with the classes it reaches.
"""
import copy
import functools

import numpy as np
import pytest

import mf_plan_ref as P
import psfr_oracle as O
import stage_b_ref as R
from muse_psfr_amd.synthetic import grid_pixscale

ROWS = {'sharp': (0.4, 0.95, 29.0), 'broad': (1.6, 0.30, 9.0), 'plateau': (0.6, 0.5, 15.0)}
# (No rung of the ladder sits at a boundary: the reference leaves out no (task, wavelength) on these planes.)
LADDER = P.LADDER
PRUNE_EPS = 1e-9
NL = 7


@functools.lru_cache(maxsize=None)
def _telescope(dim):
    """The library's `tel` (1 at the origin, exactly 0 outside the support) and `tlb` from the oracle's OTF."""
    tel = R.transposed_half_plane(O.telescope_otf(dim), dim)[0] * dim * dim
    tel = np.where(tel > 1e-9, tel, 0.0).astype(np.float32).astype(np.float64)
    h1, nks, nmt, _ = P.geometry(dim)
    pad = np.zeros((nmt * P.MTL, dim))
    pad[:h1] = tel
    with np.errstate(divide='ignore'):
        tlb = np.log2(pad.reshape(nmt, P.MTL, nks, P.KBL).max(axis=(1, 3))).astype(np.float32)
    return tel, tlb


@functools.lru_cache(maxsize=None)
def _plane(dim, row):
    see, gl, l0 = ROWS[row]
    psd = R.model_psd(dim, see, gl, l0, npl=2)
    d0 = R.transposed_half_plane(np.array([O.structure_function0(p) for p in psd]), dim)
    d0 = d0.astype(np.float32).astype(np.float64)
    d0.setflags(write=False)
    return d0


def _lb(dim, scramble=False):
    lb = R.wavelength_set(dim, grid_pixscale(dim), NL)
    return lb[np.random.default_rng(NL).permutation(NL)] if scramble else lb


@functools.lru_cache(maxsize=None)
def _ref(dim, row, tier_eps, mutate='', lines=False, scramble=False):
    """(R) on a plane: (par, plan).  lines: the block minima from per-line minima (the `dlin` path)."""
    d0 = _plane(dim, row)
    tel, tlb = _telescope(dim)
    par = P.host_par(dim, _lb(dim, scramble), tier_eps=tier_eps, prune_eps=PRUNE_EPS)
    pl = P.peak_lines(dim)
    if lines:
        dlin = np.maximum(d0, 0).reshape(d0.shape[:-1] + (dim // 32, 32)).min(axis=-1)
        dmin = P.block_minima_of_lines(dlin, overrun=mutate == 'last m-tile over 16 lines')
    else:
        dmin = P.plane_minima(d0)[1]
    return par, P.plan(par, dmin, tlb, d0[:, :pl], tel[:pl], mutate=mutate)


def _class_of(e, tk, tm):
    """0 dropped, 1 mid, 2 full per block, straight from the thresholds."""
    keep = e > tk[:, :, None, None]
    return keep.astype(int) + (keep & (e > tm[:, :, None, None]))


def _own_places(findings):
    return {f[1:5] for f in findings if f[0] == 'own'}


def _moved_blocks(ref, mut):
    a = _class_of(ref['e'], ref['thr_keep'], ref['thr_mid'])
    b = _class_of(mut['e'], mut['thr_keep'], mut['thr_mid'])
    return {tuple(int(i) for i in ix) for ix in zip(*np.nonzero(a != b))}


@pytest.mark.parametrize('dim', [128, 256])
@pytest.mark.parametrize('row', list(ROWS))
def test_the_rule_satisfies_the_guarantee(dim, row):
    d0 = _plane(dim, row)
    tel, _ = _telescope(dim)
    for te in LADDER + (0.0, float('inf')):
        par, ref = _ref(dim, row, te)
        bad = P.guarantee_blocks(ref['own'], ref['e'], par, d0, tel, PRUNE_EPS, te)
        assert not bad, (dim, row, te, bad[:3])
        blocks, pairs = P.exemptions(ref)
        assert blocks.mean() <= 1e-3 and pairs.mean() <= 0.05, (dim, row, te, blocks.sum(), pairs.sum())
        found, stats = P.compare_plan(ref, ref)
        assert not found and stats['blocks'] == blocks.size


def test_the_ladder_reaches_every_class():
    """Every class the GPU test asserts, on these planes alone -- but a (task, group) with several sweeps: 128^2 has one
    sweep, and at 256^2 the second holds the single line dim/2, outside the telescope's support; 512^2 has three."""
    seen, classes = set(), set()
    for dim in (128, 256):
        for row in ROWS:
            for te in LADDER:
                _, ref = _ref(dim, row, te)
                seen |= P.coverage(ref)
                classes |= {i[0] for i in ref['items']}
    print('classes of the ladder:', sorted(seen), 'item classes', sorted(classes))
    assert seen >= {'no lowering', 'keep lowered', 'clamp', 'mid lowered', 'no mid block', 'no tier block', 'one sweep',
                    'sweep without work'}
    assert len(classes) >= 3


def test_without_a_budget_the_thresholds_are_nominal():
    for te, floor in ((0.0, False), (float('inf'), True)):
        par, ref = _ref(256, 'plateau', te)
        want_keep = max(par.thr_eps, np.float32(-29.01)) if floor else par.thr_eps
        assert np.all(ref['thr_keep'] == want_keep)
        assert np.all(ref['thr_mid'] == (np.float32(-18.01) if floor else np.float32(-1e30)))
        assert not any(i['budget'] for r in ref['info'] for i in r)


MOVED = [('keep+2', 256, 'plateau', 1e-8), ('keep-2', 256, 'plateau', 1e-8), ('no clamp', 128, 'plateau', 1e-12),
         ('mid 2^-10', 256, 'plateau', 1e-8), ('S one line fewer', 256, 'plateau', 1.36e-7)]


@pytest.mark.parametrize('mutate,dim,row,te', MOVED)
def test_a_moved_threshold_is_reported_at_its_blocks(mutate, dim, row, te):
    """thr_keep two bits higher / lower, no clamp at the eps threshold, the mid mass counted at 2^-10, S over one line
    fewer: the comparison names exactly the blocks that change tier."""
    _, ref = _ref(dim, row, te)
    _, mut = _ref(dim, row, te, mutate)
    want = _moved_blocks(ref, mut)
    found, _ = P.compare_plan(ref, mut)
    print(mutate, len(want), 'blocks move;', len(found), 'findings')
    assert want and _own_places(found) == want
    if mutate == 'no clamp':
        assert any(i['clamp'] for r in ref['info'] for i in r)
        assert np.any(mut['thr_keep'] < mut['par'].thr_eps)


def test_the_last_m_tile_over_16_lines_is_reported_there():
    """The last m-tile has one line of its own; fifteen more are the next task's first lines, whose D is near 0."""
    dim = 256
    _, ref = _ref(dim, 'broad', 4e-6, lines=True)
    _, same = _ref(dim, 'broad', 4e-6)
    assert not P.compare_plan(ref, same)[0]                      # the two minima paths agree
    # (the support of the telescope OTF ends below line dim/2: give the last m-tile something to keep)
    tel, tlb = _telescope(dim)
    d0 = _plane(dim, 'broad')
    par = P.host_par(dim, _lb(dim), prune_eps=PRUNE_EPS)
    tlb = tlb.copy()
    tlb[-1] = tlb[0]
    dlin = np.maximum(d0, 0).reshape(d0.shape[:-1] + (dim // 32, 32)).min(axis=-1)
    pl = P.peak_lines(dim)
    ref = P.plan(par, P.block_minima_of_lines(dlin), tlb, d0[:, :pl], tel[:pl])
    mut = P.plan(par, P.block_minima_of_lines(dlin, overrun=True), tlb, d0[:, :pl], tel[:pl])
    places = _own_places(P.compare_plan(ref, mut)[0])
    assert places and {p[2] for p in places} == {P.geometry(dim)[2] - 1}


def test_a_wavelength_missing_from_uni_is_reported():
    _, ref = _ref(256, 'plateau', 4e-6)
    any_ = ref['own'].any(axis=3)
    per, ngr = ref['par'].per, ref['par'].ngr
    last = list(range((ngr - 1) * per, NL))
    assert ngr == 2 and 1 < len(last) < per + 1
    alone = {l: any_[:, l] & ~any_[:, [k for k in last if k != l]].any(axis=1) for l in last}
    lost = max(last, key=lambda l: alone[l].sum())                       # the wavelength that keeps most on its own
    _, mut = _ref(256, 'plateau', 4e-6, 'uni misses wavelength %d' % lost)
    found, _ = P.compare_plan(ref, mut)
    want = {(int(t), ngr - 1, int(mt), int(ks)) for t, mt, ks in zip(*np.nonzero(alone[lost]))}
    assert want and {f[1:] for f in found if f[0] == 'uni'} == want
    assert not _own_places(found)


def test_ksum_over_seven_m_tiles_is_reported():
    _, ref = _ref(128, 'broad', 4e-6)
    got = copy.deepcopy(ref)
    got['ksum'] = P.derive(ref['own'], ref['par'].per, ref['par'].ngr, 'ksum over 7 m-tiles')['ksum']
    want = {tuple(int(i) for i in ix) for ix in zip(*np.nonzero(got['ksum'] != ref['ksum']))}
    found, _ = P.compare_plan(ref, got)
    assert want and {f[1:] for f in found if f[0] == 'ksum'} == want and len(found) == len(want)


def test_items_dropped_duplicated_and_misfiled_are_reported():
    _, ref = _ref(256, 'plateau', 4e-6)
    item = ref['items'][len(ref['items']) // 2]

    def run(items):
        got = copy.deepcopy(ref)
        got['items'] = sorted(items)
        got['sched'] = np.bincount([i[0] for i in items], minlength=P.NLISTS)
        return P.compare_plan(ref, got)[0]
    rest = [i for i in ref['items'] if i != item]
    assert run(rest) == [('sched', item[0]), ('item missing', item)]
    assert run(ref['items'] + [item]) == [('sched', item[0]), ('item extra', item)]
    moved = (item[0] + 1,) + item[1:]
    assert run(rest + [moved]) == [('sched', item[0]), ('sched', item[0] + 1), ('item missing', item),
                                   ('item extra', moved)]


def _lines_case(dim, row, scramble):
    d0 = _plane(dim, row)[None]                                          # one task, four directions
    tel, _ = _telescope(dim)
    par = P.host_par(dim, _lb(dim, scramble), ndb=4, prune_eps=PRUNE_EPS, mf2=False)
    return par, P.plane_minima(d0)[0], d0, tel


@pytest.mark.parametrize('dim', [128, 256])
@pytest.mark.parametrize('row', list(ROWS))
def test_the_line_rule_satisfies_the_guarantee(dim, row):
    for scramble in (False, True):
        par, dline, d0, tel = _lines_case(dim, row, scramble)
        vk, out = P.vkeep(par, dline, tel)
        assert not out.any() and vk.min() >= 1 and np.all(np.diff(vk, axis=1) >= 0)
        assert not P.guarantee_lines(vk, par, d0, tel, 0.5 * PRUNE_EPS)


def test_a_pair_bounded_by_its_shorter_wavelength_is_reported():
    par, dline, d0, tel = _lines_case(256, 'plateau', False)
    vk, out = P.vkeep(par, dline, tel)
    mut, _ = P.vkeep(par, dline, tel, mutate='shorter wavelength')
    want = [(0, p) for p in range(vk.shape[1]) if mut[0, p] != vk[0, p]]
    assert want and P.compare_vkeep(vk, out, mut) == want
    assert (NL - 1) // 2 not in [p for _, p in want]                     # (the last pair is a single wavelength)


def test_a_missing_running_maximum_is_reported():
    par, dline, d0, tel = _lines_case(256, 'plateau', True)
    vk, out = P.vkeep(par, dline, tel)
    mut, _ = P.vkeep(par, dline, tel, mutate='no running maximum')
    want = [(0, p) for p in range(vk.shape[1]) if mut[0, p] != vk[0, p]]
    assert want and P.compare_vkeep(vk, out, mut) == want


def test_task_order():
    vk = np.array([[3, 7], [5, 9], [1, 7], [2, 12], [9, 9]])
    assert P.task_order(vk).tolist() == [3, 1, 4, 0, 2]


@pytest.mark.parametrize('dim', [128, 256])
def test_the_task_floor_satisfies_the_guarantee(dim):
    tel, tlb = _telescope(dim)
    pl = P.peak_lines(dim)
    for row in ROWS:
        d0 = _plane(dim, row)[None]
        for te in LADDER:
            par = P.host_par(dim, _lb(dim), ndb=4, prune_eps=PRUNE_EPS, tier_eps=te, mf2=False)
            thrf = P.peak_floor(par, d0[:, :, :pl], tel[:pl], dim)
            assert thrf[0] <= float(par.thr_floor)
            dminb = P.plane_minima(d0)[1].min(axis=1)
            assert not P.guarantee_floor(thrf, par, dminb, tlb, d0, tel, te)
