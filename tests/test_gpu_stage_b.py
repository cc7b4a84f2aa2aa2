"""GPU: the per-wavelength stage alone -- the stored structure function D_phi0 of a call in, the 40 x 40 stamps
before the convolutions out -- against the fp64 reference of the same operation (tests/stage_b_ref.py), for every
implementation of the stage:

  mfma2   k_otf_mfma2, the thin-wave matrix-core kernel for one direction (the default)
  mfma1   k_otf_mfma1<false> (mf_kernel = 1), one direction
  multi   k_otf_mfma1<true> with k_peak_floor: several directions
  fft     the mixed LDS-FFT form (otf_mfma = 0: k_otf_rowfft / k_colpass), one and four directions
  f64     the f64 form of the same two kernels, one and four directions

Every check runs the stage, fetches `dphi0` and `pre` of the same call and compares `pre` with
stamps_from_dphi0(dphi0): every stamp, every pixel, max |diff| / peak of the reference stamp.  The reference reads the
plane the kernel read (fp32 values in mixed mode), so stage A's error is not in the figure; it uses the oracle's
exact telescope OTF, so the library's log2 tel table is.

Two modes per mixed variant: (A) prune_eps = 0, which also switches the precision tiers off -- the arithmetic alone,
held to TOL_A; (B) the library's defaults, held per stamp to what include/mpsfr.h promises for eps = prune_eps +
tier_eps, eps (1 + 1600 peak / sum), on top of TOL_A.

TOL_A is 4 x the worst error measured on an MI355X per variant (profiles/stage_b_margins.json), rounded up to one
significant digit -- the error is rounding noise over ~1e5 terms and the inputs are a sample -- or the variant's
condition where that is smaller.  Conditions that do not depend on the measurement: matrix-core variants <= 2e-6 (five times the split-fp16 arithmetic model of
tests/test_stage_b_ref.py), fft <= 5e-6 (the bound the two mixed forms have against each other), f64 <= 1e-11.
"""
import functools

import numpy as np
import pytest

import psfr_oracle as O
import stage_b_ref as R
from conftest import record_margin, H
from muse_psfr_amd.synthetic import grid_pixscale

pytestmark = pytest.mark.gpu

# Worst measured (profiles/stage_b_margins.json): mfma2 6.4e-7, mfma1 5.6e-7, multi 5.8e-7, fft 1.13e-6, f64 7.4e-13.
# Times 4, rounded up: 3e-6, 3e-6, 3e-6, 5e-6, 3e-12.  For the three matrix-core variants that is above their
# condition, so the condition is what they are held to (a factor 3.1 - 3.6 over the measurement instead of 4): their
# error is the size of the split-fp16 model's own (6.4e-7 at 256^2 x 4 on the CPU), not a defect.
TOL_A = {'mfma2': 2e-6, 'mfma1': 2e-6, 'multi': 2e-6, 'fft': 5e-6, 'f64': 3e-12}
CONDITION = {'mfma2': 2e-6, 'mfma1': 2e-6, 'multi': 2e-6, 'fft': 5e-6, 'f64': 1e-11}
TIER_EPS, PRUNE_EPS = 4.0e-6, 1.0e-9        # the library's defaults (include/mpsfr.h)

OPTS = {'mfma2': {}, 'mfma1': {'mf_kernel': 1}, 'multi': {}, 'fft': {'otf_mfma': 0}, 'f64': {}}
# (variant, mode): every mixed variant in both modes, f64 with its defaults
VM = [(v, m) for v in ('mfma2', 'mfma1', 'fft') for m in 'AB'] + [('f64', 'default')]
VM_MF = [(v, m) for v in ('mfma2', 'mfma1') for m in 'AB']


def test_tolerances_are_inside_their_conditions():
    for v, c in CONDITION.items():
        assert TOL_A[v] <= c, v


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _context(api, dim, variant, mode, extra=()):
    ctx = api.Context(dim=dim, pixscale=grid_pixscale(dim), precision='f64' if variant == 'f64' else 'mixed')
    ctx.set_option('streams', 1)                     # one lane, one chunk: debug_fetch hands out the whole call
    for k, v in OPTS[variant].items():
        ctx.set_option(k, v)
    if mode == 'A':
        ctx.set_option('prune_eps', 0.0)             # (tiers = prune && ...: no tiers either)
    for k, v in extra:
        ctx.set_option(k, v)
    return ctx


def _compare(label, variant, mode, dim, lb, d0, pre, check=True):
    """d0 [ntask][ndir][dim/2+1][dim], pre [ntask][nl][40][40] of one call -> the errors [ntask][nl]; asserted
    against the mode's bound, the worst recorded."""
    ps = grid_pixscale(dim)
    assert np.all(np.isfinite(d0)) and np.all(np.isfinite(pre))
    # (stage A skips no line and stores no placeholder value: the plane is the structure function throughout, and
    # nothing stage A gives away is in the figure)
    assert d0.max() < 1e29, (label, d0.max())
    assert d0.min() >= -1e-6 * d0.max(), (label, d0.min(), d0.max())      # the kernel's clamp of D at 0 cannot matter
    err = np.empty(pre.shape[:2])
    bound = np.empty(pre.shape[:2])
    for k in range(pre.shape[0]):
        ref = R.stamps_from_dphi0(d0[k], dim, lb, ps)
        err[k] = R.stamp_errors(pre[k], ref)
        peak = ref.max(axis=(1, 2))
        bound[k] = TOL_A[variant]
        if mode == 'B':
            bound[k] += (PRUNE_EPS + TIER_EPS) * (1 + 1600 * peak / ref.sum(axis=(1, 2)))
    print('stage_b %-34s %-5s %-7s dim %4d  tasks %d  nl %2d  ndir %2d  worst %.3e  (bound %.3e)'
          % (label, variant, mode, dim, pre.shape[0], pre.shape[1], d0.shape[1], err.max(), bound.flat[err.argmax()]))
    if check:
        record_margin('stage_b_alone', **{'%s_%s' % (variant, mode): err.max()})
        assert np.all(err <= bound), (label, variant, mode, float(err.max()), float((err / bound).max()))
    return err


# ---- model rows through `reconstruct` ---------------------------------------------------------------------------

#        seeing  GL    L0    three LGS
ROWS = [(0.4, 0.95, 29.0, 0),        # sharp
        (1.6, 0.30, 9.0, 0),         # broad
        (0.6, 0.5, 15.0, 0),         # the five rows with the coherent plateau just below the floor tier
        (0.5, 0.9, 20.0, 0),
        (0.3, 0.5, 29.0, 1),
        (0.9, 0.9, 11.0, 0),
        (0.4, 0.95, 29.0, 0),
        (1.0, 0.7, 25.0, 0),
        (0.45, 0.93, 28.5, 1)]


def _rows(ntask):
    rows = {1: ROWS[:1], 3: [ROWS[0], ROWS[1], ROWS[4]], 7: ROWS[:7], 9: ROWS}[ntask]
    return tuple(np.array([r[k] for r in rows]) for k in range(4))


def _wavelengths(api, dim, nl, scramble=False):
    """nl wavelengths for this grid: the shortest it admits first, then (from four on) npix_crop a multiple of 40,
    just above it, 930 nm, and an even fill between."""
    lb = R.wavelength_set(dim, grid_pixscale(dim), nl)
    return lb[np.random.default_rng(nl).permutation(nl)] if scramble else lb


def _run_rows(api, label, variant, mode, dim, ntask, nl, npl=1, scramble=False):
    see, gl, l0, three = _rows(ntask)
    lb = _wavelengths(api, dim, nl, scramble)
    ctx = _context(api, dim, variant, mode)
    try:
        ctx.reconstruct(lb, see, gl, l0, three, H, npsflin=npl)
        d0 = ctx.debug_fetch('dphi0', (ntask, npl * npl, dim // 2 + 1, dim))
        pre = ctx.debug_fetch('pre', (ntask, nl, 40, 40))
    finally:
        ctx.close()
    return _compare(label, variant, mode, dim, lb, d0, pre)


# task counts 1 / 7 / 9 (8 XCD shares; (task, group, sweep) items), wavelength counts 1 / 6 / 7 / 8 / 9 / 13 (groups
# of at most mf_permax = 6 and of at most 8; pairs in the FFT form), one call with the wavelengths scrambled
SHAPES = [(128, 9, 13, False), (256, 7, 8, False), (256, 7, 9, True), (512, 1, 1, False), (512, 7, 6, False),
          (512, 9, 7, False)]


@pytest.mark.parametrize('dim,ntask,nl,scramble', SHAPES)
@pytest.mark.parametrize('variant,mode', VM)
def test_model_rows_one_direction(api, variant, mode, dim, ntask, nl, scramble):
    _run_rows(api, 'rows', variant, mode, dim, ntask, nl, 1, scramble)


@pytest.mark.parametrize('dim,npl,ntask,nl', [(128, 2, 7, 7), (256, 3, 9, 6), (256, 5, 7, 8), (512, 2, 7, 13),
                                              (512, 3, 1, 9)])
@pytest.mark.parametrize('mode', ['A', 'B'])
def test_model_rows_several_directions(api, mode, dim, npl, ntask, nl):
    _run_rows(api, 'rows', 'multi', mode, dim, ntask, nl, npl)


@pytest.mark.parametrize('variant,mode', [('fft', 'A'), ('fft', 'B'), ('f64', 'default')])
def test_model_rows_four_directions_fft_forms(api, variant, mode):
    _run_rows(api, 'rows', variant, mode, 256, 7, 9, 2)
    _run_rows(api, 'rows', variant, mode, 128, 1, 7, 2)


@pytest.mark.parametrize('dim', [1024, 1280])
@pytest.mark.parametrize('mode', ['A', 'B'])
def test_large_grids(api, dim, mode):
    """Above 512^2 the budget of k_mf_prep sums two lines instead of four and the wave layout differs."""
    _run_rows(api, 'rows', 'mfma2', mode, dim, 3, 3)


# ---- arbitrary PSDs through `psf_from_psd` (one task, 256^2) ------------------------------------------------------

DIM = 256
LB_PSD = np.array([480.0, 600.0, 700.0, 800.0, 930.0])


def _psd(name):
    return _psd_cached(name).copy()


@functools.lru_cache(maxsize=None)
def _psd_cached(name):
    if name == 'sharp':
        return R.model_psd(DIM, 0.4, 0.95, 29.0)[0]
    if name == 'broad':
        return R.model_psd(DIM, 1.6, 0.30, 9.0)[0]
    if name == 'ridge':
        return R.ridge_psd(DIM)
    if name == 'model4':
        return R.model_psd(DIM, 0.8, 0.6, 15.0, npl=2)
    raise KeyError(name)


def _run_psd(api, ctx, label, variant, mode, psd, lb, check=True):
    psd = np.asarray(psd)
    if psd.ndim == 2:
        psd = psd[None]
    assert psd.min() >= 0.0
    pre = ctx.psf_from_psd(psd, lb)
    d0 = ctx.debug_fetch('dphi0', (1, psd.shape[0], DIM // 2 + 1, DIM))
    return pre, _compare(label, variant, mode, DIM, lb, d0, pre[None], check)


@pytest.mark.parametrize('ndir', [4, 9, 25])
@pytest.mark.parametrize('mode', ['A', 'B'])
def test_zero_psd_several_directions(api, mode, ndir):
    ctx = _context(api, DIM, 'multi', mode)
    try:
        _run_psd(api, ctx, 'zero', 'multi', mode, np.zeros((ndir, DIM, DIM)), _wavelengths(api, DIM, 7))
    finally:
        ctx.close()


@pytest.mark.parametrize('variant,mode', VM)
def test_zero_psd(api, variant, mode):
    """OTF = telescope OTF: the sharpest stamp possible, nothing pruned by D_phi0, the largest dynamic range the
    fp16 halves see."""
    ctx = _context(api, DIM, variant, mode)
    try:
        _run_psd(api, ctx, 'zero', variant, mode, np.zeros((DIM, DIM)), _wavelengths(api, DIM, 7))
    finally:
        ctx.close()


@pytest.mark.parametrize('variant,mode', VM + [('multi', 'A'), ('multi', 'B')])
def test_tilted_ridge_and_its_transpose(api, variant, mode):
    """A PSD with no symmetry between u and v, and its transpose: each against the reference, and the stamps of the
    transposed PSD equal to the transposed stamps within TOL_A (in both modes) -- a swap of the E and G tables or of the mirror signs
    of P +- Q breaks both."""
    if variant == 'multi':
        r = _psd('ridge')
        psd = np.stack([r, 0.5 * r.T, _psd('sharp'), 1.5 * r])
    else:
        psd = _psd('ridge')[None]
    ctx = _context(api, DIM, variant, mode)
    try:
        a, _ = _run_psd(api, ctx, 'ridge', variant, mode, psd, LB_PSD)
        b, _ = _run_psd(api, ctx, 'ridge transposed', variant, mode, np.ascontiguousarray(np.swapaxes(psd, 1, 2)),
                        LB_PSD)
    finally:
        ctx.close()
    assert R.stamp_errors(a, np.swapaxes(a, 1, 2)).max() > 1e-3                  # (the stamps are not symmetric)
    # (both modes at TOL_A: the blocks the tiers act on are not symmetric under the transposition, yet what the tiers
    # do to these stamps is inside the rounding noise)
    err = R.stamp_errors(b, np.swapaxes(a, 1, 2))
    print('stage_b transposition %s %s %.3e' % (variant, mode, err.max()))
    assert np.all(err <= TOL_A[variant]), (variant, mode, float(err.max()))


LADDER = (-10.0, -17.0, -19.0, -28.0, -30.0, -40.0)


def _ladder(api, variant, mode, extra=(), check=True):
    """The ladder through one context -> 'mf_work' of every rung, [6][5]: tile steps executed, m-tiles, tile steps
    without any pruning, steps with all three products, steps without the low half of the OTF."""
    psd = _psd('model4') if variant == 'multi' else _psd('model4')[:1]
    d0 = np.array([O.structure_function0(p) for p in psd])
    work = []
    ctx = _context(api, DIM, variant, mode, extra)
    try:
        for s, t in zip(R.ladder_scales(d0, 700.0, LADDER, R.telescope_support(DIM)), LADDER):
            _run_psd(api, ctx, 'ladder 2^%d' % t, variant, mode, s * psd, np.array([480.0, 700.0, 930.0]), check)
            work.append(ctx.debug_fetch('mf_work', (5,)))
    finally:
        ctx.close()
    return np.array(work)


@pytest.mark.parametrize('variant,mode', VM_MF + [('multi', 'A'), ('multi', 'B')])
def test_ladder_across_the_tier_thresholds(api, variant, mode):
    """One model PSD times s, s such that the smallest exponent of the OTF on the telescope support at 700 nm steps
    through 2^-10 ... 2^-40: either side of the mid tier at 2^-18 and of the floor at 2^-29.  The work counters show
    that each mode ran what it is named for: (A) every tile step of the half plane with all three products; (B) fewer
    steps the further down the ladder, fewer than the eps rule alone leaves (the same ladder with tier_eps = 0: the
    floor tier dropped blocks), and in k_otf_mfma2 steps without the low half of the OTF (the mid tier)."""
    work = _ladder(api, variant, mode)
    print('stage_b ladder work %s %s' % (variant, mode), work[:, [0, 2, 3, 4]].tolist())
    if mode == 'A':
        assert np.all(work[:, 0] == work[:, 2]) and np.all(work[:, 3] == work[:, 2]) and np.all(work[:, 4] == 0)
        return
    eps_only = _ladder(api, variant, mode, extra=(('tier_eps', 0.0),), check=False)
    print('stage_b ladder work %s eps rule alone' % variant, eps_only[:, [0, 2, 3, 4]].tolist())
    assert np.all(work[:, 0] < work[:, 2]) and work[-1, 0] < work[0, 0]
    assert np.all(eps_only[:, 4] == 0) and np.all(work[:, 0] <= eps_only[:, 0])
    assert work[:, 0].sum() < eps_only[:, 0].sum()
    if variant == 'mfma2':
        assert work[:, 4].sum() > 0


@pytest.mark.parametrize('ndir', [4, 9, 25])
@pytest.mark.parametrize('mode', ['A', 'B'])
def test_sharp_and_broad_directions_in_one_stamp(api, mode, ndir):
    """One sharp and ndir - 1 broad directions, and the reverse: the floor of k_peak_floor sums over all directions
    at the shortest wavelength, the stamp is the direction mean."""
    sharp, broad = _psd('sharp'), _psd('broad')
    ctx = _context(api, DIM, 'multi', mode)
    try:
        for label, one, rest in (('1 sharp', sharp, broad), ('1 broad', broad, sharp)):
            for at in (0, ndir - 1):
                psd = np.stack([one if d == at else rest for d in range(ndir)])
                _run_psd(api, ctx, '%s of %d at %d' % (label, ndir, at), 'multi', mode, psd, LB_PSD)
    finally:
        ctx.close()


def test_the_yardstick_sees_a_lost_low_half(api):
    """Sensitivity: with tier_eps = inf (tiers without a budget) and mf_mid_log2 raised above every block bound, every
    block of k_otf_mfma2 runs without the low fp16 half of the OTF.  By the split-fp16 model that moves the zero-PSD
    stamps by SENS of the peak (tests/test_stage_b_ref.py: at least ten times the largest TOL_A a matrix-core variant
    may get) -- and the comparison with the fp64 reference shows it: above TOL_A, where test_zero_psd holds the
    same call without the two switches below it."""
    lb = _wavelengths(api, DIM, 7)
    ctx = _context(api, DIM, 'mfma2', 'B', extra=(('tier_eps', float('inf')), ('mf_mid_log2', 100.0)))
    try:
        _, err = _run_psd(api, ctx, 'zero, no low half', 'mfma2', 'B', np.zeros((DIM, DIM)), lb, check=False)
    finally:
        ctx.close()
    print('stage_b sensitivity: every block without the low OTF half', err)
    assert err.max() > TOL_A['mfma2'], err
