"""GPU: mpsfr_psd_to_psf on arbitrary PSDs, pupils and sizes, every plane pixel by pixel against the fp64 yardstick
tests/psd_to_psf_ref.py (held on the CPU by tests/test_psd_to_psf_ref.py), as max |diff| / peak of the yardstick's
plane at the bound of tests/test_gpu_psd_to_psf.py.  Every plane is also held to sum 1 and to point symmetry.
Then the batches, a sequence of calls on one context, the refusals and a PSD with a NaN."""
import numpy as np
import pytest

from conftest import record_margin
import psd_to_psf_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-10          # of the yardstick's peak
D = 8.0
LB = 500e-9
_PREC = {128: 'mixed', 256: 'f64', 512: 'mixed', 1024: 'f64', 1280: 'mixed'}     # (the call is fp64 in both)


def _new_context(dim):
    from muse_psfr_amd import Context, grid_pixscale
    return Context(dim=dim, pixscale=grid_pixscale(dim), precision=_PREC[dim])


@pytest.fixture(scope='module')
def ctx_for():
    """One context per grid for the whole module."""
    made = {}

    def get(dim):
        if dim not in made:
            made[dim] = _new_context(dim)
        return made[dim]
    yield get
    for c in made.values():
        c.close()


def _check(cls, got, want):
    """Every plane of `got` against the plane of `want`, and the properties that need no yardstick."""
    got = got.reshape((-1,) + got.shape[-2:])
    want = want.reshape((-1,) + want.shape[-2:])
    assert got.shape == want.shape
    for g, w in zip(got, want):
        err = float(np.abs(g - w).max() / np.abs(w).max())
        record_margin('psd_to_psf_inputs', **{cls: err})
        assert np.isfinite(g).all(), cls
        assert abs(g.sum() - 1) <= 1e-12, (cls, g.sum())
        assert np.abs(g - np.roll(g[::-1, ::-1], 1, axis=(0, 1))).max() <= 1e-14 * np.abs(g).max(), cls
        assert err <= TOL, (cls, err)


def _run(ctx, cls, psd, pup, lbda, phase=None, dimnum=None, d=D):
    got = ctx.psd_to_psf(psd, pup, d, lbda, phase_static=phase, dimnum=dimnum)[0]
    _check(cls, got, R.psd_to_psf_ref(psd, pup, d, np.atleast_1d(lbda), phase, dimnum))
    return got


# ---- sizes: every transform length and every kind of window -------------------------------------------------

SIZES = [(128, 128), (256, 128), (256, 256), (512, 128), (512, 256), (512, 512), (1024, 128), (1024, 512),
         (1024, 1024), (1280, 128), (1280, 1024), (1280, 1280)]


@pytest.mark.parametrize('phased', [False, True], ids=['plain', 'phased'])
@pytest.mark.parametrize('dim,dimnum', SIZES)
def test_sizes(ctx_for, dim, dimnum, phased):
    npup = dimnum // 2 - 3                           # odd
    pup = R.rand_pupil(npup)
    psd = R.scaled_psd(R.asym_psd(dim), pup, D, LB, dimnum, 10.0)
    phase = R.rand_phase(npup, 1.0, LB) if phased else None
    _run(ctx_for(dim), 'size_%d_%d' % (dim, dimnum), psd, pup, np.array([LB, 850e-9]), phase, dimnum)


# ---- pupil sizes ----------------------------------------------------------------------------------------------

def _npup_cases(m):
    """Either side of a multiple of the lines per workgroup and of the threads per line of Plan<m>, an odd size
    near half, one below the transform length and the length itself (nothing padded: the autocorrelation wraps)."""
    tpr, sl = R.PLAN[m]['TPR'], R.PLAN[m]['SLOTS']
    near_half = 333 if m == 1280 else m // 2 - 1
    return [('3xSLOTS-1', 3 * sl - 1), ('3xSLOTS+1', 3 * sl + 1), ('TPR-1', tpr - 1), ('TPR', tpr), ('TPR+1', tpr + 1),
            ('3xTPR-1', 3 * tpr - 1), ('3xTPR+1', 3 * tpr + 1), ('odd_near_half', near_half), ('dimnum-1', m - 1),
            ('dimnum', m)]


NPUPS = ([(128, 'npup_%d' % p, p) for p in (1, 2, 3, 7, 63, 64, 65, 127, 128)]
         + [(m, name, p) for m in (512, 1280) for name, p in _npup_cases(m)])


@pytest.mark.parametrize('m,name,npup', NPUPS, ids=['%d_%s_%d' % c for c in NPUPS])
def test_pupil_sizes(ctx_for, m, name, npup):
    pup = R.rand_pupil(npup)
    psd = R.scaled_psd(R.asym_psd(m), pup, D, LB, m, 10.0)
    got = _run(ctx_for(m), 'npup_%d' % m, psd, pup, LB, R.rand_phase(npup, 1.0, LB))
    if npup == 1:                                    # one sample: the OTF is its DC term, the PSF is flat
        np.testing.assert_allclose(got, 1.0 / m ** 2, rtol=1e-15, atol=0)


# ---- shapes of the inputs (256 -> 128: the window is cut from a larger grid, the pupil is odd) ----------------

def _shape_cases():
    n, m, p = 256, 128, 61
    pup = R.rand_pupil(p)                            # in [-0.2, 1]
    asym = R.scaled_psd(R.asym_psd(n), pup, D, LB, m, 10.0)
    ridge = R.scaled_psd(R.ridge_psd(n), pup, D, LB, m, 10.0)
    lpup, lphase = R.l_pupil_with_huge_phase(p, LB)
    neg = R.rand_pupil(p, lo=-1.0, hi=0.2)
    assert neg.sum() < 0
    assert (np.roll(asym[::-1, ::-1], 1, axis=(0, 1)) != asym).mean() > 0.99             # psd[i][j] != psd[-i][-j]
    signed = R.scaled_psd(R.signed_psd(n), pup, D, LB, m, 20.0)
    assert (signed < 0).mean() > 0.2 and R.max_exponent(signed, pup, D, LB, m) < 700
    return {
        'psd_no_symmetry': (asym, pup, None),
        'psd_ridge': (ridge, pup, None),
        'psd_ridge_transposed': (np.ascontiguousarray(ridge.T), pup, None),
        'psd_negative_values': (signed, pup, None),
        'psd_zero': (np.zeros((n, n)), lpup, None),                 # the pupil's diffraction pattern
        'pupil_random': (asym, pup, R.rand_phase(p, 1.0, LB)),
        'pupil_l_shaped': (asym, lpup, None),
        'pupil_negative_sum': (asym, neg, None),
        'pupil_times_1e-30': (asym, pup * 1e-30, None),
        'pupil_times_1e30': (asym, pup * 1e30, None),
        'phase_huge_where_pupil_is_zero': (asym, lpup, lphase),
        'phase_1e-3_rad': (asym, pup, R.rand_phase(p, 1e-3, LB)),
        'phase_1_rad': (asym, pup, R.rand_phase(p, 1.0, LB)),
        'phase_30_rad': (asym, pup, R.rand_phase(p, 30.0, LB)),
    }


SHAPES = ['psd_no_symmetry', 'psd_ridge', 'psd_ridge_transposed', 'psd_negative_values', 'psd_zero', 'pupil_random',
          'pupil_l_shaped', 'pupil_negative_sum', 'pupil_times_1e-30', 'pupil_times_1e30',
          'phase_huge_where_pupil_is_zero', 'phase_1e-3_rad', 'phase_1_rad', 'phase_30_rad']


@pytest.fixture(scope='module')
def shape_cases():
    cases = _shape_cases()
    assert sorted(cases) == sorted(SHAPES)
    return cases


@pytest.mark.parametrize('name', SHAPES)
def test_input_shapes(ctx_for, shape_cases, name):
    psd, pup, phase = shape_cases[name]
    _run(ctx_for(256), name, psd, pup, np.array([LB, 850e-9]), phase, 128)


# ---- ranges -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dim,dimnum', [(256, 128), (1280, 1280)])
@pytest.mark.parametrize('exponent', [1e-6, 1.0, 50.0, 700.0, 800.0, 1e5])
def test_psd_scale_ladder(ctx_for, dim, dimnum, exponent):
    """max over the window of (1/2) (2 pi / lambda_nm)^2 Dphi0 from 1e-6 (the diffraction pattern) across the
    underflow of exp (above 745) to a PSF that is flat but for rounding."""
    npup = dimnum // 2 - 3
    pup = R.rand_pupil(npup)
    psd = R.scaled_psd(R.asym_psd(dim), pup, D, LB, dimnum, exponent)
    _run(ctx_for(dim), 'scale_%g_at_%d' % (exponent, dimnum), psd, pup, LB, None, dimnum)


@pytest.mark.parametrize('d', [1.0, 39.0])
def test_wavelengths_and_diameters(ctx_for, d):
    pup = R.rand_pupil(61)
    psd = R.scaled_psd(R.asym_psd(256), pup, D, LB, 128, 10.0)      # scaled for D = 8 and 500 nm
    _run(ctx_for(256), 'lambda_300nm_5um_D_%g' % d, psd, pup, np.array([300e-9, 5e-6]), R.rand_phase(61, 1.0, LB),
         128, d=d)


# ---- batches against the yardstick --------------------------------------------------------------------------

@pytest.mark.parametrize('nl', [9, 17])
def test_batches(ctx_for, nl):
    """Three PSDs, more wavelengths than a chunk of 8 holds and one left over: the last chunk has one plane and its
    OTFs (static phase: one per wavelength) are rebuilt at an offset.  Into host memory and through a device pointer."""
    import torch
    ctx = ctx_for(256)
    pup = R.rand_pupil(61)
    phase = R.rand_phase(61, 1.0, LB)
    psd = np.stack([R.scaled_psd(p, pup, D, LB, 128, t) for p, t in
                    ((R.asym_psd(256), 10.0), (R.ridge_psd(256), 3.0), (R.asym_psd(256, seed=7), 40.0))])
    lb = np.linspace(460e-9, 940e-9, nl)
    want = np.stack([R.psd_to_psf_ref(p, pup, D, lb, phase, 128) for p in psd])
    host = ctx.psd_to_psf(psd, pup, D, lb, phase_static=phase, dimnum=128)
    assert host.shape == (3, nl, 128, 128)
    _check('batch_host', host, want)
    dev = torch.full(host.shape, np.nan, dtype=torch.float64, device='cuda:0')
    assert ctx.psd_to_psf(psd, pup, D, lb, phase_static=phase, dimnum=128, out=dev.data_ptr()) is None
    _check('batch_device', dev.cpu().numpy(), want)


# ---- a sequence of calls on one context ---------------------------------------------------------------------

# (dimnum, npup, phased, nl): dimnum 512 -> 128 -> 512 -> 256 (the twiddle table of the last length), npup
# 100 -> 31 -> 256 (grow-only workspaces), phased and unphased alternating (the OTF stride), nl 17 -> 1 -> 17
SEQUENCE = [(512, 100, True, 17), (128, 31, False, 1), (512, 256, True, 1), (256, 100, False, 17), (512, 31, True, 1)]


def _sequence_call(ctx, step):
    dimnum, npup, phased, nl = SEQUENCE[step]
    pup = R.rand_pupil(npup, seed=10 + step)
    psd = R.scaled_psd(R.asym_psd(512), pup, D, LB, dimnum, 10.0)
    lb = np.linspace(460e-9, 940e-9, nl)
    return ctx.psd_to_psf(psd, pup, D, lb, phase_static=R.rand_phase(npup, 1.0, LB) if phased else None, dimnum=dimnum)


def test_call_sequence_equals_fresh_contexts():
    """Each call of the sequence equals, bit for bit, the same call made first on a fresh context."""
    ctx = _new_context(512)
    try:
        seq = [_sequence_call(ctx, i) for i in range(len(SEQUENCE))]
    finally:
        ctx.close()
    for i in range(len(SEQUENCE)):
        fresh = _new_context(512)
        try:
            np.testing.assert_array_equal(_sequence_call(fresh, i), seq[i], err_msg='step %d' % i)
        finally:
            fresh.close()


# ---- refusals and a PSD with a NaN --------------------------------------------------------------------------

def test_refusals_leave_no_trace(ctx_for):
    from muse_psfr_amd._lib import MpsfrError
    ctx = ctx_for(256)
    pup = R.rand_pupil(61)
    phase = R.rand_phase(61, 1.0, LB)
    psd = R.scaled_psd(R.asym_psd(256), pup, D, LB, 128, 10.0)
    lb = np.array([LB, 850e-9])

    def valid():
        return ctx.psd_to_psf(psd, pup, D, lb, phase_static=phase, dimnum=128)
    before = valid()
    zero_sum = np.random.default_rng(6).integers(-2, 3, (61, 61)).astype(float)      # whole numbers: any order of
    zero_sum[0, 0] -= zero_sum.sum()                                                 # summation gives exactly 0
    assert zero_sum.sum() == 0.0 and np.abs(zero_sum).sum() > 1000
    inf = pup.copy()
    inf[5, 7] = np.inf
    refused = [
        (r'dimnum=192 not supported', dict(dimnum=192)),
        (r'dimnum=512 larger than the grid \(dim=256\)', dict(dimnum=512)),
        (r'npup=129 must be in \[1, dimnum=128\]', dict(pup=R.rand_pupil(129), phase_static=None)),
        (r'D must be > 0', dict(D=0.0)),
        (r'D must be > 0', dict(D=np.nan)),
        (r'lbda_m\[1\] must be > 0', dict(lbda_m=np.array([LB, 0.0]))),
        (r'lbda_m\[0\] must be > 0', dict(lbda_m=np.array([np.nan, LB]))),
        (r'sum\(pup\) must be finite and non-zero', dict(pup=zero_sum)),
        (r'sum\(pup\) must be finite and non-zero', dict(pup=inf)),
    ]
    for msg, change in refused:
        kw = dict(psd=psd, pup=pup, D=D, lbda_m=lb, phase_static=phase, dimnum=128)
        kw.update(change)
        with pytest.raises(MpsfrError, match=msg):
            ctx.psd_to_psf(**kw)
        np.testing.assert_array_equal(valid(), before, err_msg=msg)


def test_psd_with_a_nan(ctx_for):
    """include/mpsfr.h: a PSD with a NaN is not refused; its planes are NaN in every pixel, the other PSDs of the
    call are computed as ever, and the next call on the context equals a fresh one."""
    ctx = ctx_for(256)
    pup = R.rand_pupil(61)
    phase = R.rand_phase(61, 1.0, LB)
    good = R.scaled_psd(R.asym_psd(256), pup, D, LB, 128, 10.0)
    bad = good.copy()
    bad[200, 13] = np.nan
    lb = np.array([LB, 850e-9])
    fresh = _new_context(256)
    try:
        want = fresh.psd_to_psf(good, pup, D, lb, phase_static=phase, dimnum=128)
    finally:
        fresh.close()
    got = ctx.psd_to_psf(np.stack([good, bad, good]), pup, D, lb, phase_static=phase, dimnum=128)
    assert np.isnan(got[1]).all()
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[2], want[0])
    np.testing.assert_array_equal(ctx.psd_to_psf(good, pup, D, lb, phase_static=phase, dimnum=128), want)
