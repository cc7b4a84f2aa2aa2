"""GPU: the PSF-model fit of observed stars (mpsfr_fit_stamps_psf), both precisions.

1. parity with the fp64 SciPy yardstick (psf_fit_ref) on the shared noisy, masked stars, all four variants
   (background x fixed shift), every star: each fitted variable within SIGMA_TOL of the yardstick's minimum in units
   of its formal error (f64 1e-5: ten times the floor tests/test_psf_fit_host.py asserts for the yardstick; mixed 2e-6:
   see SIGMA_TOL below), the error columns and chi2 within 1e-3 relative, n_used equal.
2. exact cases: d = F roll(P, (k, l)) + b on Moffat stamps whose wings are below 1e-12 of the peak at the rolled edge,
   (k, l) = (0, 0) and (2, -3): the minimum sits on a knot of the interpolant.
3. invariances, bit for bit: var x 4; data x 2^k with var x 4^k; the stored values of unused pixels; batch = single
   stars; device = host pointers; psf_index sharing one stamp = copies of it.  To tolerance: transposition.
4. fixed shift: the closed-form weighted least squares; a free fit started at the yardstick's minimum stays there.
5. degenerate rows and refusals.
6. a device-output reconstruct_field chained into the device form; fit_stars_with_psf.
Margins go to record_margin('fit_psf', ...).
"""
import ctypes as C

import numpy as np
import pytest

import psf_fit_ref as R
from conftest import H, record_margin

pytestmark = pytest.mark.gpu

TOL = {'f64': 1e-8, 'mixed': 1e-4}            # tests/test_gpu_fit_ell.py
# mixed: the worst value of the first GPU run was 4.3e-7 (profiles/psf_fit_margins.json, sigma_mixed_fixed; the float
# gradient of the fp64 polish); three times that, rounded up to one digit -- far inside 1e-2, the mixed tolerance of the
# observed fit, which it may never exceed
SIGMA_TOL = {'f64': 1e-5, 'mixed': 2e-6}
ERR_TOL = 1e-3
PRECS = ['mixed', 'f64']
NF = 16


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


def _status(fit):
    return fit[:, 10].astype(int)


def _sigma(row, want):
    """Worst |difference| of the fitted variables in units of the yardstick's formal error, and the worst relative
    difference of the error columns."""
    val, err = R.gpu_values(row)
    free = want['free']
    return (float(np.max(np.abs(val - want['x'])[free] / want['err'][free])),
            float(np.max(np.abs(err - want['err'])[free] / want['err'][free])))


# ---- 1. parity against the yardstick
@pytest.mark.parametrize('back,fixed', R.VARIANTS)
@pytest.mark.parametrize('prec', PRECS)
def test_parity_with_scipy_on_noisy_masked_stars(ctx, prec, back, fixed):
    data, var, psf, truth, shift, ref = R.yardstick(back, fixed)
    assert len(data) == 24
    fit = ctx.fit_stamps_psf(data, psf, var=var, shift=shift, background=back, fixed_shift=fixed)
    assert fit.shape == (24, NF)
    assert np.all(_status(fit) == 0), _status(fit)
    assert np.all(np.isfinite(fit))
    worst, worst_err, worst_chi2 = 0.0, 0.0, 0.0
    for row, want in zip(fit, ref):
        assert int(row[11]) == want['npix']
        s, e = _sigma(row, want)
        worst, worst_err = max(worst, s), max(worst_err, e)
        worst_chi2 = max(worst_chi2, abs(row[4] - want['chi2']) / want['chi2'])
    tag = '%s%s%s' % (prec, '_back' if back else '', '_fixed' if fixed else '')
    print('fit_psf parity %s: worst |d| / sigma %.2e; error columns %.2e, chi2 %.2e relative; iterations %d - %d' % (
        tag, worst, worst_err, worst_chi2, fit[:, 5].min(), fit[:, 5].max()))
    record_margin('fit_psf', **{'sigma_' + tag: worst, 'err_' + tag: worst_err, 'chi2_' + tag: worst_chi2})
    assert worst <= SIGMA_TOL[prec]
    assert worst_err <= ERR_TOL and worst_chi2 <= ERR_TOL
    # fields of variables that are not fitted are 0, a fixed shift is echoed, flux = F sum(P)
    assert np.all(fit[:, 14:16] == 0)
    if not back:
        assert np.all(fit[:, 3] == 0) and np.all(fit[:, 9] == 0)
    if fixed:
        assert np.array_equal(fit[:, 1:3], shift) and np.all(fit[:, 7:9] == 0) and np.all(fit[:, 5] == 1)
    sums = psf.sum(axis=(1, 2))
    assert np.max(np.abs(fit[:, 12] - fit[:, 0] * sums) / np.abs(fit[:, 12])) <= 1e-13
    assert np.max(np.abs(fit[:, 13] - fit[:, 6] * np.abs(sums)) / fit[:, 13]) <= 1e-13


# ---- 2. exact cases
def _compact_moffats():
    """Moffat stamps (sum 1) with wings below 1e-12 of the peak 16 pixels from the centre."""
    st = np.array([R.moffat(20.0, 20.0, fw, n) for fw, n in ((2.5, 30.0), (3.0, 30.0), (4.0, 40.0))])
    st /= st.sum(axis=(1, 2))[:, None, None]
    for s in st:
        assert max(s[:4].max(), s[-4:].max(), s[:, :4].max(), s[:, -4:].max()) < 1e-12 * s.max()
    return st


@pytest.mark.parametrize('kl', [(0, 0), (2, -3)])
@pytest.mark.parametrize('prec', PRECS)
def test_rolled_stamps_come_back_exactly(ctx, prec, kl):
    psf = _compact_moffats()
    F = np.array([3.0, 700.0, 0.02])
    peak = F * psf.max(axis=(1, 2))
    b = np.array([0.01, -0.005, 0.03]) * peak
    stars = F[:, None, None] * np.roll(psf, kl, axis=(1, 2)) + b[:, None, None]
    fit = ctx.fit_stamps_psf(stars, psf, background=True)
    assert np.all(_status(fit) == 0), _status(fit)
    assert np.all(np.isfinite(fit)) and np.all(fit[:, 11] == 1600)
    w = dict(F=np.max(np.abs(fit[:, 0] - F) / F), back=np.max(np.abs(fit[:, 3] - b) / peak),
             dp=np.max(np.abs(fit[:, 1] - kl[0])), dq=np.max(np.abs(fit[:, 2] - kl[1])))
    record_margin('fit_psf', **{'exact_%s_%d_%d_%s' % (prec, kl[0], kl[1], k): v / TOL[prec] for k, v in w.items()})
    assert max(w.values()) <= TOL[prec], w
    # without a background term on stars without one
    f0 = ctx.fit_stamps_psf(stars - b[:, None, None], psf, background=False)
    assert np.all(_status(f0) == 0)
    assert np.max(np.abs(f0[:, 0] - F) / F) <= TOL[prec] and np.max(np.abs(f0[:, 1:3] - np.array(kl))) <= TOL[prec]


# ---- 3. invariances
def _call(ctx, back, fixed, data, var, psf, shift, **kw):
    return ctx.fit_stamps_psf(data, psf, var=var, shift=shift, background=back, fixed_shift=fixed, **kw)


@pytest.mark.parametrize('back,fixed', R.VARIANTS)
@pytest.mark.parametrize('prec', PRECS)
def test_scales_of_var_and_data_bit_for_bit(ctx, prec, back, fixed):
    data, var, psf, truth, shift, _ = R.yardstick(back, fixed)
    data, var, psf = data[:8], var[:8], psf[:8]
    shift = None if shift is None else shift[:8]
    base = _call(ctx, back, fixed, data, var, psf, shift)
    assert np.all(_status(base) == 0)
    f4 = _call(ctx, back, fixed, data, 4.0 * var, psf, shift)
    other = [k for k in range(NF) if k != 4]
    assert np.array_equal(f4[:, other], base[:, other])
    assert np.array_equal(f4[:, 4] * 4.0, base[:, 4])
    amp = [0, 3, 6, 9, 12, 13]                      # F, back, err_F, err_back, flux, err_flux
    rest = [k for k in range(NF) if k not in amp]
    for k in (20, -20):
        fk = _call(ctx, back, fixed, data * 2.0 ** k, var * 4.0 ** k, psf, shift)
        assert np.array_equal(fk[:, amp], base[:, amp] * 2.0 ** k), k
        assert np.array_equal(fk[:, rest], base[:, rest]), k
    # a factor on the model stamp: F and err_F take its inverse, nothing else moves (a power of two: exactly)
    fp = _call(ctx, back, fixed, data, var, psf * 2.0 ** 7, shift)
    assert np.array_equal(fp[:, [0, 6]] * 2.0 ** 7, base[:, [0, 6]])
    keep = [k for k in range(NF) if k not in (0, 6)]
    assert np.array_equal(fp[:, keep], base[:, keep])


@pytest.mark.parametrize('prec', PRECS)
def test_unused_values_batches_device_pointers_and_psf_index_bit_for_bit(ctx, prec):
    import torch
    data, var, psf, truth, _, _ = R.yardstick(True, False)
    data, var, psf = data[:6], var[:6], psf[:6]
    base = ctx.fit_stamps_psf(data, psf, var=var)
    assert np.all(_status(base) == 0)
    # the stored value of an unused pixel
    bad_var = ~(var > 0)
    d2, v2 = data.copy(), var.copy()
    d2[bad_var] = 1e30
    d2[np.isnan(data)] = np.nan
    v2[np.isnan(data)] = 7.0
    assert np.array_equal(ctx.fit_stamps_psf(d2, psf, var=v2), base)
    d3, v3 = data.copy(), var.copy()
    d3[bad_var] = np.inf                            # an infinite value under an invalid variance is unused too
    v3[bad_var] = np.nan
    v3[np.isnan(data)] = -np.inf
    assert np.array_equal(ctx.fit_stamps_psf(d3, psf, var=v3), base)
    # the batch is the single stars
    for k in range(len(data)):
        assert np.array_equal(ctx.fit_stamps_psf(data[k], psf[k], var=var[k]), base[k:k + 1]), k
    # psf_index: every star with the model stamp of star 0 (a poor model for most: whatever the rows hold, they are the
    # same), shared against copies, and a permutation
    shared = ctx.fit_stamps_psf(data, psf[:1], var=var, psf_index=np.zeros(len(data), dtype=int))
    copies = ctx.fit_stamps_psf(data, np.repeat(psf[:1], len(data), axis=0), var=var)
    assert np.array_equal(shared, copies)
    perm = np.array([3, 5, 0, 1, 4, 2])
    assert np.array_equal(ctx.fit_stamps_psf(data, psf[np.argsort(perm)], var=var, psf_index=perm), base)
    # device pointers, every variant
    dev = torch.device('cuda:0')
    ts = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    tv = torch.from_numpy(np.ascontiguousarray(var)).to(dev)
    tp = torch.from_numpy(np.ascontiguousarray(psf)).to(dev)
    sh = np.round(truth[:6, 1:3] * 8) / 8
    tsh = torch.from_numpy(np.ascontiguousarray(sh)).to(dev)
    tix = torch.from_numpy(perm.astype(np.int32)).to(dev)
    tpp = torch.from_numpy(np.ascontiguousarray(psf[np.argsort(perm)])).to(dev)
    tf = torch.full((len(data), NF), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_stamps_psf_device(len(data), ts.data_ptr(), len(data), tpp.data_ptr(), tf.data_ptr(), var_ptr=tv.data_ptr(),
                              psf_index_ptr=tix.data_ptr())
    ctx.sync()
    assert np.array_equal(tf.cpu().numpy(), base)
    for back, fixed in R.VARIANTS:
        want = ctx.fit_stamps_psf(data, psf, var=None, shift=sh, background=back, fixed_shift=fixed)
        tf.fill_(-1.0)
        torch.cuda.synchronize()
        ctx.fit_stamps_psf_device(len(data), ts.data_ptr(), len(data), tp.data_ptr(), tf.data_ptr(),
                                  shift_ptr=tsh.data_ptr(), background=back, fixed_shift=fixed)
        ctx.sync()
        assert np.array_equal(tf.cpu().numpy(), want), (back, fixed)


@pytest.mark.parametrize('prec', PRECS)
def test_transposing_both_stamps_swaps_the_shift(ctx, prec):
    data, var, psf, truth, _, ref = R.yardstick(True, False)
    f0 = ctx.fit_stamps_psf(data, psf, var=var)
    ft = ctx.fit_stamps_psf(np.transpose(data, (0, 2, 1)).copy(), np.transpose(psf, (0, 2, 1)).copy(),
                            var=np.transpose(var, (0, 2, 1)).copy())
    assert np.all(_status(f0) == 0) and np.all(_status(ft) == 0)
    assert np.array_equal(ft[:, 11], f0[:, 11])
    # both lie within SIGMA_TOL of the minimum, in units of the formal error
    swap = [0, 2, 1, 3]
    worst = 0.0
    for a, t, want in zip(f0, ft, ref):
        worst = max(worst, float(np.max(np.abs(t[:4][swap] - a[:4]) / want['err'])))
        assert abs(t[4] - a[4]) <= ERR_TOL * a[4]
    record_margin('fit_psf', **{'transpose_sigma_%s' % prec: worst})
    assert worst <= 2 * SIGMA_TOL[prec]


# ---- 4. fixed shift
@pytest.mark.parametrize('back', [False, True])
@pytest.mark.parametrize('prec', PRECS)
def test_fixed_shift_is_closed_form_and_a_start_at_the_minimum_stays(ctx, prec, back):
    data, var, psf, truth, shift, ref = R.yardstick(back, True)
    fit = ctx.fit_stamps_psf(data, psf, var=var, shift=shift, background=back, fixed_shift=True)
    assert np.all(_status(fit) == 0) and np.all(fit[:, 5] == 1)
    worst = 0.0
    for k, row in enumerate(fit):
        F, b = R.linear_solve(data[k], var[k], psf[k], shift[k, 0], shift[k, 1], back)
        worst = max(worst, abs(row[0] - F) / abs(F), abs(row[3] - b) / abs(b) if back else abs(row[3]))
    print('fixed shift %s back=%d: worst relative difference to the closed form %.2e' % (prec, back, worst))
    record_margin('fit_psf', **{'closed_form_%s_%d' % (prec, back): worst})
    if prec == 'f64':
        assert worst <= 1e-12
    # a free fit started from the yardstick's minimum stays there
    _, _, _, _, _, free = R.yardstick(back, False)
    start = np.array([f['x'][1:3] for f in free])
    f2 = ctx.fit_stamps_psf(data, psf, var=var, shift=start, background=back)
    assert np.all(_status(f2) == 0)
    stay = max(_sigma(row, want)[0] for row, want in zip(f2, free))
    record_margin('fit_psf', **{'stay_sigma_%s_%d' % (prec, back): stay})
    assert stay <= SIGMA_TOL[prec]


# ---- 5. degenerate rows and refusals
@pytest.mark.parametrize('back,fixed', R.VARIANTS)
@pytest.mark.parametrize('prec', PRECS)
def test_degenerate_rows(ctx, prec, back, fixed):
    npar = 1 + (0 if fixed else 2) + back
    P = R.moffat(20.0, 20.0, 4.0, 2.5)
    P /= P.sum()
    good = 100.0 * R.resample(P, 0.4, -1.3) + (0.02 if back else 0.0)
    n = 7
    st, psf, var = np.array([good] * n), np.array([P] * n), np.ones((n, 40, 40))
    sh = np.tile([0.5, -1.25], (n, 1))
    psf[1] = 0.0                                       # an all-zero model stamp
    psf[2, 3, 4] = np.nan                              # a NaN in the model
    keep = np.zeros(1600, dtype=bool)
    keep[[20 * 40 + 17 + k for k in range(npar)]] = True
    st[3] = np.where(keep.reshape(40, 40), good, np.nan)       # n_used = npar
    st[4, 7, 9] = np.inf                               # an infinite pixel under a valid variance
    psf[5, 0, 0] = -np.inf                             # an infinite model pixel
    kw = dict(var=var, shift=sh, background=back, fixed_shift=fixed)
    fit = ctx.fit_stamps_psf(st, psf, **kw)
    assert not np.any(np.isnan(fit))
    assert list(_status(fit)) == [0, 2, 2, 2, 2, 2, 0], _status(fit)
    assert list(fit[:, 11].astype(int)) == [1600, 1600, 1600, npar, 1599, 1600, 1600]
    other = [k for k in range(NF) if k not in (10, 11)]
    assert np.all(fit[1:6][:, other] == 0)
    # the good rows are what they are alone, and right
    alone = ctx.fit_stamps_psf(good, P, var=np.ones((40, 40)), shift=sh[:1], background=back, fixed_shift=fixed)
    assert np.array_equal(fit[0:1], alone) and np.array_equal(fit[6:7], alone)
    if not fixed:
        assert abs(alone[0, 0] - 100.0) <= TOL[prec] * 100.0
        assert abs(alone[0, 1] - 0.4) <= TOL[prec] and abs(alone[0, 2] + 1.3) <= TOL[prec]
    # one used pixel more than parameters is fitted or refused, never NaN in a row that claims a minimum
    keep[20 * 40 + 17 + npar] = True
    f3 = ctx.fit_stamps_psf(np.where(keep.reshape(40, 40), good, np.nan), P, var=None, shift=sh[:1], background=back,
                            fixed_shift=fixed)
    assert int(f3[0, 11]) == npar + 1
    assert int(f3[0, 10]) != 0 or np.all(np.isfinite(f3))
    # the amplitude rule, for the star and for the model stamp
    f4 = ctx.fit_stamps_psf(np.array([good * 2.0 ** 41, good * 2.0 ** -48, good * 2.0 ** 30, good, good, good]),
                            np.array([P, P, P, P * 2.0 ** 50, P * 2.0 ** -40, P * 2.0 ** 30]), shift=np.tile(sh[0], (6, 1)),
                            background=back, fixed_shift=fixed)
    assert list(_status(f4)) == [2, 2, 0, 2, 2, 0]
    assert abs(f4[2, 0] / 2.0 ** 30 - alone[0, 0]) <= TOL[prec] * alone[0, 0]
    assert abs(f4[5, 0] * 2.0 ** 30 - alone[0, 0]) <= TOL[prec] * alone[0, 0]


@pytest.mark.parametrize('prec', PRECS)
def test_a_star_12_px_from_its_model_ends_against_the_bound(ctx, prec):
    P = R.moffat(20.0, 20.0, 4.0, 2.5)
    P /= P.sum()
    stars = np.array([50.0 * R.moffat(32.0, 20.0, 4.0, 2.5) + 0.1, 50.0 * R.moffat(20.0, 8.0, 4.0, 2.5) + 0.1])
    for back in (False, True):
        fit = ctx.fit_stamps_psf(stars, np.array([P, P]), background=back)
        assert list(_status(fit)) == [1, 1], (back, fit)
        assert np.all(np.isfinite(fit))
        assert fit[0, 1] == 8.0 and fit[1, 2] == -8.0


def test_bad_arguments_are_refused_and_leave_the_output(api):
    import torch
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    P = R.moffat(20.0, 20.0, 4.0, 2.5)
    st = np.ascontiguousarray(np.array([3.0 * P, 2.0 * P]))
    ps = np.ascontiguousarray(np.array([P, P]))
    out = np.full((2, NF), -7.0)
    ix = np.array([0, 1], dtype=np.int32)
    sh = np.zeros((2, 2))
    vp = C.c_void_p

    def ptr(a):
        return None if a is None else vp(a.ctypes.data)

    def call(nstamp=2, stamps=st, var=None, npsf=2, psf=ps, index=None, shift=None, flags=1, fit=out):
        return ctx.lib.mpsfr_fit_stamps_psf(ctx._h, nstamp, ptr(stamps), ptr(var), npsf, ptr(psf), ptr(index),
                                            ptr(shift), flags, ptr(fit), 0)

    bad = (dict(nstamp=0), dict(nstamp=-1), dict(npsf=0), dict(stamps=None), dict(psf=None), dict(fit=None),
           dict(flags=8), dict(flags=-1), dict(flags=2), dict(flags=3), dict(flags=7),      # unknown bits, elliptical
           dict(npsf=1),                                                                   # no index, npsf != nstamp
           dict(index=np.array([0, 2], dtype=np.int32)), dict(index=np.array([-1, 0], dtype=np.int32)),
           dict(shift=np.array([[0.0, np.nan], [0.0, 0.0]])), dict(shift=np.array([[0.0, 0.0], [np.inf, 0.0]])),
           dict(shift=np.array([[8.5, 0.0], [0.0, 0.0]])), dict(shift=np.array([[0.0, 0.0], [0.0, -8.01]])),
           dict(flags=4), dict(flags=5))                                                   # fixed shift without shift
    for kw in bad:
        assert call(**kw) == -1, kw                    # MPSFR_E_INVALID
        assert np.all(out == -7.0), kw
    for kw in (dict(), dict(index=ix, shift=sh), dict(npsf=1, index=np.zeros(2, dtype=np.int32)),
               dict(flags=5, shift=sh), dict(flags=4, shift=sh), dict(flags=0)):
        out[:] = -7.0
        assert call(**kw) == 0, kw
        assert np.all(out[:, 10] == 0) and np.all(out[:, 11] == 1600), kw
        assert np.max(np.abs(out[:, 0] - [3.0, 2.0])) <= 1e-4 and np.max(np.abs(out[:, 1:3])) <= 1e-4
    with pytest.raises(ValueError):
        ctx.fit_stamps_psf(st, ps, background=1)
    with pytest.raises(ValueError):
        ctx.fit_stamps_psf(st, ps[:1])
    with pytest.raises(ValueError):
        ctx.fit_stamps_psf(st, ps, fixed_shift=True)
    with pytest.raises(ValueError):
        ctx.fit_stamps_psf_device(0, 1, 1, 1, 1)
    with pytest.raises(ValueError):
        ctx.fit_stamps_psf_device(2, 1, 1, 1, 1)       # no index, npsf != nstamp
    with pytest.raises(ValueError):
        ctx.fit_stamps_psf_device(2, 1, 2, 0, 1)
    # the device form: an index out of range or a shift outside the domain is that row's status 2, nothing else
    dev = torch.device('cuda:0')
    ts, tp = torch.from_numpy(np.concatenate([st, st])).to(dev), torch.from_numpy(ps).to(dev)
    tix = torch.tensor([0, 2, -1, 1], dtype=torch.int32, device=dev)
    tsh = torch.tensor([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64, device=dev)
    tf = torch.full((4, NF), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_stamps_psf_device(4, ts.data_ptr(), 2, tp.data_ptr(), tf.data_ptr(), psf_index_ptr=tix.data_ptr(),
                              shift_ptr=tsh.data_ptr())
    ctx.sync()
    assert list(tf.cpu().numpy()[:, 10].astype(int)) == [0, 2, 2, 0]
    tix = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=dev)
    tsh = torch.tensor([[0.0, 0.0], [float('nan'), 0.0], [0.0, 9.0], [0.0, -8.0]], dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_stamps_psf_device(4, ts.data_ptr(), 2, tp.data_ptr(), tf.data_ptr(), psf_index_ptr=tix.data_ptr(),
                              shift_ptr=tsh.data_ptr())
    ctx.sync()
    got = tf.cpu().numpy()
    assert list(got[:, 10].astype(int))[:3] == [0, 2, 2] and not np.any(np.isnan(got))
    ctx.close()


def test_timed_under_the_profiling_id_of_the_fit(api):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    data, var, psf, _ = R.noisy_stars(True)
    ctx.set_option('profile', 1)
    ctx.profile_reset()
    ctx.fit_stamps_psf(data[:4], psf[:4], var=var[:4])
    prof = ctx.profile()
    assert prof['fit'][1] == 1 and prof['fit'][0] > 0
    assert all(v[1] == 0 for k, v in prof.items() if k != 'fit'), prof
    ctx.close()


# ---- 6. chaining and plumbing
@pytest.mark.parametrize('prec', PRECS)
def test_reconstruct_field_device_chained_into_the_fit(api, prec):
    import torch
    dim = 128
    ps = api.grid_pixscale(dim)
    lb = np.array([600.0, 850.0])
    see, gl, l0, three = np.array([1.0, 0.8]), np.array([0.7, 0.5]), np.array([25.0, 20.0]), np.array([0, 1])
    pos = np.array([[0.0, 0.0], [-20.0, 40.0]])
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    ref = ctx.reconstruct_field(lb, see, gl, l0, three, H, pos)
    models = ref['psf'].reshape(-1, 40, 40)
    nst = len(models)
    assert nst == 8
    rng = np.random.default_rng(8)
    truth = np.column_stack([rng.uniform(100, 1000, nst), rng.uniform(-3, 3, nst), rng.uniform(-3, 3, nst),
                             rng.uniform(-0.01, 0.03, nst)])
    stars = np.array([R.model(m, t) for m, t in zip(models, truth)])
    dev = torch.device('cuda:0')
    tp = torch.empty(ref['psf'].shape, dtype=torch.float64, device=dev)
    tsum = torch.empty(ref['psf_sum'].shape, dtype=torch.float64, device=dev)
    tfit = torch.empty(ref['fit'].shape, dtype=torch.float64, device=dev)
    tstar = torch.from_numpy(stars).to(dev)
    te = torch.full((nst, NF), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.reconstruct_field_device(lb, see, gl, l0, three, H, 12.0, pos, None, tp.data_ptr(), tsum.data_ptr(),
                                 tfit.data_ptr())
    ctx.fit_stamps_psf_device(nst, tstar.data_ptr(), nst, tp.data_ptr(), te.data_ptr())
    ctx.sync()
    assert np.array_equal(tp.cpu().numpy(), ref['psf'])
    want = ctx.fit_stamps_psf(stars, models)
    assert np.all(_status(want) == 0)
    got = te.cpu().numpy()
    assert np.array_equal(got, want)
    peak = truth[:, 0] * models.max(axis=(1, 2))
    w = dict(F=np.max(np.abs(got[:, 0] - truth[:, 0]) / truth[:, 0]), shift=np.max(np.abs(got[:, 1:3] - truth[:, 1:3])),
             back=np.max(np.abs(got[:, 3] - truth[:, 3]) / peak))
    record_margin('fit_psf', **{'chain_%s_%s' % (prec, k): v / TOL[prec] for k, v in w.items()})
    assert max(w.values()) <= TOL[prec], w
    ctx.close()
    t = api.fit_stars_with_psf(stars, models, pixscale=0.2, precision=prec)
    names = list(t.colnames if hasattr(t, 'colnames') else t.keys())
    assert names == ['scale', 'shift', 'back', 'flux', 'chi2', 'npix', 'status', 'err_scale', 'err_shift', 'err_back',
                     'err_flux']
    np.testing.assert_array_equal(np.asarray(t['scale']), want[:, 0])
    np.testing.assert_array_equal(np.asarray(t['shift']), want[:, 1:3] * 0.2)
    np.testing.assert_array_equal(np.asarray(t['back']), want[:, 3])
    np.testing.assert_array_equal(np.asarray(t['flux']), want[:, 12])
    np.testing.assert_array_equal(np.asarray(t['chi2']), want[:, 4])
    np.testing.assert_array_equal(np.asarray(t['npix']), want[:, 11].astype(int))
    np.testing.assert_array_equal(np.asarray(t['status']), want[:, 10].astype(int))
    np.testing.assert_array_equal(np.asarray(t['err_scale']), want[:, 6])
    np.testing.assert_array_equal(np.asarray(t['err_shift']), want[:, 7:9] * 0.2)
    np.testing.assert_array_equal(np.asarray(t['err_back']), want[:, 9])
    np.testing.assert_array_equal(np.asarray(t['err_flux']), want[:, 13])
    # a start in arcsec, held fixed: the shift is echoed
    t2 = api.fit_stars_with_psf(stars, models, shift=truth[:, 1:3] * 0.2, fixed_shift=True, pixscale=0.2,
                                precision=prec)
    assert np.max(np.abs(np.asarray(t2['scale']) - truth[:, 0]) / truth[:, 0]) <= TOL[prec]
    assert np.all(np.asarray(t2['err_shift']) == 0)
