"""GPU: the weighted Moffat fit of observed stars (mpsfr_fit_stamps_observed), both precisions.

1. parity with the fp64 SciPy yardstick (moffat_obs_ref) on noisy, masked stamps, all four variants, every stamp:
   each parameter within SIGMA_TOL of the SciPy minimum in units of the SciPy formal error (f64 1e-5: ten times the
   yardstick's own floor, tests/test_fit_obs_host.py; mixed 1e-2, the worst value recorded), the error columns
   within 1e-3 relative, npix equal.  Rotation: (1 - b/a) |d rot| against (1 - b/a) err_rot, the factor of
   test_gpu_fit_ell.py on both sides.
2. consistency with fit_stamps / fit_stamps_elliptical on exact Moffats and the golden stamps (var=None, no
   background), the background of a stamp without one, a constant added to a stamp.  On the golden stamps, which are
   not Moffats, the minimum of Moffat + b has b != 0 by itself (|b| up to 1.5e-3 of the peak, the SciPy minimum's
   too); there the background of every golden stamp is compared with the SciPy minimum (to TOL x peak) and its size
   printed, and b = 0 is asserted on the exact Moffats.
3. invariances: var x 4, the stored values of masked pixels, batch = single stamps, device = host pointers,
   transpose and row reversal.
4. degenerate rows, infinite pixels, bad flags.
5. a device-output reconstruct_field chained into the device form; fit_psf_cube(var=..., fit_back=True).
Margins go to record_margin('fit_obs', ...).
"""
import numpy as np
import pytest

import moffat_ell_ref as M
import moffat_obs_ref as R
from conftest import H, record_margin

pytestmark = pytest.mark.gpu

TOL = {'f64': 1e-8, 'mixed': 1e-4}            # tests/test_gpu_fit_ell.py
SIGMA_TOL = {'f64': 1e-5, 'mixed': 1e-2}
ERR_TOL = 1e-3
PRECS = ['mixed', 'f64']


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
    return fit[:, 18].astype(int)


# ---- 1. parity against the yardstick
_YARD = {}


def _yardstick(ell, back):
    if (ell, back) not in _YARD:
        data, var, _ = R.noisy_stamps(ell, back)
        _YARD[ell, back] = (data, var, [R.fit(d, va, ell, back) for d, va in zip(data, var)])
    return _YARD[ell, back]


@pytest.mark.parametrize('ell,back', R.VARIANTS)
@pytest.mark.parametrize('prec', PRECS)
def test_parity_with_scipy_on_noisy_masked_stamps(ctx, prec, ell, back):
    data, var, ref = _yardstick(ell, back)
    fit = ctx.fit_stamps_observed(data, var, background=back, circular=not ell)
    assert fit.shape == (len(data), 24)
    assert np.all(_status(fit) & 3 == 0), _status(fit)
    assert np.all(_status(fit) & 4 == 0)
    assert np.all(np.isfinite(fit))
    worst, worst_err = parity_worst(fit, ref, ell, back)
    tag = '%s_%s%s' % (prec, 'ell' if ell else 'circ', '_back' if back else '')
    print('fit_obs parity %s: worst |d| / sigma %s; worst relative error of the error columns %s' % (
        tag, {k: '%.2e' % v for k, v in worst.items()}, {k: '%.2e' % v for k, v in worst_err.items()}))
    record_margin('fit_obs', **{'sigma_%s_%s' % (tag, k): v for k, v in worst.items()})
    record_margin('fit_obs', **{'err_%s_%s' % (tag, k): v for k, v in worst_err.items()})
    assert max(worst.values()) <= SIGMA_TOL[prec], worst
    assert max(worst_err.values()) <= ERR_TOL, worst_err
    if not ell:
        assert np.array_equal(fit[:, 3], fit[:, 4]) and np.array_equal(fit[:, 7], fit[:, 8])
        assert np.array_equal(fit[:, 14], fit[:, 15]) and np.all(fit[:, 6] == 0) and np.all(fit[:, 16] == 0)
    if not back:
        assert np.all(fit[:, 21:23] == 0)


def parity_worst(fit, ref, ell, back):
    """Per fitted variable the worst |difference| in units of the yardstick's formal error and the worst relative
    difference of the error columns, of the rows `fit` against the yardstick's fits `ref`; the used pixels and chi2
    are asserted here."""
    keys = [k for k in R.KEYS if (ell or k != 'rot') and (back or k != 'back')]
    worst, worst_err = {}, {}
    for row, want in zip(fit, ref):
        assert int(row[23]) == want['npix']
        val, err = R.gpu_values(row)
        for i, k in enumerate(R.KEYS):
            if k not in keys:
                continue
            if k == 'rot':
                # (1 - b/a) |d rot| in units of (1 - b/a) err_rot
                w = 1.0 - want['ba']
                dv = w * np.rad2deg(M.rot_diff(val[i], want['val'][i]))
                sig = w * want['verr'][i]
            else:
                dv, sig = abs(val[i] - want['val'][i]), want['verr'][i]
            worst[k] = max(worst.get(k, 0.0), dv / sig)
            worst_err[k] = max(worst_err.get(k, 0.0), abs(err[i] - want['verr'][i]) / want['verr'][i])
        assert abs(row[9] - want['chi2']) <= ERR_TOL * want['chi2']
    return worst, worst_err


# ---- 2. consistency with the existing kernels
def _exact_moffats(ell):
    rng = np.random.default_rng(5)
    return np.array([M.stamp(rng.uniform(0.5, 2), *(19.5 + rng.uniform(-2, 2, 2)), fw, ba, rot, n)
                     for n in (1.8, 2.5, 4.0) for fw in (3.0, 6.0, 9.0)
                     for ba, rot in (((0.7, 40.0), (0.9, 130.0)) if ell else ((1.0, 0.0),))])


def _golden_stamps(golden):
    g, gd = golden('g9_profile'), golden('g9_profile_field')
    return np.concatenate([g['a_fin'], g['b_fin'], g['c_fin'], gd['d_fin'].reshape(-1, 40, 40)])


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _against_existing(ctx, st, ell):
    """Worst relative difference of the observed fit (var=None, no background) to the existing kernel's rows."""
    fo = ctx.fit_stamps_observed(st, None, background=False, circular=not ell)
    assert np.all(_status(fo) & 3 == 0)
    assert np.all(fo[:, 23] == 1600) and np.all(fo[:, 21:23] == 0)
    if ell:
        fe = ctx.fit_stamps_elliptical(st)
        w = {k: _rel(fo[:, i], fe[:, i]) for k, i in (('peak', 0), ('p0', 1), ('q0', 2), ('n', 5), ('fwhm_major', 7),
                                                      ('fwhm_minor', 8), ('flux', 19))}
        ba = fe[:, 8] / fe[:, 7]
        w['rot'] = float(np.max((1 - ba) * M.rot_diff(fo[:, 6], fe[:, 6])))
    else:
        fc = ctx.fit_stamps(st)
        w = {k: _rel(fo[:, i], fc[:, j]) for k, i, j in (('peak', 0, 0), ('p0', 1, 1), ('q0', 2, 2), ('n', 5, 4),
                                                         ('fwhm', 7, 5), ('alpha', 3, 3), ('flux', 19, 15))}
    return w


@pytest.mark.parametrize('ell', [False, True])
@pytest.mark.parametrize('prec', PRECS)
def test_unit_weights_give_the_existing_fits(ctx, prec, ell, golden):
    for name, st in (('exact', _exact_moffats(ell)), ('golden', _golden_stamps(golden))):
        w = _against_existing(ctx, st, ell)
        record_margin('fit_obs', **{'existing_%s_%s_%d_%s' % (name, prec, ell, k): v / TOL[prec]
                                    for k, v in w.items()})
        assert max(w.values()) <= TOL[prec], (name, w)


_GOLDEN_BACK = {}


@pytest.mark.parametrize('ell', [False, True])
@pytest.mark.parametrize('prec', PRECS)
def test_background_of_a_stamp_without_one(ctx, prec, ell, golden):
    st = _exact_moffats(ell)
    f0 = ctx.fit_stamps_observed(st, None, background=False, circular=not ell)
    fb = ctx.fit_stamps_observed(st, None, background=True, circular=not ell)
    assert np.all(_status(fb) & 3 == 0)
    worst = float(np.max(np.abs(fb[:, 21]) / fb[:, 0]))
    record_margin('fit_obs', **{'zero_background_%s_%d' % (prec, ell): worst / TOL[prec]})
    assert worst <= TOL[prec]
    for i in (0, 1, 2, 5, 7, 8):
        assert _rel(fb[:, i], f0[:, i]) <= 10 * TOL[prec], i     # (n and b are correlated: b to TOL is n to a few TOL)
    # the golden stamps are not Moffats: the minimum has its own b, the SciPy one
    gs = _golden_stamps(golden)
    fg = ctx.fit_stamps_observed(gs, None, background=True, circular=not ell)
    assert np.all(_status(fg) & 3 == 0)
    worst = 0.0
    if ell not in _GOLDEN_BACK:
        _GOLDEN_BACK[ell] = [R.fit(s, None, ell, True)['val'][7] for s in gs]
    for row, want in zip(fg, _GOLDEN_BACK[ell]):
        worst = max(worst, abs(row[21] - want) / row[0])
    print('golden stamps, %s ell=%d: |b| / peak up to %.2e, |b - b_scipy| / peak up to %.2e' % (
        prec, ell, np.max(np.abs(fg[:, 21]) / fg[:, 0]), worst))
    record_margin('fit_obs', **{'golden_background_%s_%d' % (prec, ell): worst / TOL[prec]})
    assert worst <= TOL[prec]


@pytest.mark.parametrize('ell', [False, True])
@pytest.mark.parametrize('prec', PRECS)
def test_a_constant_moves_the_background_only(ctx, prec, ell):
    st = _exact_moffats(ell)
    c = 0.03
    f0 = ctx.fit_stamps_observed(st, None, background=True, circular=not ell)
    f1 = ctx.fit_stamps_observed(st + c, None, background=True, circular=not ell)
    assert np.all(_status(f1) & 3 == 0)
    assert float(np.max(np.abs(f1[:, 21] - f0[:, 21] - c) / f0[:, 0])) <= TOL[prec]
    for i in (0, 1, 2, 5, 7, 8, 19):
        assert _rel(f1[:, i], f0[:, i]) <= 10 * TOL[prec], i
    if ell:
        ba = f0[:, 8] / f0[:, 7]
        assert float(np.max((1 - ba) * M.rot_diff(f1[:, 6], f0[:, 6]))) <= 10 * TOL[prec]


# ---- 3. invariances
@pytest.mark.parametrize('ell,back', R.VARIANTS)
@pytest.mark.parametrize('prec', PRECS)
def test_scale_of_var_changes_nothing(ctx, prec, ell, back):
    data, var, _ = R.noisy_stamps(ell, back, count=12)
    f1 = ctx.fit_stamps_observed(data, var, background=back, circular=not ell)
    f4 = ctx.fit_stamps_observed(data, 4.0 * var, background=back, circular=not ell)
    cols = [k for k in range(24) if k not in (9, 10, 18, 23)]
    den = np.where(f1[:, cols] != 0, np.abs(f1[:, cols]), 1.0)
    assert float(np.max(np.abs(f4[:, cols] - f1[:, cols]) / den)) <= TOL[prec]
    assert np.array_equal(f4[:, [18, 23]], f1[:, [18, 23]])
    assert float(np.max(np.abs(f4[:, 9] * 4.0 - f1[:, 9]) / f1[:, 9])) <= max(TOL[prec], 1e-6)


@pytest.mark.parametrize('prec', PRECS)
def test_masked_values_batches_and_device_pointers_bit_for_bit(ctx, prec):
    import torch
    data, var, _ = R.noisy_stamps(True, True, count=6)
    masked = ~R.used_pixels(data, var)
    assert masked.sum() > 6 * 9
    base = ctx.fit_stamps_observed(data, var, background=True, circular=False)
    assert np.all(_status(base) & 3 == 0)
    # the stored value of a masked pixel: NaN <-> 1e30 in the data under var = 0, and any variance under NaN data
    d2, v2 = data.copy(), var.copy()
    d2[var == 0] = 1e30
    d2[np.isnan(data)] = np.nan
    v2[np.isnan(data)] = 7.0
    assert np.array_equal(ctx.fit_stamps_observed(d2, v2, background=True, circular=False), base)
    d3, v3 = data.copy(), var.copy()
    d3[var == 0] = np.nan
    v3[np.isnan(data) & (var > 0)] = -1.0
    assert np.array_equal(ctx.fit_stamps_observed(d3, v3, background=True, circular=False), base)
    d4, v4 = data.copy(), var.copy()
    d4[var == 0] = np.inf                          # an infinite value under an invalid variance is masked too
    v4[var == 0] = np.nan
    assert np.array_equal(ctx.fit_stamps_observed(d4, v4, background=True, circular=False), base)
    # the batch is the single stamps
    for k in range(len(data)):
        one = ctx.fit_stamps_observed(data[k], var[k], background=True, circular=False)
        assert np.array_equal(one, base[k:k + 1]), k
    # device pointers
    dev = torch.device('cuda:0')
    ts = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    tv = torch.from_numpy(np.ascontiguousarray(var)).to(dev)
    tf = torch.full((len(data), 24), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_stamps_observed_device(len(data), ts.data_ptr(), tf.data_ptr(), tv.data_ptr(), background=True,
                                   circular=False)
    ctx.sync()
    assert np.array_equal(tf.cpu().numpy(), base)
    for back, circ in ((False, True), (True, True), (False, False)):
        want = ctx.fit_stamps_observed(data, None, background=back, circular=circ)
        tf.fill_(-1.0)
        torch.cuda.synchronize()
        ctx.fit_stamps_observed_device(len(data), ts.data_ptr(), tf.data_ptr(), None, background=back, circular=circ)
        ctx.sync()
        assert np.array_equal(tf.cpu().numpy(), want), (back, circ)


@pytest.mark.parametrize('prec', PRECS)
def test_transpose_and_row_reversal(ctx, prec, golden):
    gd = golden('g9_profile_field')['d_fin'].reshape(-1, 40, 40)
    syn = [M.stamp(1.0, 19.2, 20.7, 5.0, 0.8, 30.0, 2.5), M.stamp(1.5, 20.9, 18.6, 8.0, 0.6, 112.0, 3.5)]
    st = np.concatenate([gd[::5], np.array(syn)])
    st = st + 0.01 * st.max(axis=(1, 2))[:, None, None]
    p, q = np.mgrid[0:40, 0:40]
    var = np.broadcast_to(1.0 + 0.02 * p + 0.01 * q, st.shape).copy()
    st[:, 5:8, 30:34] = np.nan
    var[:, 25, 12:15] = 0.0
    kw = dict(background=True, circular=False)
    f0 = ctx.fit_stamps_observed(st, var, **kw)
    ft = ctx.fit_stamps_observed(np.transpose(st, (0, 2, 1)).copy(), np.transpose(var, (0, 2, 1)).copy(), **kw)
    fr = ctx.fit_stamps_observed(st[:, ::-1, :].copy(), var[:, ::-1, :].copy(), **kw)
    assert np.all(_status(f0) & 3 == 0) and np.all(f0[:, 23] == 1600 - 12 - 3)
    assert np.array_equal(ft[:, 23], f0[:, 23]) and np.array_equal(fr[:, 23], f0[:, 23])
    tol = 1e-9 if prec == 'f64' else TOL[prec]
    worst = 0.0
    for a, t, r in zip(f0, ft, fr):
        ba = a[8] / a[7]
        for k in (0, 5, 7, 8):                       # peak, n, fwhm_major, fwhm_minor
            worst = max(worst, abs(t[k] - a[k]) / abs(a[k]) / tol, abs(r[k] - a[k]) / abs(a[k]) / tol)
        worst = max(worst, abs(t[21] - a[21]) / a[0] / tol, abs(r[21] - a[21]) / a[0] / tol)
        worst = max(worst, abs(t[1] - a[2]) / a[2] / tol, abs(t[2] - a[1]) / a[1] / tol)
        worst = max(worst, abs(r[1] - (39.0 - a[1])) / a[1] / tol, abs(r[2] - a[2]) / a[2] / tol)
        worst = max(worst, (1 - ba) * M.rot_diff(t[6], 90.0 - a[6]) / tol,
                    (1 - ba) * M.rot_diff(r[6], 180.0 - a[6]) / tol)
    record_margin('fit_obs', **{'symmetry_%s' % prec: worst})
    assert worst <= 1.0


# ---- 4. degenerate inputs
@pytest.mark.parametrize('ell,back', R.VARIANTS)
@pytest.mark.parametrize('prec', PRECS)
def test_degenerate_rows(ctx, prec, ell, back):
    npar = 5 + 2 * ell + back
    good = M.stamp(1.0, 20.0, 19.0, 5.0, 0.8 if ell else 1.0, 40.0, 2.5) + (0.01 if back else 0.0)
    st = np.array([good] * 7)
    var = np.ones_like(st)
    st[0] = np.nan                                     # all masked
    keep = np.zeros(1600, dtype=bool)
    keep[[20 * 40 + 19 + k for k in range(npar)]] = True
    st[2] = np.where(keep.reshape(40, 40), good, np.nan)       # n_used = npar
    st[4] = 0.0                                        # all zero
    st[5, 7, 9] = np.inf                               # an infinite pixel under a valid variance
    var[6] = -1.0                                      # no valid variance
    kw = dict(background=back, circular=not ell)
    fit = ctx.fit_stamps_observed(st, var, **kw)
    assert not np.any(np.isnan(fit))
    s = _status(fit)
    assert list(s & 3) == [2, 0, 2, 0, 2, 2, 2], s
    assert list(fit[:, 23].astype(int)) == [0, 1600, npar, 1600, 1600, 1599, 0]
    # the other rows of the call are what they are alone
    alone = ctx.fit_stamps_observed(good, np.ones((40, 40)), **kw)
    assert np.array_equal(fit[1:2], alone) and np.array_equal(fit[3:4], alone)
    # -inf, with and without a variance plane
    st2 = np.array([good, good])
    st2[1, 0, 0] = -np.inf
    for va in (None, np.ones_like(st2)):
        f2 = ctx.fit_stamps_observed(st2, va, **kw)
        assert list(_status(f2) & 3) == [0, 2]
    # one used pixel more than parameters is fitted or refused, never NaN in a row that claims a minimum
    keep[20 * 40 + 19 + npar] = True
    f3 = ctx.fit_stamps_observed(np.where(keep.reshape(40, 40), good, np.nan), None, **kw)
    assert int(f3[0, 23]) == npar + 1
    assert (int(f3[0, 18]) & 3) != 0 or np.all(np.isfinite(f3))
    # the amplitude rule
    f4 = ctx.fit_stamps_observed(np.array([good * 2.0 ** 41, good * 2.0 ** -42, good * 2.0 ** 30, good * 2.0 ** -30]),
                                 None, **kw)
    assert list(_status(f4) & 3) == [2, 2, 0, 0]
    assert abs(f4[2, 5] - alone[0, 5]) <= TOL[prec] * alone[0, 5]
    # a used pixel beyond 2^60 times the brightest one (in modulus) is refused, one inside is fitted
    deep = np.array([good, good])
    deep[0, 3, 3] = -2.0 ** 62
    deep[1, 3, 3] = -2.0 ** 20
    f5 = ctx.fit_stamps_observed(deep, None, **kw)
    assert int(f5[0, 18]) & 3 == 2 and not np.any(np.isnan(f5))
    assert (int(f5[1, 18]) & 3) != 0 or np.all(np.isfinite(f5[1]))
    assert abs(f4[3, 0] / 2.0 ** -30 - alone[0, 0]) <= TOL[prec] * alone[0, 0]


def test_bad_arguments_are_refused_and_leave_the_output(api):
    import ctypes as C
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    st = np.ascontiguousarray(np.array([M.stamp(1.0, 20.0, 19.0, 5.0, 1.0, 0.0, 2.5)]))
    out = np.full((1, 24), -7.0)
    vp = C.c_void_p

    def call(n, stamps, flags, fit):
        return ctx.lib.mpsfr_fit_stamps_observed(ctx._h, n, stamps, None, flags, fit, 0)

    for args in ((1, vp(st.ctypes.data), 4, vp(out.ctypes.data)), (1, vp(st.ctypes.data), -1, vp(out.ctypes.data)),
                 (1, vp(st.ctypes.data), 7, vp(out.ctypes.data)), (0, vp(st.ctypes.data), 1, vp(out.ctypes.data)),
                 (-3, vp(st.ctypes.data), 1, vp(out.ctypes.data)), (1, None, 1, vp(out.ctypes.data)),
                 (1, vp(st.ctypes.data), 1, None)):
        assert call(*args) == -1                       # MPSFR_E_INVALID
        assert np.all(out == -7.0)
    assert call(1, vp(st.ctypes.data), 3, vp(out.ctypes.data)) == 0
    assert int(out[0, 18]) & 3 == 0 and out[0, 23] == 1600
    with pytest.raises(ValueError):
        ctx.fit_stamps_observed(st, None, background=1)
    with pytest.raises(ValueError):
        ctx.fit_stamps_observed_device(0, 1, 1)
    with pytest.raises(ValueError):
        ctx.fit_stamps_observed_device(1, 0, 1)
    ctx.close()


# ---- 5. chaining and plumbing
@pytest.mark.parametrize('prec', PRECS)
def test_reconstruct_field_device_chained_into_the_fit(api, prec):
    import torch
    dim = 256
    ps = api.grid_pixscale(dim)
    lb = np.array([500.0, 700.0, 900.0])
    see, gl, l0, three = np.array([1.0, 0.8]), np.array([0.7, 0.5]), np.array([25.0, 20.0]), np.array([0, 1])
    pos = np.array([[0.0, 0.0], [30.0, 0.0], [-20.0, 40.0]])
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    ref = ctx.reconstruct_field(lb, see, gl, l0, three, H, pos)
    dev = torch.device('cuda:0')
    tp = torch.empty(ref['psf'].shape, dtype=torch.float64, device=dev)
    ts = torch.empty(ref['psf_sum'].shape, dtype=torch.float64, device=dev)
    tf = torch.empty(ref['fit'].shape, dtype=torch.float64, device=dev)
    nst = int(np.prod(ref['psf'].shape[:-2]))
    te = torch.empty((nst, 24), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.reconstruct_field_device(lb, see, gl, l0, three, H, 12.0, pos, None, tp.data_ptr(), ts.data_ptr(),
                                 tf.data_ptr())
    ctx.fit_stamps_observed_device(nst, tp.data_ptr(), te.data_ptr(), None, background=True, circular=False)
    ctx.sync()
    assert np.array_equal(tp.cpu().numpy(), ref['psf'])
    want = ctx.fit_stamps_observed(ref['psf'], None, background=True, circular=False)
    assert np.all(_status(want) & 3 == 0)
    assert np.array_equal(te.cpu().numpy(), want)
    ctx.close()


def test_timed_under_the_profiling_id_of_the_fit(api):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    data, var, _ = R.noisy_stamps(True, True, count=4)
    ctx.set_option('profile', 1)
    ctx.profile_reset()
    ctx.fit_stamps_observed(data, var, background=True, circular=False)
    prof = ctx.profile()
    assert prof['fit'][1] == 1 and prof['fit'][0] > 0
    assert all(v[1] == 0 for k, v in prof.items() if k != 'fit'), prof
    ctx.fit_stamps_observed(data, None, background=False, circular=True)
    assert ctx.profile()['fit'][1] == 2
    ctx.close()


def test_fit_psf_cube_observed_columns(api):
    from muse_psfr_amd import psfrec
    data, var, _ = R.noisy_stamps(True, True, count=3)
    lb = np.array([500.0, 700.0, 900.0])
    ctx = psfrec.get_context(128, 0.2, 40, 'mixed', 0)
    for circular, cols in ((True, psfrec._FIT_COLS), (False, psfrec._FIT_COLS_ELL)):
        t = api.fit_psf_cube(lb, data, circular=circular, var=var, fit_back=True)
        names = list(t.colnames if hasattr(t, 'colnames') else t.keys())
        assert names == list(cols) + ['back', 'err_back', 'npix']
        want = ctx.fit_stamps_observed(data, var, background=True, circular=circular)
        np.testing.assert_array_equal(np.asarray(t['back']), want[:, 21])
        np.testing.assert_array_equal(np.asarray(t['err_back']), want[:, 22])
        np.testing.assert_array_equal(np.asarray(t['npix']), want[:, 23].astype(int))
        np.testing.assert_array_equal(np.asarray(t['fwhm']), want[:, 7:9] * 0.2)
        np.testing.assert_array_equal(np.asarray(t['n']), want[:, 5])

    class Cube:
        pass
    cube = Cube()
    cube.data = np.ma.MaskedArray(np.where(np.isnan(data), 0.0, data), mask=np.isnan(data))
    cube.var = var
    t = api.fit_psf_cube(lb, cube, circular=False, var=True, fit_back=True)
    np.testing.assert_array_equal(np.asarray(t['back']), want[:, 21])
    # unit weights with a background; the old path is untouched without var and fit_back
    clean = np.array([M.stamp(1.0, 20.0, 19.0, 5.0, 1.0, 0.0, 2.5)] * 3)
    t = api.fit_psf_cube(lb, clean, fit_back=True)
    assert np.all(np.asarray(t['npix']) == 1600)
    t0 = api.fit_psf_cube(lb, clean)
    names = list(t0.colnames if hasattr(t0, 'colnames') else t0.keys())
    assert names == list(psfrec._FIT_COLS)
