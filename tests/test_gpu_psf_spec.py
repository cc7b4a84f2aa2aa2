"""GPU: the PSF-model fit of star cubes (mpsfr_fit_spectra_psf), both precisions of a context.

1. parity with the fp64 joint yardstick (psf_spec_ref) on the shared stars and on the stars of 2 W + 3 layers, all four
   variants (background x drift), every star: theta, every F_l and b_l within SIGMA_TOL of the yardstick's minimum in
   units of its formal error, the error columns, chi2 and chi2_l within ERR_TOL relative, N_used, L, dof and the
   per-layer n_used and status equal; what a left-out layer stores changes no bit.
2. nl = 1 without drift is the problem of mpsfr_fit_stamps_psf: its rows on the shared stars of psf_fit_ref.
3. exact cases: noise-free cubes rolled by (2, -3), and an exact linear drift on knots (x = -1, 0, 1, sp = 1).
4. invariances, bit for bit; to the parity bound: the layers permuted together with x.
5. degenerate rows and refusals.
6. a device-output reconstruct_field chained into the device form; fit_star_spectra_with_psf.
7. timed under the fit's profiling id only.
Margins go to record_margin('fit_spec', ...).
"""
import ctypes as C

import numpy as np
import pytest

import psf_fit_ref as R
import psf_spec_ref as SR
from conftest import H, record_margin

pytestmark = pytest.mark.gpu

TOL = {'f64': 1e-8, 'mixed': 1e-4}            # tests/test_gpu_psf_fit.py
# f64: the value of the PSF-model fit of single stamps, ten times the floor tests/test_psf_spec_host.py asserts for the
# yardstick.  mixed: the worst value of the first GPU run was 1.37e-6 (profiles/psf_spec_fit_margins.json,
# sigma_mixed_back_drift); three times that, rounded up to one digit -- far inside 1e-2, the mixed tolerance of the
# observed fit, which it may never exceed.  (A mixed context runs the fp64 kernel: the fit has no float path, and its
# rows are those of an f64 context bit for bit, which is asserted below; the 1.37e-6 is where the descent stops telling
# chi2 values apart on the faintest stars.)
SIGMA_TOL = {'f64': 1e-5, 'mixed': 5e-6}
ERR_TOL = 1e-3
PRECS = ['mixed', 'f64']
NH, NLAY = 16, 10
IDS = ['%s-%s' % ('back' if b else 'noback', 'drift' if d else 'nodrift') for b, d in SR.VARIANTS]


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


def _groups(ss):
    """Runs of consecutive stars that one call can hold: equal nl, all with or all without a start."""
    out = []
    for k, s in enumerate(ss):
        key = (len(s['cube']), s['shift'] is None)
        if out and out[-1][0] == key:
            out[-1][1].append(k)
        else:
            out.append((key, [k]))
    return [ks for _, ks in out]


def _fit(ctx, ss, back, drift):
    """(head, layers) per star of a list of shared stars."""
    res = [None] * len(ss)
    for ks in _groups(ss):
        cubes, var, psf, sh = SR.batch([ss[k] for k in ks])
        head, lay = ctx.fit_spectra_psf(cubes, psf, var=var, shift=sh, background=back,
                                        x=ss[ks[0]]['x'] if drift else None)
        for i, k in enumerate(ks):
            res[k] = (head[i], lay[i])
    return res


def _compare(head, lay, ref, prob):
    """Worst differences of a row against the yardstick: (sigma units, error columns, chi2) and the exact fields."""
    nt, fl = prob.nt, prob.layers
    sig = np.max(np.abs(head[:nt] - ref['theta'][:nt]) / ref['err_theta'][:nt])
    sig = max(sig, np.max(np.abs(lay[fl, 0] - ref['F'][fl]) / ref['err_F'][fl]))
    err = np.max(np.abs(head[4:4 + nt] - ref['err_theta'][:nt]) / ref['err_theta'][:nt])
    err = max(err, np.max(np.abs(lay[fl, 2] - ref['err_F'][fl]) / ref['err_F'][fl]))
    if prob.back:
        sig = max(sig, np.max(np.abs(lay[fl, 1] - ref['b'][fl]) / ref['err_b'][fl]))
        err = max(err, np.max(np.abs(lay[fl, 3] - ref['err_b'][fl]) / ref['err_b'][fl]))
    chi = max(abs(head[8] - ref['chi2']) / ref['chi2'], np.max(np.abs(lay[fl, 6] - ref['chi2_l'][fl]) / ref['chi2_l'][fl]))
    assert int(head[11]) == ref['npix'] and int(head[12]) == ref['nlayers'] and int(head[13]) == ref['dof']
    assert np.array_equal(lay[:, 7].astype(int), prob.n_used)
    assert np.array_equal(lay[:, 8].astype(int), np.where(prob.fitted, 0, 2))
    out = ~prob.fitted
    assert np.all(lay[out][:, [0, 1, 2, 3, 4, 5, 6, 9]] == 0)
    assert head[14] == 0 and head[15] == 0 and np.all(lay[:, 9] == 0)
    if nt == 2:
        assert np.all(head[2:4] == 0) and np.all(head[6:8] == 0)
    if not prob.back:
        assert np.all(lay[:, 1] == 0) and np.all(lay[:, 3] == 0)
    sums = prob.psfs.sum(axis=(1, 2))
    assert np.max(np.abs(lay[fl, 4] - lay[fl, 0] * sums[fl]) / np.abs(lay[fl, 4])) <= 1e-13
    assert np.max(np.abs(lay[fl, 5] - lay[fl, 2] * np.abs(sums[fl])) / lay[fl, 5]) <= 1e-13
    return float(sig), float(err), float(chi)


# ---- 1. parity against the yardstick
@pytest.mark.parametrize('back,drift', SR.VARIANTS, ids=IDS)
@pytest.mark.parametrize('prec', PRECS)
def test_parity_with_the_joint_yardstick(ctx, prec, back, drift):
    tag = '%s%s%s' % (prec, '_back' if back else '', '_drift' if drift else '')
    for uneven in (False, True):
        ss, refs = SR.yardstick(back, drift, uneven)
        rows = _fit(ctx, ss, back, drift)
        worst = [0.0, 0.0, 0.0]
        its = []
        for s, ref, (head, lay) in zip(ss, refs, rows):
            assert int(head[10]) == 0, head
            assert np.all(np.isfinite(head)) and np.all(np.isfinite(lay))
            prob = SR.problem(s, back, drift)
            assert prob.inside(head[:4])
            worst = [max(a, b) for a, b in zip(worst, _compare(head, lay, ref, prob))]
            its.append(int(head[9]))
        name = tag + ('_uneven' if uneven else '')
        print('fit_spec parity %s: worst |d| / sigma %.2e; error columns %.2e, chi2 %.2e relative; iterations %s' % (
            name, worst[0], worst[1], worst[2], its))
        record_margin('fit_spec', **{'sigma_' + name: worst[0], 'err_' + name: worst[1], 'chi2_' + name: worst[2]})
        assert worst[0] <= SIGMA_TOL[prec]
        assert worst[1] <= ERR_TOL and worst[2] <= ERR_TOL


def test_a_mixed_context_gives_the_rows_of_an_f64_one(api):
    ss = SR.stars(True, True)
    got = {}
    for prec in PRECS:
        c = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision=prec)
        got[prec] = _fit(c, ss, True, True)
        c.close()
    for (h0, l0), (h1, l1) in zip(got['mixed'], got['f64']):
        assert np.array_equal(h0, h1) and np.array_equal(l0, l1)


@pytest.mark.parametrize('prec', PRECS)
def test_what_a_left_out_layer_stores_does_not_matter(ctx, prec):
    k, l = SR.NAN_LAYER
    for back, drift in ((True, False), (False, True)):
        s = SR.stars(back, drift)[k]
        x = s['x'] if drift else None
        want = ctx.fit_spectra_psf(s['cube'], s['psfs'], var=s['var'], background=back, x=x)
        assert want[1][0, l, 8] == 2 and want[1][0, l, 7] == 0 and want[0][0, 10] == 0 and want[0][0, 12] == len(s['x']) - 1
        rng = np.random.default_rng(5)
        for kind in range(3):
            cube, var, psfs = s['cube'].copy(), s['var'].copy(), s['psfs'].copy()
            if kind == 0:                     # finite garbage under invalid variances
                cube[l] = rng.normal(size=(40, 40)) * 1e30
                var[l] = np.where(rng.uniform(size=(40, 40)) < 0.5, 0.0, np.nan)
            elif kind == 1:                   # infinities under NaN variances, a huge model stamp
                cube[l] = np.inf
                var[l] = np.nan
                psfs[l] = psfs[l] * 1e6
            else:                             # a valid layer whose model stamp is not finite: left out as well
                cube[l] = s['cube'][0]
                var[l] = s['var'][0]
                psfs[l, 3, 4] = np.nan
            got = ctx.fit_spectra_psf(cube, psfs, var=var, background=back, x=x)
            assert np.array_equal(got[0], want[0])
            keep = [i for i in range(len(cube)) if i != l]
            assert np.array_equal(got[1][0, keep], want[1][0, keep])
            assert got[1][0, l, 8] == 2 and np.all(got[1][0, l, :7] == 0)


# ---- 2. one layer is the fit of single stamps
@pytest.mark.parametrize('back', [False, True])
@pytest.mark.parametrize('prec', PRECS)
def test_one_layer_is_the_fit_of_single_stamps(ctx, prec, back):
    data, var, psf, truth, _, ref = R.yardstick(back, False)
    single = ctx.fit_stamps_psf(data, psf, var=var, background=back)
    head, lay = ctx.fit_spectra_psf(data[:, None], psf[:, None], var=var[:, None], background=back)
    assert np.all(head[:, 10] == 0) and np.all(single[:, 10] == 0)
    assert np.array_equal(head[:, 11], single[:, 11]) and np.all(head[:, 12] == 1)
    assert np.array_equal(lay[:, 0, 7], single[:, 11])
    worst, worst_err = 0.0, 0.0
    for k, want in enumerate(ref):
        val = np.array([lay[k, 0, 0], head[k, 0], head[k, 1], lay[k, 0, 1]])
        err = np.array([lay[k, 0, 2], head[k, 4], head[k, 5], lay[k, 0, 3]])
        free = want['free']
        worst = max(worst, np.max(np.abs(val - single[k, 0:4])[free] / want['err'][free]),
                    np.max(np.abs(val - want['x'])[free] / want['err'][free]))
        worst_err = max(worst_err, np.max(np.abs(err - single[k, 6:10])[free] / single[k, 6:10][free]),
                        abs(head[k, 8] - single[k, 4]) / single[k, 4], abs(lay[k, 0, 6] - single[k, 4]) / single[k, 4],
                        abs(lay[k, 0, 4] - single[k, 12]) / abs(single[k, 12]),
                        abs(lay[k, 0, 5] - single[k, 13]) / single[k, 13])
    tag = '%s%s' % (prec, '_back' if back else '')
    print('fit_spec one layer %s: worst |d| / sigma %.2e, errors and chi2 %.2e relative' % (tag, worst, worst_err))
    record_margin('fit_spec', **{'single_sigma_' + tag: worst, 'single_err_' + tag: worst_err})
    # (the single-stamp fit of a mixed context has its own bound against the yardstick: both differences are inside
    # the sum of the two)
    assert worst <= SIGMA_TOL[prec] + (2e-6 if prec == 'mixed' else 0.0)
    assert worst_err <= ERR_TOL


# ---- 3. exact cases
def _compact_cube():
    """Three Moffat stamps (sum 1) with wings below 1e-12 of the peak 16 pixels from the centre: the layers of a cube."""
    st = np.array([R.moffat(20.0, 20.0, fw, n) for fw, n in ((2.5, 30.0), (3.0, 30.0), (4.0, 40.0))])
    return st / st.sum(axis=(1, 2))[:, None, None]


@pytest.mark.parametrize('prec', PRECS)
def test_rolled_cubes_and_an_exact_drift_come_back(ctx, prec):
    P = _compact_cube()
    F = np.array([[3.0, 700.0, 0.02], [40.0, 50.0, 60.0]])
    peak = F * P.max(axis=(1, 2))[None]
    b = np.array([[0.01, -0.005, 0.03], [0.0, 0.02, -0.01]]) * peak
    psf = np.array([P, P])
    x = np.array([-1.0, 0.0, 1.0])
    for drift, sp in ((False, (0, 0)), (True, (0, 0)), (True, (1, 0)), (True, (1, -1))):
        cubes = np.array([[F[s, l] * np.roll(P[l], (2 + sp[0] * int(x[l]), -3 + sp[1] * int(x[l])), axis=(0, 1)) + b[s, l]
                           for l in range(3)] for s in range(2)])
        head, lay = ctx.fit_spectra_psf(cubes, psf, background=True, x=x if drift else None)
        assert np.all(head[:, 10] == 0), head
        assert np.all(np.isfinite(head)) and np.all(np.isfinite(lay))
        assert np.all(head[:, 11] == 4800) and np.all(head[:, 12] == 3) and np.all(lay[:, :, 7] == 1600)
        want = np.array([2.0, -3.0, sp[0], sp[1]])
        w = dict(F=np.max(np.abs(lay[:, :, 0] - F) / F), back=np.max(np.abs(lay[:, :, 1] - b) / peak),
                 theta=np.max(np.abs(head[:, :4] - want)))
        record_margin('fit_spec', **{'exact_%s_%d%d%d_%s' % (prec, drift, sp[0], sp[1], k): v / TOL[prec]
                                     for k, v in w.items()})
        assert max(w.values()) <= TOL[prec], (drift, sp, w)
        if not drift:
            h0, l0 = ctx.fit_spectra_psf(cubes - b[:, :, None, None], psf, background=False)
            assert np.all(h0[:, 10] == 0)
            assert np.max(np.abs(l0[:, :, 0] - F) / F) <= TOL[prec] and np.max(np.abs(h0[:, :2] - want[:2])) <= TOL[prec]


# ---- 4. invariances
def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('back,drift', [(True, True), (False, False)], ids=['back-drift', 'noback-nodrift'])
@pytest.mark.parametrize('prec', PRECS)
def test_scalings_and_unused_pixels_change_exactly_what_they_should(ctx, prec, back, drift):
    ss = SR.stars(back, drift)[2:4]                       # two stars of five layers with a given start
    cubes, var, psf, sh = SR.batch(ss)
    x = ss[0]['x'] if drift else None
    kw = dict(shift=sh, background=back, x=x)
    base = ctx.fit_spectra_psf(cubes, psf, var=var, **kw)
    assert np.all(base[0][:, 10] == 0)
    # a constant factor on var: chi2 alone changes, by that factor
    got = ctx.fit_spectra_psf(cubes, psf, var=var * 4.0, **kw)
    h, la = base[0].copy(), base[1].copy()
    h[:, 8] /= 4.0
    la[:, :, 6] /= 4.0
    assert _same(got, (h, la))
    # 2^k on the data with 4^k on var
    for k in (20, -20):
        got = ctx.fit_spectra_psf(cubes * 2.0 ** k, psf, var=var * 4.0 ** k, **kw)
        h, la = base[0].copy(), base[1].copy()
        la[:, :, :6] *= 2.0 ** k
        assert _same(got, (h, la))
    # 2^7 on one layer's model: that layer's F and err_F, by 2^-7
    p2 = psf.copy()
    p2[:, 3] *= 2.0 ** 7
    got = ctx.fit_spectra_psf(cubes, p2, var=var, **kw)
    h, la = base[0].copy(), base[1].copy()
    la[:, 3, 0] *= 2.0 ** -7
    la[:, 3, 2] *= 2.0 ** -7
    assert _same(got, (h, la))
    # garbage in unused pixels
    c2, v2 = cubes.copy(), var.copy()
    un = ~(np.isfinite(cubes) & np.isfinite(var) & (var > 0))
    rng = np.random.default_rng(3)
    c2[un] = rng.normal(size=int(un.sum())) * 1e20
    v2[un] = np.where(rng.uniform(size=int(un.sum())) < 0.5, -1.0, np.inf)
    assert _same(ctx.fit_spectra_psf(c2, psf, var=v2, **kw), base)


@pytest.mark.parametrize('prec', PRECS)
def test_a_row_depends_on_its_star_alone(ctx, prec):
    import torch
    back, drift = True, True
    ss = SR.stars(back, drift)[:4]                        # five layers each
    cubes = np.array([s['cube'] for s in ss])
    var = np.array([s['var'] for s in ss])
    psf = np.array([s['psfs'] for s in ss])
    sh = np.array([np.round(s['truth']['theta'][:2] * 2) / 2 for s in ss])
    x = ss[0]['x']
    kw = dict(background=back, x=x)
    base = ctx.fit_spectra_psf(cubes, psf, var=var, shift=sh, **kw)
    # alone, and in the reversed batch
    for k in range(4):
        one = ctx.fit_spectra_psf(cubes[k], psf[k], var=var[k], shift=sh[k:k + 1], **kw)
        assert np.array_equal(one[0][0], base[0][k]) and np.array_equal(one[1][0], base[1][k])
    rev = ctx.fit_spectra_psf(cubes[::-1], psf[::-1], var=var[::-1], shift=sh[::-1], **kw)
    assert _same((rev[0][::-1], rev[1][::-1]), base)
    # shared model cubes through psf_index against copies
    shared = ctx.fit_spectra_psf(cubes, psf[:2], var=var, psf_index=[0, 1, 0, 1], shift=sh, **kw)
    copies = ctx.fit_spectra_psf(cubes, psf[[0, 1, 0, 1]], var=var, shift=sh, **kw)
    assert _same(shared, copies)
    assert np.array_equal(shared[0][:2], base[0][:2])
    # device pointers against host pointers
    dev = torch.device('cuda:0')
    tc, tv, tp = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (cubes, var, psf))
    tsh = torch.from_numpy(sh).to(dev)
    tf = torch.full((4, NH + NLAY * 5), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_spectra_psf_device(4, 5, tc.data_ptr(), 4, tp.data_ptr(), tf.data_ptr(), var_ptr=tv.data_ptr(),
                               shift_ptr=tsh.data_ptr(), **kw)
    ctx.sync()
    got = tf.cpu().numpy()
    assert np.array_equal(got[:, :NH], base[0]) and np.array_equal(got[:, NH:].reshape(4, 5, NLAY), base[1])
    # the layers permuted together with x: the same problem, to the parity bound
    perm = np.array([3, 0, 4, 1, 2])
    ph, pl = ctx.fit_spectra_psf(cubes[:, perm], psf[:, perm], var=var[:, perm], shift=sh, background=back, x=x[perm])
    worst = 0.0
    for k in range(4):
        fl = base[1][k, :, 8] == 0
        worst = max(worst, np.max(np.abs(ph[k, :4] - base[0][k, :4]) / base[0][k, 4:8]),
                    np.max(np.abs(pl[k][np.argsort(perm)][fl, 0] - base[1][k, fl, 0]) / base[1][k, fl, 2]),
                    np.max(np.abs(pl[k][np.argsort(perm)][fl, 1] - base[1][k, fl, 1]) / base[1][k, fl, 3]))
        assert np.array_equal(pl[k][np.argsort(perm)][:, 7:9], base[1][k, :, 7:9])
    record_margin('fit_spec', **{'permuted_sigma_' + prec: worst})
    assert worst <= SIGMA_TOL[prec]


# ---- 5. degenerate rows and refusals
@pytest.mark.parametrize('prec', PRECS)
def test_degenerate_rows(ctx, prec):
    P = SR.model_cube(3)
    x = np.array([-1.0, 0.0, 1.0])
    good = np.array([100.0 * (l + 1) * R.resample(P[l], 1.0, -1.0) + 0.5 for l in range(3)])

    def status2(head, lay, nused, nfit):
        assert int(head[10]) == 2 and int(head[11]) == nused and int(head[12]) == nfit
        assert np.all(np.delete(head, [10, 11, 12]) == 0)
        assert np.all(lay[:, [0, 1, 2, 3, 4, 5, 6, 9]] == 0)

    for back, drift in SR.VARIANTS:
        kw = dict(background=back, x=x if drift else None)
        nlin, nt = (2 if back else 1), (4 if drift else 2)
        h, la = ctx.fit_spectra_psf(good, P, **kw)
        assert h[0, 10] == 0 and np.all(la[0, :, 8] == 0) and h[0, 13] == 4800 - nt - 3 * nlin
        # all layers NaN
        h, la = ctx.fit_spectra_psf(np.full((3, 40, 40), np.nan), P, **kw)
        status2(h[0], la[0], 0, 0)
        assert np.all(la[0, :, 8] == 2) and np.all(la[0, :, 7] == 0)
        # an all-zero model cube
        h, la = ctx.fit_spectra_psf(good, np.zeros_like(P), **kw)
        status2(h[0], la[0], 0, 0)
        assert np.all(la[0, :, 8] == 2) and np.all(la[0, :, 7] == 1600)
        # all fitted layers at one x: only layer 1 survives
        c = good.copy()
        c[0] = np.nan
        c[2] = np.nan
        h, la = ctx.fit_spectra_psf(c, P, **kw)
        if drift:
            status2(h[0], la[0], 1600, 1)
        else:
            assert h[0, 10] == 0 and h[0, 12] == 1
        assert list(la[0, :, 8]) == [2, 0, 2]
        # dof < 1: nlin + 1 used pixels in each of two layers
        c = np.full((3, 40, 40), np.nan)
        c[0, 19:21, 19:21].flat[:nlin + 1] = good[0, 19:21, 19:21].flat[:nlin + 1]
        c[2, 19:21, 19:21].flat[:nlin + 1] = good[2, 19:21, 19:21].flat[:nlin + 1]
        h, la = ctx.fit_spectra_psf(c, P, **kw)
        if 2 * (nlin + 1) - (nt + 2 * nlin) < 1:
            status2(h[0], la[0], 2 * (nlin + 1), 2)
        assert list(la[0, :, 8]) == [0, 2, 0] and list(la[0, :, 7]) == [nlin + 1, 0, nlin + 1]
        # an infinite pixel under a valid variance: that layer is left out
        c = good.copy()
        c[1, 5, 5] = np.inf
        h, la = ctx.fit_spectra_psf(c, P, **kw)
        assert h[0, 10] == 0 and list(la[0, :, 8]) == [0, 2, 0] and h[0, 11] == 3200
        # the amplitude rule of the star
        for k, st in ((41, 2), (-48, 2), (30, 0)):
            h, la = ctx.fit_spectra_psf(good * 2.0 ** k, P, **kw)
            assert h[0, 10] == st, (k, h[0])


@pytest.mark.parametrize('prec', PRECS)
def test_a_star_12_px_from_its_model_rests_on_the_bound(ctx, prec):
    Pm = R.moffat(20.0, 20.0, 4.0, 2.5)
    Pm /= Pm.sum()
    P = np.array([Pm, Pm, Pm])
    cubes = np.array([[50.0 * (l + 1) * R.moffat(32.0, 20.0, 4.0, 2.5) + 0.1 for l in range(3)],
                      [50.0 * (l + 1) * R.moffat(20.0, 8.0, 4.0, 2.5) + 0.1 for l in range(3)]])
    for back in (False, True):
        head, lay = ctx.fit_spectra_psf(cubes, np.array([P, P]), background=back)
        assert list(head[:, 10]) == [1, 1], (back, head)
        assert np.all(np.isfinite(head)) and np.all(np.isfinite(lay))
        assert head[0, 0] == 8.0 and head[1, 1] == -8.0


def test_bad_arguments_are_refused_and_leave_the_output(api):
    import torch
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    P = SR.model_cube(3)
    cu = np.ascontiguousarray(np.array([3.0 * P, 2.0 * P]))
    ps = np.ascontiguousarray(np.array([P, P]))
    out = np.full((2, NH + NLAY * 3), -7.0)
    ix = np.array([0, 1], dtype=np.int32)
    sh = np.zeros((2, 2))
    xs = np.array([-1.0, 0.0, 1.0])
    vp = C.c_void_p

    def ptr(a):
        return None if a is None else vp(a.ctypes.data)

    def call(nstar=2, nl=3, cubes=cu, var=None, npsf=2, psf=ps, index=None, shift=None, x=None, flags=1, fit=out):
        return ctx.lib.mpsfr_fit_spectra_psf(ctx._h, nstar, nl, ptr(cubes), ptr(var), npsf, ptr(psf), ptr(index),
                                             ptr(shift), ptr(x), flags, ptr(fit), 0)

    bad = (dict(nstar=0), dict(nstar=-1), dict(nl=0), dict(nl=4097), dict(cubes=None), dict(psf=None), dict(fit=None),
           dict(flags=2), dict(flags=3), dict(flags=4), dict(flags=5), dict(flags=8), dict(flags=9), dict(flags=32),
           dict(flags=-1),                                                       # refused and unknown bits
           dict(flags=16), dict(flags=17),                                       # drift without x
           dict(flags=17, x=np.array([0.5, 0.5, 0.5])), dict(flags=17, x=np.array([-1.0, 0.0, 1.5])),
           dict(flags=17, x=np.array([-1.0, np.nan, 1.0])), dict(flags=16, x=np.array([-1.0, 0.0, np.inf])),
           dict(flags=17, nl=1, x=xs),                                           # drift with one layer
           dict(npsf=1),                                                         # no index, npsf != nstar
           dict(index=np.array([0, 2], dtype=np.int32)), dict(index=np.array([-1, 0], dtype=np.int32)),
           dict(shift=np.array([[0.0, np.nan], [0.0, 0.0]])), dict(shift=np.array([[8.5, 0.0], [0.0, 0.0]])),
           dict(shift=np.array([[0.0, 0.0], [0.0, -8.01]])))
    for kw in bad:
        assert call(**kw) == -1, kw                    # MPSFR_E_INVALID
        assert np.all(out == -7.0), kw
    for kw in (dict(), dict(index=ix, shift=sh), dict(npsf=1, index=np.zeros(2, dtype=np.int32)), dict(flags=0),
               dict(flags=17, x=xs), dict(flags=16, x=xs), dict(x=np.array([np.nan] * 3))):        # x ignored without drift
        out[:] = -7.0
        assert call(**kw) == 0, kw
        assert np.all(out[:, 10] == 0) and np.all(out[:, 11] == 4800) and np.all(out[:, 12] == 3), kw
        assert np.max(np.abs(out[:, NH::NLAY] - np.array([[3.0], [2.0]]))) <= 1e-8 and np.max(np.abs(out[:, :4])) <= 1e-8
    with pytest.raises(ValueError):
        ctx.fit_spectra_psf(cu, ps, background=1)
    with pytest.raises(ValueError):
        ctx.fit_spectra_psf(cu, ps[:1])
    with pytest.raises(ValueError):
        ctx.fit_spectra_psf(cu, ps, x=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        ctx.fit_spectra_psf_device(0, 3, 1, 1, 1, 1)
    with pytest.raises(ValueError):
        ctx.fit_spectra_psf_device(2, 3, 1, 1, 1, 1)       # no index, npsf != nstar
    with pytest.raises(ValueError):
        ctx.fit_spectra_psf_device(2, 0, 1, 2, 1, 1)
    with pytest.raises(ValueError):
        ctx.fit_spectra_psf_device(2, 3, 1, 2, 0, 1)
    # the device form: an index out of range or a start outside the domain is that row's status 2, nothing else
    dev = torch.device('cuda:0')
    tc, tp = torch.from_numpy(np.concatenate([cu, cu])).to(dev), torch.from_numpy(ps).to(dev)
    want = ctx.fit_spectra_psf(cu, ps, shift=sh, x=xs)
    for tix, tsh, stat in (([0, 2, -1, 1], [[0.0, 0.0]] * 4, [0, 2, 2, 0]),
                           ([0, 1, 0, 1], [[0.0, 0.0], [float('nan'), 0.0], [0.0, 9.0], [0.0, 0.0]], [0, 2, 2, 0])):
        ti = torch.tensor(tix, dtype=torch.int32, device=dev)
        ts = torch.tensor(tsh, dtype=torch.float64, device=dev)
        tf = torch.full((4, NH + NLAY * 3), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.fit_spectra_psf_device(4, 3, tc.data_ptr(), 2, tp.data_ptr(), tf.data_ptr(), psf_index_ptr=ti.data_ptr(),
                                   shift_ptr=ts.data_ptr(), x=xs)
        ctx.sync()
        got = tf.cpu().numpy()
        assert list(got[:, 10].astype(int)) == stat and not np.any(np.isnan(got))
        assert np.array_equal(got[0, :NH], want[0][0]) and np.array_equal(got[3, :NH], want[0][1])
        assert np.array_equal(got[0, NH:], want[1][0].ravel()) and np.array_equal(got[3, NH:], want[1][1].ravel())
        for k in (1, 2):
            assert np.all(np.delete(got[k, :NH], [10, 11, 12]) == 0)
    ctx.close()


# ---- 7. timing
def test_timed_under_the_profiling_id_of_the_fit(api):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    cubes, var, psf, sh = SR.batch(SR.stars(True, True)[:2])
    ctx.set_option('profile', 1)
    ctx.profile_reset()
    ctx.fit_spectra_psf(cubes, psf, var=var, x=SR.stars(True, True)[0]['x'])
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
    lb = np.array([500.0, 700.0, 900.0])
    see, gl, l0, three = np.array([1.0, 0.8]), np.array([0.7, 0.5]), np.array([25.0, 20.0]), np.array([0, 1])
    pos = np.array([[0.0, 0.0], [-20.0, 40.0]])
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    ref = ctx.reconstruct_field(lb, see, gl, l0, three, H, pos)
    models = ref['psf'].reshape(-1, 3, 40, 40)
    nst = len(models)
    assert nst == 4
    rng = np.random.default_rng(8)
    theta = np.column_stack([rng.uniform(-3, 3, (nst, 2)), rng.uniform(-0.4, 0.4, (nst, 2))])
    F = rng.uniform(100, 1000, (nst, 3))
    back = rng.uniform(-0.01, 0.03, (nst, 3))
    x = np.array([-1.0, 0.0, 1.0])
    cubes = np.array([[R.model(models[s, l], (F[s, l], theta[s, 0] + theta[s, 2] * x[l], theta[s, 1] + theta[s, 3] * x[l],
                                              back[s, l])) for l in range(3)] for s in range(nst)])
    dev = torch.device('cuda:0')
    tp = torch.empty(ref['psf'].shape, dtype=torch.float64, device=dev)
    tsum = torch.empty(ref['psf_sum'].shape, dtype=torch.float64, device=dev)
    tfit = torch.empty(ref['fit'].shape, dtype=torch.float64, device=dev)
    tcube = torch.from_numpy(cubes).to(dev)
    te = torch.full((nst, NH + NLAY * 3), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.reconstruct_field_device(lb, see, gl, l0, three, H, 12.0, pos, None, tp.data_ptr(), tsum.data_ptr(),
                                 tfit.data_ptr())
    ctx.fit_spectra_psf_device(nst, 3, tcube.data_ptr(), nst, tp.data_ptr(), te.data_ptr(), x=x)
    ctx.sync()
    assert np.array_equal(tp.cpu().numpy(), ref['psf'])
    want = ctx.fit_spectra_psf(cubes, models, x=x)
    assert np.all(want[0][:, 10] == 0)
    got = te.cpu().numpy()
    assert np.array_equal(got[:, :NH], want[0]) and np.array_equal(got[:, NH:].reshape(nst, 3, NLAY), want[1])
    peak = F * models.max(axis=(2, 3))
    w = dict(F=np.max(np.abs(want[1][:, :, 0] - F) / F), theta=np.max(np.abs(want[0][:, :4] - theta)),
             back=np.max(np.abs(want[1][:, :, 1] - back) / peak))
    record_margin('fit_spec', **{'chain_%s_%s' % (prec, k): v / TOL[prec] for k, v in w.items()})
    assert max(w.values()) <= TOL[prec], w
    ctx.close()
    t = api.fit_star_spectra_with_psf(cubes, models, lb, drift=True, pixscale=0.2, precision=prec)
    names = list(t.colnames if hasattr(t, 'colnames') else t.keys())
    assert names == ['shift', 'err_shift', 'drift', 'err_drift', 'chi2', 'npix', 'nlayers', 'status', 'flux', 'err_flux',
                     'scale', 'back', 'layer_status', 'lbda']
    head, lay = want
    np.testing.assert_array_equal(np.asarray(t['shift']), head[:, 0:2] * 0.2)
    np.testing.assert_array_equal(np.asarray(t['err_shift']), head[:, 4:6] * 0.2)
    np.testing.assert_array_equal(np.asarray(t['drift']), head[:, 2:4] * 0.2)
    np.testing.assert_array_equal(np.asarray(t['err_drift']), head[:, 6:8] * 0.2)
    np.testing.assert_array_equal(np.asarray(t['chi2']), head[:, 8])
    np.testing.assert_array_equal(np.asarray(t['npix']), head[:, 11].astype(int))
    np.testing.assert_array_equal(np.asarray(t['nlayers']), head[:, 12].astype(int))
    np.testing.assert_array_equal(np.asarray(t['status']), head[:, 10].astype(int))
    np.testing.assert_array_equal(np.asarray(t['flux']), lay[:, :, 4])
    np.testing.assert_array_equal(np.asarray(t['err_flux']), lay[:, :, 5])
    np.testing.assert_array_equal(np.asarray(t['scale']), lay[:, :, 0])
    np.testing.assert_array_equal(np.asarray(t['back']), lay[:, :, 1])
    np.testing.assert_array_equal(np.asarray(t['layer_status']), lay[:, :, 8].astype(int))
    np.testing.assert_array_equal(np.asarray(t['lbda']), np.tile(lb, (nst, 1)))
    # a start in arcsec, no drift on cubes without one
    flat = np.array([[R.model(models[s, l], (F[s, l], theta[s, 0], theta[s, 1], 0.0)) for l in range(3)]
                     for s in range(nst)])
    t2 = api.fit_star_spectra_with_psf(flat, models, lb, shift=np.round(theta[:, :2]) * 0.2, fit_back=False, pixscale=0.2,
                                       precision=prec)
    assert np.max(np.abs(np.asarray(t2['scale']) - F) / F) <= TOL[prec]
    assert np.max(np.abs(np.asarray(t2['shift']) - theta[:, :2] * 0.2)) <= TOL[prec]
    assert np.all(np.asarray(t2['drift']) == 0) and np.all(np.asarray(t2['err_drift']) == 0)
