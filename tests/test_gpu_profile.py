"""GPU: multi-layer Cn2 profiles with per-layer wind (mpsfr_reconstruct_profile, mpsfr_simul_psd_profile).

1. the PSD of a profile against the reference's dsp4muse (tests/golden/g9_profile.npz, tools/make_golden_profile.py);
2. the two-layer profile of the reference is the legacy call, bit for bit (averaged, field, both precisions, three
   grids, the full-size stage A at L0 = 5 m);
3. invariances: a layer of weight 0, a layer split in two, the field spread of a ground layer against a high one;
4. forms: batch against single rows, device and asynchronous outputs against host outputs;
5. the table cache across profile and legacy calls on one context.
"""
import numpy as np
import pytest

from conftest import H, rel_err

pytestmark = pytest.mark.gpu

REF_DIR = (0.628163, -0.326497)
LB = np.array([490.0, 600.0, 750.0, 930.0])
ROWS = (np.array([1.0, 0.6, 0.8]), np.array([0.7, 0.4, 0.55]), np.array([25.0, 12.0, 18.0]), np.array([0, 1, 0]))
FIELD5 = [(0.0, 0.0), (30.0, 0.0), (-30.0, 0.0), (0.0, 45.0), (-50.0, -50.0)]


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _same_all(r, ref):
    for k in ('psf', 'psf_sum', 'fit'):
        assert _same(r[k], ref[k]), k


def _masks(ref_masks):
    # the reference's [i_fx][j_fy] masks, as the library takes them
    return ref_masks


# ---- 1. PSD against the reference
@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd'])
@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_psd_matches_reference_profiles(api, golden, ref_masks, case, prec):
    g = golden('g9_profile_field' if case == 'd' else 'g9_profile')
    dim = 512
    ctx = api.Context(dim=dim, pixscale=api.grid_pixscale(dim), precision=prec)
    kw = dict(three_lgs=bool(g[case + '_three']), masks=_masks(ref_masks))
    npl = int(g[case + '_npsflin'])
    if npl:
        kw['npsflin'] = npl
    else:
        kw['positions'] = g[case + '_dirs'].T
    see, l0 = float(g[case + '_seeing']), float(g[case + '_L0'])
    psd = ctx.simul_psd_profile(see, l0, g[case + '_cn2'], g[case + '_h'], g[case + '_ws'], g[case + '_wd'], **kw)
    sl = slice(dim // 2 - 40, dim // 2 + 40)
    zone = g[case + '_zone']
    assert psd.shape == (zone.shape[0], dim, dim)
    assert rel_err(psd[:, sl, sl], zone) <= 1e-12
    # outside the zone the PSD is the fitting term, the legacy call's
    leg = ctx.simul_psd(see, 0.5, l0, kw['three_lgs'], H, npsflin=1, masks=_masks(ref_masks))[0]
    out = np.ones((dim, dim), bool)
    out[sl, sl] = False
    for d in range(psd.shape[0]):
        assert rel_err(psd[d][out], leg[out]) <= 1e-12
    ctx.close()


# ---- 1b. stamps and fits against the reference (psf_muse, convolve_final_psf, the oracle's Moffat fit), at the
# tolerances of tests/test_gpu_parity.py: stamps relative to their maximum, fwhm [arcsec] and beta absolute
TOL = {'f64': dict(stamp=1e-9, fit=1e-6), 'mixed': dict(stamp=2e-5, fit=1e-4)}


@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd'])
@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_stamps_and_fits_match_reference_profiles(api, golden, ref_masks, case, prec):
    g = golden('g9_profile_field' if case == 'd' else 'g9_profile')
    dim = int(g[case + '_dim'])
    ps = api.grid_pixscale(dim)
    lb = g[case + '_lbda']
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    npl = int(g[case + '_npsflin'])
    kw = dict(npsflin=npl) if npl else dict(positions=g[case + '_dirs'].T)
    r = ctx.reconstruct_profile(lb, [float(g[case + '_seeing'])], [float(g[case + '_gl'])], [float(g[case + '_L0'])],
                                g[case + '_cn2'], g[case + '_h'], g[case + '_ws'], g[case + '_wd'],
                                three_lgs=[int(g[case + '_three'])], masks=_masks(ref_masks), **kw)
    npos = 1 if npl else g[case + '_dirs'].shape[1]
    pre = ctx.debug_fetch('pre', (npos, lb.size, 40, 40))
    ctx.close()
    gpre = g[case + '_pre'].reshape(npos, lb.size, 40, 40)
    for d in range(npos):
        assert rel_err(pre[d], gpre[d]) < TOL[prec]['stamp'], (d, rel_err(pre[d], gpre[d]))
    check_final_stamps_and_fits(g, case, prec, ps, r, npos)


def check_final_stamps_and_fits(g, case, prec, ps, r, npos):
    """The final stamps and the fits of a reconstruct_profile result `r` of the golden case against the reference's,
    per direction.  Returns the worst relative error of a stamp."""
    from muse_psfr_amd import FIT_ILL_CONDITIONED
    nl = g[case + '_lbda'].size
    gfin = g[case + '_fin'].reshape(npos, nl, 40, 40)
    gfit = g[case + '_fit'].reshape(npos, nl, 5)
    fin, fit = r['psf'].reshape(npos, nl, 40, 40), r['fit'].reshape(npos, nl, -1)
    worst = 0.0
    for d in range(npos):
        worst = max(worst, rel_err(fin[d], gfin[d]))
        assert rel_err(fin[d], gfin[d]) < TOL[prec]['stamp'], (d, rel_err(fin[d], gfin[d]))
        # (a fit flagged ill-conditioned is held on peak and centre only, as in tests/test_gpu_field.py)
        assert np.abs(fit[d][:, 1:3] - gfit[d][:, 1:3]).max() < 1e-3
        assert np.all(np.abs(fit[d][:, 0] / gfit[d][:, 0] - 1) < 1e-3)
        well = (fit[d][:, 14].astype(int) & FIT_ILL_CONDITIONED) == 0
        assert well.any()
        assert np.abs(fit[d][well, 5] * ps - gfit[d][well, 3]).max() < TOL[prec]['fit']
        assert np.abs(fit[d][well, 4] - gfit[d][well, 4]).max() < TOL[prec]['fit']
    return worst


def test_simul_psd_wfm_profile_keyword(api, golden, ref_masks):
    g = golden('g9_profile')
    psd = api.simul_psd_wfm(g['a_cn2'], g['a_h'], float(g['a_seeing']), float(g['a_L0']), dim=512, verbose=False,
                            precision='f64', cutoff_masks=_masks(ref_masks), wind_speed=g['a_ws'],
                            wind_dir=g['a_wd'])
    assert rel_err(psd[:, 216:296, 216:296], g['a_zone']) <= 1e-12


# ---- 2. the reference's two layers are the legacy call, bit for bit
def _legacy_profile(gl, ws=12.0):
    return dict(cn2=np.stack([gl, 1.0 - gl], axis=1), h=(100.0, 10000.0), wind_speed=(ws, ws), wind_dir=REF_DIR)


@pytest.mark.parametrize('dim', [256, 512, 1280])
@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_two_layer_profile_is_the_legacy_call(api, dim, prec):
    see, gl, l0, three = ROWS
    ctx = api.Context(dim=dim, pixscale=api.grid_pixscale(dim), precision=prec)
    p = _legacy_profile(gl)
    for l0s in ((l0, np.array([25.0, 5.0, 18.0])) if dim == 512 else (l0,)):     # (L0 = 5 m: the full-size stage A)
        for npl in (1, 3):
            ref = ctx.reconstruct(LB, see, gl, l0s, three, H, wind_speed=12.0, npsflin=npl)
            r = ctx.reconstruct_profile(LB, see, gl, l0s, three_lgs=three, npsflin=npl, **p)
            _same_all(r, ref)
        ref = ctx.reconstruct_field(LB, see, gl, l0s, three, H, FIELD5, wind_speed=12.0)
        r = ctx.reconstruct_profile(LB, see, gl, l0s, three_lgs=three, positions=FIELD5, **p)
        _same_all(r, ref)
    ctx.close()


# ---- 3. invariances
A3 = dict(h=[0.0, 1000.0, 10000.0], wind_speed=[8.0, 15.0, 30.0], wind_dir=[0.3, -1.0, 2.0])


def test_zero_weight_layer_changes_no_bit(api):
    see, gl, l0, three = ROWS
    ctx = api.Context(dim=512, pixscale=api.grid_pixscale(512), precision='mixed')
    cn2 = np.array([[0.6, 0.25, 0.15], [0.3, 0.3, 0.4], [0.8, 0.1, 0.1]])
    ref = ctx.reconstruct_profile(LB, see, gl, l0, cn2, three_lgs=three, npsflin=3, **A3)
    for at, hz in ((0, 20000.0), (1, 500.0), (3, 0.0)):
        p = {k: np.insert(np.asarray(v, float), at, 7.0 if k != 'h' else hz) for k, v in A3.items()}
        r = ctx.reconstruct_profile(LB, see, gl, l0, np.insert(cn2, at, 0.0, axis=1), three_lgs=three, npsflin=3,
                                    **p)
        _same_all(r, ref)
    ctx.close()


def test_split_layer_moves_stamps_below_1e12(api):
    see, gl, l0, three = ROWS
    ctx = api.Context(dim=512, pixscale=api.grid_pixscale(512), precision='f64')
    cn2 = np.array([0.6, 0.25, 0.15])
    ref = ctx.reconstruct_profile(LB, see, gl, l0, cn2, three_lgs=three, **A3)
    p = {k: np.insert(np.asarray(v, float), 2, v[1]) for k, v in A3.items()}
    r = ctx.reconstruct_profile(LB, see, gl, l0, np.array([0.6, 0.125, 0.125, 0.15]), three_lgs=three, **p)
    assert rel_err(r['psf'], ref['psf']) <= 1e-12
    ctx.close()


def test_field_spread_grows_with_high_turbulence(api):
    pos = api.direction_perf(3).T
    ctx = api.Context(dim=512, pixscale=api.grid_pixscale(512), precision='f64')
    lb = np.array([500.0, 700.0, 900.0])
    ground = ctx.reconstruct_profile(lb, [0.8], [1.0], [25.0], [1.0], [0.0], [10.0], [0.5], positions=pos)
    high = ctx.reconstruct_profile(lb, [0.8], [0.5], [25.0], [0.5, 0.5], [0.0, 10000.0], [10.0, 10.0], [0.5, 0.5],
                                   positions=pos)
    fw_g, fw_h = ground['fit'][0, :, :, 5], high['fit'][0, :, :, 5]         # [position][wavelength]
    spread_g = (fw_g.max(axis=0) - fw_g.min(axis=0)) / fw_g.mean(axis=0)
    spread_h = (fw_h.max(axis=0) - fw_h.min(axis=0)) / fw_h.mean(axis=0)
    assert np.all(spread_g <= 1e-3), spread_g
    assert np.all(spread_h > spread_g), (spread_h, spread_g)
    ctx.close()


# ---- 4. forms
B8 = dict(h=[0.0, 300.0, 1000.0, 2500.0, 5000.0, 9000.0, 13000.0, 18000.0],
          wind_speed=[5.0, 8.0, 10.0, 14.0, 20.0, 30.0, 25.0, 12.0],
          wind_dir=[0.0, 0.4, -0.8, 1.2, 2.5, -2.0, 3.0, -0.3])


@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_batch_equals_single_rows_and_output_forms(api, prec):
    import torch
    see, gl, l0, three = ROWS
    rng = np.random.default_rng(9)
    cn2 = rng.random((3, 8))
    ctx = api.Context(dim=512, pixscale=api.grid_pixscale(512), precision=prec)
    for kw in (dict(npsflin=2), dict(positions=FIELD5)):
        ref = ctx.reconstruct_profile(LB, see, gl, l0, cn2, three_lgs=three, **kw, **B8)
        for t in range(3):
            r = ctx.reconstruct_profile(LB, see[t:t + 1], gl[t:t + 1], l0[t:t + 1], cn2[t:t + 1],
                                        three_lgs=three[t:t + 1], **kw, **B8)
            assert _same(r['psf'][0], ref['psf'][t]) and _same(r['fit'][0], ref['fit'][t])
        dev = torch.device('cuda:0')
        tp, ts, tf = (torch.empty(ref[k].shape, dtype=torch.float64, device=dev) for k in ('psf', 'psf_sum', 'fit'))
        torch.cuda.synchronize()
        ctx.reconstruct_profile_device(LB, see, gl, l0, cn2, B8['h'], B8['wind_speed'], B8['wind_dir'], three,
                                       kw.get('npsflin', 0), kw.get('positions'), None, tp.data_ptr(),
                                       ts.data_ptr(), tf.data_ptr())
        ctx.sync()
        _same_all(dict(psf=tp.cpu().numpy(), psf_sum=ts.cpu().numpy(), fit=tf.cpu().numpy()), ref)
        _same_all(ctx.reconstruct_profile_async(LB, see, gl, l0, cn2, three_lgs=three, **kw, **B8).wait(), ref)
    ctx.close()


# ---- 5. the table cache
def test_cache_across_profiles_and_legacy_calls(api):
    see, gl, l0, three = ROWS
    pa = dict(cn2=[0.6, 0.25, 0.15], **A3)
    pb = dict(cn2=np.random.default_rng(4).random(8), **B8)
    l0_5 = np.array([5.0, 5.0, 5.0])
    pc = dict(cn2=[1.0], h=[0.0], wind_speed=[10.0], wind_dir=[1.2])
    seq = [('A', pa, l0), ('B', pb, l0), ('A', pa, l0), ('legacy', None, l0), ('C', pc, l0), ('A', pa, l0_5)]
    ctx = api.Context(dim=512, pixscale=api.grid_pixscale(512), precision='mixed')

    def run(c, p, l0s):
        if p is None:
            return c.reconstruct(LB, see, gl, l0s, three, H, npsflin=3)
        return c.reconstruct_profile(LB, see, gl, l0s, three_lgs=three, npsflin=3, **p)
    for name, p, l0s in seq:
        got = run(ctx, p, l0s)
        fresh = api.Context(dim=512, pixscale=api.grid_pixscale(512), precision='mixed')
        _same_all(got, run(fresh, p, l0s))
        fresh.close()
        # (debug_fetch refuses a shape whose size is not what the library holds: [2][ndir][max(nlayer, 2) + 1][80][80]
        # after a profile call, [2][ndir][3][80][80] after a legacy one)
        ntab = 2 if p is None else max(len(p['h']), 2)
        tabs = ctx.debug_fetch('ao_tables', (2, 9, ntab + 1, 80, 80))
        assert np.all(np.isfinite(tabs)) and np.any(tabs[:, :, :ntab] != 0) and np.any(tabs[:, :, ntab] != 0)
        if p is not None and len(p['h']) == 1:       # a single layer: its table, a zero table, the noise
            assert np.all(tabs[:, :, 1] == 0) and np.any(tabs[:, :, 0] != 0)
    ctx.close()
