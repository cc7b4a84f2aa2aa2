"""GPU: Cn2-profile calls (mpsfr_reconstruct_profile, mpsfr_simul_psd_profile) against the fp64 oracle on every form of
stage A.  The cases, and the oracle of each, are those of tests/profile_cases.py; tests/test_profile_oracle_host.py holds
that oracle to the reference's goldens and to long double, and shows that the cases tell a wrong mixing from a right one.

1. The case matrix, both precisions: the form of stage A the case names did run (launch counts); `ao_tables`, `dphi0`,
   the stamps before and after the convolutions and, from 512^2 on, the fits against the oracle.  Every bound is one
   the legacy atmosphere is already held to: tables 1e-12 (test_gpu_parity.py::test_every_stage_against_the_oracle),
   dphi0 1e-12 / 2e-7 of its maximum on the telescope's support and exactly 0 or within the bound outside
   (test_gpu_series_hermitian.py::_check_d0), stamps 1e-9 / 2e-5 of their maximum, fwhm [arcsec] and beta 1e-6 / 1e-4
   with no fit flagged ill-conditioned.
2. mpsfr_simul_psd_profile on 128^2, 256^2, 1024^2 and 1280^2, profiles P8 and PX, both geometries, npsflin = 3 and 25
   positions: the whole plane within 1e-12 (test_gpu_profile.py::test_psd_matches_reference_profiles).
3. Chunks and lanes bit for bit on the full-size and on the series form; single rows against the batch on both, rows
   with zeros in layers the others use included (this found the mixing sum depending on them: ao_mix_sum, psd_model.h).
4. A layer of weight 0 in every row is dropped, on a full-size-form grid.
5. The order of the layers changes nothing beyond the bounds of the one oracle.

Worst error / bound per class goes to record_margin('profile_oracle', ...) (profiles/profile_oracle_margins.json).
"""
import numpy as np
import pytest

import profile_cases as PC
import psfr_oracle as O
from conftest import record_margin, rel_err

pytestmark = pytest.mark.gpu

EPS_TAB = 1e-12
EPS_D = {'f64': 1e-12, 'mixed': 2e-7}
TOL_STAMP = {'f64': 1e-9, 'mixed': 2e-5}
TOL_FIT = {'f64': 1e-6, 'mixed': 1e-4}
EPS_PSD = 1e-12
FULL, SERIES = ('psd_rowfft', 'colfft_dphi'), ('patch', 'dphi_series')


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _context(api, dim, prec, **opts):
    ctx = api.Context(dim=dim, pixscale=api.grid_pixscale(dim), precision=prec)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def _call(ctx, inp, **over):
    a = dict(inp, **over)
    return ctx.reconstruct_profile(a['lbda'], a['seeing'], a['gl'], a['l0'], a['cn2'], a['h'], a['wind_speed'],
                                   a['wind_dir'], three_lgs=a['three'], **a['kw'])


def _form_that_ran(ctx):
    prof = ctx.profile()
    full, series = [prof[k][1] for k in FULL], [prof[k][1] for k in SERIES]
    if all(n > 0 for n in full) and not any(series):
        return 'full'
    if all(n > 0 for n in series) and not any(full):
        return 'series'
    return 'mixed up: %r' % {k: prof[k][1] for k in FULL + SERIES}


def _oracle_table_stack(T, noise):
    """The oracle's tables in the library's layout [dir][ntab + 1][80][80] (test_every_stage_against_the_oracle)."""
    T = T.copy()
    T[..., 0, 0] = 0                                      # psfrec.py:490
    tabs = [np.swapaxes(t, -1, -2) for t in T]
    if len(tabs) == 1:
        tabs.append(np.zeros_like(tabs[0]))               # a single layer: a zero second table
    return np.stack(tabs + [np.swapaxes(noise, -1, -2)], axis=1)


def _check_tables(tab, otabs, tag):
    worst = 0.0
    for g in (0, 1):
        ot = _oracle_table_stack(*otabs[g])
        assert tab[g].shape == ot.shape
        for t in range(ot.shape[1]):                      # every layer table and the noise, each against its own maximum
            if not np.any(ot[:, t]):
                assert not np.any(tab[g][:, t])
                continue
            worst = max(worst, rel_err(tab[g][:, t], ot[:, t]))
    print('%s ao_tables vs oracle: %.3e (bound %.1e)' % (tag, worst, EPS_TAB))
    record_margin('profile_oracle', tables=worst / EPS_TAB)
    assert worst < EPS_TAB
    return worst


def _check_d0(d0, od0, tel, prec, tag, key='dphi0'):
    """The rule of tests/test_gpu_series_hermitian.py::_check_d0, per row."""
    eps, worst = EPS_D[prec], 0.0
    for k in range(d0.shape[0]):
        inside = np.broadcast_to(tel > 0, d0[k].shape)
        scale = np.abs(od0[k]).max()
        worst = max(worst, np.abs(d0[k] - od0[k])[inside].max() / scale)
        out = d0[k][~inside]        # whole pieces of a line outside the support are skipped, the others computed
        assert np.all((out == 0) | (np.abs(out - od0[k][~inside]) / scale < eps))
    print('%s dphi0 vs oracle: %.3e (bound %.1e)' % (tag, worst, eps))
    record_margin('profile_oracle', **{'%s_%s' % (key, prec): worst / eps})
    assert worst < eps


def _check_stamps(got, want, prec, tag, key):
    """Groups of nl stamps (a row, or a row at a position), each against its own maximum."""
    got, want = np.asarray(got, float), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    g, w = got.reshape(-1, *want.shape[-3:]), want.reshape(-1, *want.shape[-3:])
    worst = max(rel_err(a, b) for a, b in zip(g, w))
    print('%s %s vs oracle: %.3e (bound %.1e)' % (tag, key, worst, TOL_STAMP[prec]))
    record_margin('profile_oracle', **{'%s_%s' % (key, prec): worst / TOL_STAMP[prec]})
    assert worst < TOL_STAMP[prec]


def _check_fits(fit, ofit, ps, prec, tag):
    fit = np.asarray(fit)
    assert fit.shape[:-1] == ofit.shape[:-1]
    assert np.all(fit[..., 14] == 0)                    # no fit is ill-conditioned: all of them are compared
    e_fwhm = np.abs(fit[..., 5] * ps - ofit[..., 3]).max()
    e_beta = np.abs(fit[..., 4] - ofit[..., 4]).max()
    print('%s fit vs oracle: fwhm %.3e beta %.3e (bound %.1e)' % (tag, e_fwhm, e_beta, TOL_FIT[prec]))
    record_margin('profile_oracle', **{'fwhm_%s' % prec: e_fwhm / TOL_FIT[prec], 'beta_%s' % prec: e_beta / TOL_FIT[prec]})
    assert e_fwhm < TOL_FIT[prec] and e_beta < TOL_FIT[prec]


def _check_outputs(r, pre, o, dim, ps, prec, tag):
    _check_stamps(pre.reshape(o['pre'].shape), o['pre'], prec, tag, 'pre')
    _check_stamps(r['psf'], o['fin'], prec, tag, 'stamp')
    if dim >= 512:                          # (smaller grids: as in test_gpu_parity.py, the fits are not compared)
        _check_fits(r['fit'], o['fit'], ps, prec, tag)


# ---- 1. the case matrix
@pytest.mark.parametrize('prec', ['f64', 'mixed'])
@pytest.mark.parametrize('cid', list(PC.CASES))
def test_profile_case_against_the_oracle(api, cid, prec):
    c = PC.CASES[cid]
    dim, inp = c['dim'], PC.case_inputs(cid)
    nrow, ndir, nl = len(inp['seeing']), inp['dirs'].shape[1], inp['lbda'].size
    ntab = max(len(inp['h']), 2)
    gpp = ndir if 'positions' in inp['kw'] else 1           # stamps per row and wavelength
    # (one lane, one chunk: debug_fetch hands out the whole call)
    ctx = _context(api, dim, prec, streams=1, stage_a=c['stage_a'], profile=1)
    ctx.profile_reset()
    r = _call(ctx, inp)
    form = _form_that_ran(ctx)
    tab = ctx.debug_fetch('ao_tables', (2, ndir, ntab + 1, 80, 80))
    tel = ctx.debug_fetch('tel', (dim // 2 + 1, dim))
    d0 = ctx.debug_fetch('dphi0', (nrow, ndir, dim // 2 + 1, dim))
    pre = ctx.debug_fetch('pre', (nrow, gpp, nl, 40, 40))
    ctx.close()
    assert form == c['form'], (cid, form)
    o = PC.oracle_case(cid)
    tag = '%s %s' % (cid, prec)
    _check_tables(tab, o['tabs'], tag)
    _check_d0(d0, o['d0'], tel, prec, tag)
    _check_outputs(r, pre, o, dim, api.grid_pixscale(dim), prec, tag)
    np.testing.assert_allclose(r['psf_sum'], np.asarray(r['psf']).sum(axis=0), rtol=1e-13)


# ---- 2. the PSD of a profile on the other grids
PSD_SETTINGS = {128: dict(npsflin=3), 256: dict(positions=PC.POS25), 1024: dict(positions=PC.POS2), 1280: dict(npsflin=1)}
PSD_ROW = dict(seeing=0.8, l0=16.0)
_psd_cache = {}


def _oracle_psd(dim, pname, three):
    key = (dim, pname, three)
    if key not in _psd_cache:
        prof, kw = PC.PROFILES[pname], PSD_SETTINGS[dim]
        dirs = np.asarray(kw['positions']).T if 'positions' in kw else O.eval_directions(kw['npsflin'])
        tabs = O.ao_tables(prof['h'], three, 1, exact_masks=True, wind_speed=prof['wind_speed'],
                           wind_dir=prof['wind_dir'], directions=dirs)
        _psd_cache[key] = O.residual_psd(PC.WEIGHTS[pname][0], prof['h'], PSD_ROW['seeing'], PSD_ROW['l0'], 1, dim,
                                         three, tables=tabs)
    return _psd_cache[key]


@pytest.mark.parametrize('prec', ['f64', 'mixed'])
@pytest.mark.parametrize('pname', ['P8', 'PX'])
@pytest.mark.parametrize('dim', list(PSD_SETTINGS))
def test_simul_psd_profile_against_the_oracle(api, dim, pname, prec):
    prof = PC.PROFILES[pname]
    ctx = _context(api, dim, prec)
    sl = slice(dim // 2 - 40, dim // 2 + 40)
    outside = np.ones((dim, dim), bool)
    outside[sl, sl] = False
    worst = 0.0
    for three in (False, True):
        psd = ctx.simul_psd_profile(PSD_ROW['seeing'], PSD_ROW['l0'], PC.WEIGHTS[pname][0], prof['h'],
                                    prof['wind_speed'], prof['wind_dir'], three_lgs=three, **PSD_SETTINGS[dim])
        want = _oracle_psd(dim, pname, three)
        assert psd.shape == want.shape
        for d in range(psd.shape[0]):                   # the corrected zone and the fitting term, each on its own scale
            worst = max(worst, rel_err(psd[d][sl, sl], want[d][sl, sl]), rel_err(psd[d][outside], want[d][outside]))
    ctx.close()
    print('%d %s %s psd vs oracle: %.3e (bound %.1e)' % (dim, pname, prec, worst, EPS_PSD))
    record_margin('profile_oracle', psd=worst / EPS_PSD)
    assert worst <= EPS_PSD


# ---- 3. chunks and lanes
def _five_rows(cid):
    """Five rows on a case's setting: its three, then two more with other weights, seeing, L0 and geometry."""
    inp = PC.case_inputs(cid)
    w = inp['cn2']
    return dict(inp, seeing=np.append(inp['seeing'], [0.7, 1.1]), gl=np.append(inp['gl'], [0.6, 0.85]),
                l0=np.append(inp['l0'], [12.0, 28.0]), three=np.append(inp['three'], [1, 0]).astype(np.uint8),
                cn2=np.concatenate([w, np.roll(w[:1], 3, axis=1), w[1:2, ::-1]]))


@pytest.mark.parametrize('prec', ['f64', 'mixed'])
@pytest.mark.parametrize('cid', ['F2', 'S3'])
def test_chunks_and_lanes_change_no_bit(api, cid, prec):
    c = PC.CASES[cid]
    inp = _five_rows(cid)
    ctx = _context(api, c['dim'], prec, streams=1, profile=1)
    ctx.profile_reset()
    ref = _call(ctx, inp)
    assert _form_that_ran(ctx) == c['form']
    # Each row alone is its row of the batch, on the full-size form too -- also the rows that hold zeros in layers the
    # others use: alone, such a row is a call without those layers (the host drops them), and the mixing sum must not
    # depend on that (ao_mix_sum, psd_model.h; it did, in the last bit of the PSD, before this test existed).
    for t in range(5):
        one = _call(ctx, inp, **{k: inp[k][t:t + 1] for k in ('seeing', 'gl', 'l0', 'three', 'cn2')})
        assert np.array_equal(one['psf'][0], ref['psf'][t]) and np.array_equal(one['fit'][0], ref['fit'][t]), t
    ctx.close()
    for streams in (1, 2):
        ctx = _context(api, c['dim'], prec, streams=streams, chunk_tasks=2, profile=1)
        ctx.profile_reset()
        r = _call(ctx, inp)
        assert _form_that_ran(ctx) == c['form']
        ctx.close()
        assert np.array_equal(r['psf'], ref['psf']) and np.array_equal(r['fit'], ref['fit']), streams
        np.testing.assert_allclose(r['psf_sum'], ref['psf_sum'], rtol=1e-13)   # (per-lane partial sums, test_gpu_band.py)


# ---- 4. dropped layers
@pytest.mark.parametrize('prec', ['f64', 'mixed'])
def test_a_layer_of_weight_zero_is_dropped_on_the_full_size_form(api, prec):
    inp = PC.case_inputs('F2')
    cn2 = inp['cn2'].copy()
    cn2[:, 1] = 0.0
    cn2[2, 0] = 0.3                                     # (row 2 held all its weight in the middle layer)
    keep = [0, 2]
    ctx = _context(api, 256, prec, streams=1, profile=1)
    ctx.profile_reset()
    with3 = _call(ctx, inp, cn2=cn2)
    assert _form_that_ran(ctx) == 'full'
    tab3 = ctx.debug_fetch('ao_tables', (2, 1, 3, 80, 80))             # the shape of two layers (refused otherwise)
    d3 = ctx.debug_fetch('dphi0', (3, 1, 129, 256))
    with2 = _call(ctx, inp, cn2=cn2[:, keep], **{k: np.asarray(inp[k])[keep] for k in ('h', 'wind_speed', 'wind_dir')})
    tab2 = ctx.debug_fetch('ao_tables', (2, 1, 3, 80, 80))
    d2 = ctx.debug_fetch('dphi0', (3, 1, 129, 256))
    ctx.close()
    assert np.array_equal(tab3, tab2) and np.array_equal(d3, d2)
    for k in ('psf', 'psf_sum', 'fit'):
        assert np.array_equal(with3[k], with2[k]), k


# ---- 5. layer order
@pytest.mark.parametrize('prec', ['f64', 'mixed'])
@pytest.mark.parametrize('form', ['full', 'series'])
def test_layer_order_stays_within_the_bounds_of_one_oracle(api, form, prec):
    """P5 lowest layer first and last, 512^2, three rows (one at L0 = 5 m for the full-size form)."""
    dim, ps = 512, api.grid_pixscale(512)
    prof = PC.P5
    inp = dict(lbda=PC.lbda(dim), seeing=PC.SEE, gl=PC.GL, l0=np.array([16.0, 5.0, 24.0]) if form == 'full' else PC.L0,
               three=PC.THREE, cn2=PC.W5, dirs=O.eval_directions(1), kw=dict(npsflin=1), **prof)
    key = ('order', form)
    if key not in _psd_cache:
        tabs = PC.oracle_tables(prof, inp['dirs'])
        _psd_cache[key] = PC.oracle_rows(inp, dim, tabs)
    o = _psd_cache[key]
    assert o['kappa'].max() < PC.WELL_POSED_LIMIT[dim]
    rev = dict(inp, cn2=PC.W5[:, ::-1], **{k: prof[k][::-1] for k in ('h', 'wind_speed', 'wind_dir')})
    for name, a in (('lowest first', inp), ('lowest last', rev)):
        ctx = _context(api, dim, prec, streams=1, profile=1)
        ctx.profile_reset()
        r = _call(ctx, a)
        assert _form_that_ran(ctx) == form
        tel = ctx.debug_fetch('tel', (dim // 2 + 1, dim))
        d0 = ctx.debug_fetch('dphi0', (3, 1, dim // 2 + 1, dim))
        pre = ctx.debug_fetch('pre', (3, 1, 2, 40, 40))
        ctx.close()
        tag = 'P5 %s %s %s' % (name, form, prec)
        _check_d0(d0, o['d0'], tel, prec, tag, key='order_dphi0')
        _check_outputs(r, pre, o, dim, ps, prec, tag)
