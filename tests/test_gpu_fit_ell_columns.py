"""GPU: every column and every status of the elliptical Moffat fit (mpsfr_fit_stamps_elliptical, k_fit_ell in both
precisions) against fp64 (tests/moffat_ell_ref.py: SciPy's Levenberg-Marquardt, the header's recipe for the derived
columns with numerical gradients).

(a) perturbed stamps, whose minimum is not the truth: parameters, chi2, flux and all error columns;
(b) exact stamps at the edges of the domain: |e| up to and beyond the bound, b/a = 1, n close to 1;
(c) the ill-conditioned bit against the number it is defined by;
(d) degenerate stamps between good ones;
(e) amplitudes 2^-60 ... 2^60;
(f) the start values, through the iteration count.

Parameter tolerances are those of tests/test_gpu_fit_ell.py: 1e-8 (f64) and 1e-4 (mixed), relative for peak, FWHMs
and n, in px for the centre, (1 - b/a) |d rot| in radians for the orientation.  Each test fits all its stamps in one
call and records its worst values with record_margin('fit_ell_columns', ...).
"""
import numpy as np
import pytest

import moffat_ell_ref as M
from conftest import record_margin

pytestmark = pytest.mark.gpu

TOL = {'f64': 1e-8, 'mixed': 1e-4}
STAMP_TOL = {'f64': 1e-9, 'mixed': 2e-5}         # max |model - stamp| / peak (tests/test_gpu_fit_circular.py)
COLUMN_TOL = 1e-3                                # chi2, flux and the error columns, relative
MAXIT = 200                                      # MPSFR_FIT_MAXIT
MAX_E = 0.94                                     # include/mpsfr.h: a row with status & 3 == 0 has |e| <= 0.94
PRECS = ['mixed', 'f64']
ERR_COLUMNS = ('chi2', 'err_peak', 'err_p0', 'err_q0', 'err_fwhm_major', 'err_fwhm_minor', 'err_rot', 'err_n', 'flux',
               'err_flux')


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


def _lm(peak, p0, q0, fw, ba, rot, n):
    e1, e2 = M.e_from_ratio(ba, rot)
    return np.array([peak, p0, q0, fw, e1, e2, 1.0 / n])


def _param_errors(row, v, prec):
    """error / tolerance of a fit row against the LM variables v: peak, fwhm_major, fwhm_minor, n relative, the
    centre in px, rot as (1 - b/a) |d rot| in radians."""
    want, got, t = M.derived(v), M.gpu_derived(row), TOL[prec]
    out = {k: abs(got[k] - want[k]) / abs(want[k]) / t for k in ('peak', 'fwhm_major', 'fwhm_minor', 'n')}
    out['centre'] = max(abs(got['p0'] - want['p0']), abs(got['q0'] - want['q0'])) / t
    out['rot'] = (1.0 - want['ba']) * float(M.rot_diff(got['rot'], want['rot'])) / t
    return out


def _worst(dicts):
    out = {}
    for d in dicts:
        for k, x in d.items():
            out[k] = max(out.get(k, 0.0), float(x) if np.isfinite(x) else np.inf)
    return out


def _model_residual(row, stamp):
    """max |model of the row - stamp| / max |stamp| in fp64 (inf where the row has no model)."""
    with np.errstate(all='ignore'):
        m = M.model(M.v_from_row(row)).reshape(M.NS, M.NS)
        r = np.abs(m - stamp).max() / np.abs(stamp).max()
    return float(r) if np.isfinite(r) else np.inf


def _fit_on_device(ctx, stamps):
    """The device form of the call.  The entry point accepts any data; the host wrapper refuses non-finite stamps."""
    import torch
    dev = torch.device('cuda:0')
    ts = torch.from_numpy(np.ascontiguousarray(stamps, dtype=np.float64)).to(dev)
    tf = torch.full((len(stamps), 24), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_stamps_elliptical_device(len(stamps), ts.data_ptr(), tf.data_ptr())
    ctx.sync()
    return tf.cpu().numpy()


def _status(fit):
    return fit[:, 18].astype(int)


# ---- (a) perturbed stamps: every column
@pytest.mark.parametrize('prec', PRECS)
def test_perturbed_stamps_every_column(ctx, prec):
    """16 elliptical Moffats plus a fixed perturbation of 1e-3 of the peak (M.perturbed_cases).  SciPy reaches the
    same minimum from three starts; kappa < 100.  Parameters to TOL; chi2, flux and the error columns to 1e-3 relative
    against fit_full, the bound of the circular fit's error columns (the covariance is formed the same way, from the
    last normal matrix).  Beside each column's error against the reference's minimum the test prints the error against
    the header's recipe evaluated in fp64 at the row's own point with the row's own chi2: the first holds the recipe and
    the point, the second the recipe alone."""
    refs = M.perturbed_references()
    assert len(refs) == 16
    for name, _, full, spread in refs:
        assert spread <= 1e-8, (name, spread)
        assert full['kappa'] < 100, (name, full['kappa'])
    fit = ctx.fit_stamps_elliptical(np.array([st for _, st, _, _ in refs]))
    assert fit.shape == (16, 24)
    par = _worst(_param_errors(row, full['v'], prec) for row, (_, _, full, _) in zip(fit, refs))
    cols, own = {}, {}
    for row, (name, _, full, _) in zip(fit, refs):
        at_row = M.columns_at(M.v_from_row(row), row[9])
        for c in ERR_COLUMNS:
            cols[c] = max(cols.get(c, 0.0), abs(row[M.COLUMN[c]] / full[c] - 1.0))
            if c in at_row:
                own[c] = max(own.get(c, 0.0), abs(row[M.COLUMN[c]] / at_row[c] - 1.0))
    print('perturbed %s: parameters, error / tolerance %s' % (prec, par))
    print('perturbed %s: columns, relative to fit_full %s' % (prec, cols))
    print('perturbed %s: columns, relative to the recipe at the row\'s own point %s' % (prec, own))
    print('perturbed %s: iterations %s' % (prec, fit[:, 10].astype(int)))
    record_margin('fit_ell_columns', **{'perturbed_%s_%s' % (prec, k): x for k, x in par.items()})
    record_margin('fit_ell_columns', **{'perturbed_%s_rel_%s' % (prec, k): x for k, x in cols.items()})
    record_margin('fit_ell_columns', **{'perturbed_%s_own_point_rel_%s' % (prec, k): x for k, x in own.items()})
    assert np.all(fit[:, 18] == 0), fit[:, 18]
    assert np.all(fit[:, 10] < MAXIT), fit[:, 10]
    assert np.all(fit[:, 21:] == 0.0)
    assert max(par.values()) <= 1.0, par
    assert max(cols.values()) < COLUMN_TOL, cols


# ---- (b) exact stamps at the edges of the domain
@pytest.mark.parametrize('prec', PRECS)
def test_elongation_up_to_and_beyond_the_bound(ctx, prec):
    """FWHM 6, n 2.5, centre (19.7, 20.4), rot 0, 45, 100 degrees.  b/a = 0.3 and 0.2 (e = 0.835, 0.923) lie inside
    the domain |e| <= 0.95 and come back to TOL with status 0.  b/a = 0.15 and 0.1 (e = 0.956, 0.980) lie beyond it:
    the row must not claim a minimum it does not have -- status & 3 != 0 or the right answer.  The header's rule: a
    row with status & 3 == 0 has |e| <= 0.94; where the iteration ends beyond that, against the bound, the status is
    1."""
    rots = (0.0, 45.0, 100.0)
    inside = [(1.0, 19.7, 20.4, 6.0, ba, rot, 2.5) for ba in (0.3, 0.2) for rot in rots]
    beyond = [(1.0, 19.7, 20.4, 6.0, ba, rot, 2.5) for ba in (0.15, 0.1) for rot in rots]
    assert all(np.hypot(*M.e_from_ratio(p[4], p[5])) < 0.93 for p in inside)
    assert all(np.hypot(*M.e_from_ratio(p[4], p[5])) > 0.95 for p in beyond)
    fit = ctx.fit_stamps_elliptical(np.array([M.stamp(*p) for p in inside + beyond]))
    st = _status(fit)
    e_fit = [float(np.hypot(*M.v_from_row(r)[4:6])) for r in fit]
    print('elongation %s: status %s iterations %s fitted |e| %s' % (prec, st, fit[:, 10].astype(int), e_fit))
    par = _worst(_param_errors(row, _lm(*p), prec) for row, p in zip(fit, inside))
    print('elongation %s: inside the bound, error / tolerance %s' % (prec, par))
    record_margin('fit_ell_columns', **{'elongated_%s_%s' % (prec, k): x for k, x in par.items()})
    assert np.all(fit[:6, 18] == 0), fit[:6, 18]
    assert max(par.values()) <= 1.0, par
    bad = []
    for row, p, s, e in zip(fit[6:], beyond, st[6:], e_fit[6:]):
        w = _param_errors(row, _lm(*p), prec)
        if (s & 3) == 0 and not max(w.values()) <= 1.0:
            bad.append((p, 'status 0 on a wrong answer', row))
        if (s & 3) == 0 and not e <= MAX_E:
            bad.append((p, 'status 0 beyond |e| = 0.94', e))
    assert not bad, bad
    assert np.all(np.isfinite(fit[(st & 3) == 0]))


def _round_noisy():
    rng = np.random.default_rng(77)
    noise = rng.standard_normal((M.NS, M.NS))
    return M.stamp(1.0, 19.7, 20.4, 6.0, 1.0, 0.0, 2.5) + noise * (1e-3 / np.abs(noise).max())


@pytest.mark.parametrize('prec', PRECS)
def test_round_stamp_has_a_finite_rot_and_a_large_err_rot(ctx, prec):
    """b/a = 1 exactly (e = 0): FWHM 6, n 2.5, centre (19.7, 20.4).  rot is finite in [0, 180), err_rot finite in
    [0, 180], b/a within 1e-6 (f64) / 1e-4 (mixed) of 1, everything else at TOL.

    How large err_rot must be is a statement about noise, so it is asserted on the same round stamp plus the seeded
    noise field of the perturbed cases (1e-3 of the peak).  There (e1, e2) of the fit are two estimates of zero with
    the standard deviation s the covariance gives, so |e| / s is Rayleigh distributed: |e| <= 5 s with probability
    1 - 4e-6, and err_rot = s / (2 |e|) rad >= 0.1 rad = 5.7 degrees (or the cap of 180).  On the exact stamp chi2 is
    rounding noise (f64) or the remainder of the polish (mixed) and |e| / s is no statistic: printed, not asserted."""
    exact, noisy = M.stamp(1.0, 19.7, 20.4, 6.0, 1.0, 0.0, 2.5), _round_noisy()
    fit = ctx.fit_stamps_elliptical(np.array([exact, noisy]))
    print('round %s: exact rot %.6g err_rot %.6g 1 - b/a %.3g chi2 %.3g; noisy rot %.6g err_rot %.6g 1 - b/a %.3g' % (
        prec, fit[0, 6], fit[0, 16], 1 - fit[0, 8] / fit[0, 7], fit[0, 9], fit[1, 6], fit[1, 16],
        1 - fit[1, 8] / fit[1, 7]))
    assert np.all(fit[:, 18] == 0) and np.all(np.isfinite(fit))
    for row in fit:
        assert 0.0 <= row[6] < 180.0 and 0.0 <= row[16] <= 180.0, row
    w = _param_errors(fit[0], _lm(1.0, 19.7, 20.4, 6.0, 1.0, 0.0, 2.5), prec)
    w['1-b/a'] = (1.0 - fit[0, 8] / fit[0, 7]) / (1e-6 if prec == 'f64' else 1e-4)
    record_margin('fit_ell_columns', **{'round_%s_%s' % (prec, k): x for k, x in w.items()})
    assert max(w.values()) <= 1.0, w
    full = M.fit_full(noisy, _lm(1.0, 19.7, 20.4, 6.0, 1.0, 0.0, 2.5))
    print('round %s: noisy stamp, fp64 reference rot %.6g err_rot %.6g 1 - b/a %.3g' % (
        prec, full['rot'], full['err_rot'], 1 - full['ba']))
    record_margin('fit_ell_columns', **{'round_noisy_%s_err_rot_deg' % prec: fit[1, 16]})
    assert full['err_rot'] >= np.rad2deg(0.1)
    assert fit[1, 16] >= np.rad2deg(0.1), fit[1, 16]
    own = M.columns_at(M.v_from_row(fit[1]), fit[1, 9])['err_rot']        # the recipe at the row's own (e1, e2)
    assert abs(fit[1, 16] / own - 1.0) < COLUMN_TOL, (fit[1, 16], own)


@pytest.mark.parametrize('prec', PRECS)
def test_flux_and_err_flux_where_n_minus_1_is_small(ctx, prec):
    """n = 1.05, 1.6, 8 at FWHM 5, b/a 0.7, rot 30, centre (19.7, 20.4), exact stamps.  Parameters to TOL.  flux =
    peak pi alpha_major alpha_minor / (n - 1) against the truth's: its relative error is at most that of the peak, of
    the two FWHMs, and of n times |d ln flux / d ln n| = n / (n - 1) + |d ln alpha^2 / d ln n|, the last below 1.5
    for n > 1 -- (4.5 + n / (n - 1)) TOL, 25.5 TOL at n = 1.05.  err_flux of an exact stamp is rounding noise times
    the recipe; it is held to the header's recipe evaluated in fp64 at the row's own point with the row's own chi2.
    The matrix of the mixed mode is the float one of the last LM pass, whose point lies within the 1e-3 of the float
    convergence test of the final one, and the flux gradient's eta term n^2 / (n - 1) changes by 1 + n / (n - 1)
    times that: the bound is 1e-3 (1 + n / (n - 1)), 2.2e-2 at n = 1.05 and 3.7e-3 at n = 1.6."""
    ns = (1.05, 1.6, 8.0)
    pars = [(1.0, 19.7, 20.4, 5.0, 0.7, 30.0, n) for n in ns]
    assert max(M.kappa(_lm(*p)) for p in pars) < 100
    fit = ctx.fit_stamps_elliptical(np.array([M.stamp(*p) for p in pars]))
    assert np.all(fit[:, 18] == 0) and np.all(np.isfinite(fit)) and np.all(fit[:, 10] < MAXIT), fit[:, [10, 18]]
    worst = {}
    for row, p in zip(fit, pars):
        n = p[6]
        w = _param_errors(row, _lm(*p), prec)
        want = M.QUANTITIES['flux'](_lm(*p))
        w['flux'] = abs(row[19] / want - 1.0) / ((4.5 + n / (n - 1.0)) * TOL[prec])
        at_row = M.columns_at(M.v_from_row(row), row[9])
        if at_row['err_flux'] > 0.0 or row[20] > 0.0:
            w['err_flux'] = abs(row[20] / at_row['err_flux'] - 1.0) / (COLUMN_TOL * (1.0 + n / (n - 1.0)))
        assert row[20] >= 0.0 and row[19] > 0.0
        print('n near 1 %s: n = %g flux %.12g (truth %.12g) err_flux %.6g (recipe at the row %.6g) chi2 %.3g: '
              'error / bound %s' % (prec, n, row[19], want, row[20], at_row['err_flux'], row[9], w))
        for k, x in w.items():
            worst[k] = max(worst.get(k, 0.0), x)
    record_margin('fit_ell_columns', **{'n_near_1_%s_%s' % (prec, k): x for k, x in worst.items()})
    assert max(worst.values()) <= 1.0, worst


# ---- (c) the ill-conditioned bit against kappa
FLAGGED = ((2, 8), (3, 12), (5, 12), (8, 20), (12, 20), (20, 20))
CLEAR = ((2, 4), (3, 4), (5, 8), (8, 8), (12, 8), (20, 8), (5, 2.5), (3, 1.5))


@pytest.mark.parametrize('prec', PRECS)
def test_ill_conditioned_bit_against_kappa(ctx, prec):
    """The status bit MPSFR_FIT_ILL_CONDITIONED equals kappa >= 100, kappa from the 7-column fp64 Jacobian, on exact
    stamps away from the threshold: centre (19.5, 19.5), rot 30, b/a 1, 0.7, 0.5; flagged side kappa >= 130, clear
    side kappa <= 65.  Flagged rows converge and are held as the circular test holds them: peak to 1e-3, centre to 1e-3
    px, the fitted model reproduces the stamp to the stamp tolerance."""
    bas = (1.0, 0.7, 0.5)
    flagged = [(1.0, 19.5, 19.5, float(fw), ba, 30.0, float(n)) for ba in bas for fw, n in FLAGGED]
    clear = [(1.0, 19.5, 19.5, float(fw), ba, 30.0, float(n)) for ba in bas for fw, n in CLEAR]
    assert len(flagged) + len(clear) == 14 * 3
    kf, kc = [M.kappa(_lm(*p)) for p in flagged], [M.kappa(_lm(*p)) for p in clear]
    print('flag %s: kappa flagged %.4g .. %.4g, clear .. %.4g' % (prec, min(kf), max(kf), max(kc)))
    assert min(kf) >= 130 and max(kc) <= 65, (min(kf), max(kc))
    stamps = np.array([M.stamp(*p) for p in flagged + clear])
    fit = ctx.fit_stamps_elliptical(stamps)
    st, nf = _status(fit), len(flagged)
    print('flag %s: flagged side status %s, clear side status %s' % (prec, st[:nf], st[nf:]))
    dpk = max(abs(r[0] / p[0] - 1.0) for r, p in zip(fit, flagged))
    dce = max(max(abs(r[1] - p[1]), abs(r[2] - p[2])) for r, p in zip(fit, flagged))
    res = max(_model_residual(r, s) for r, s in zip(fit[:nf], stamps[:nf]))
    par = _worst(_param_errors(r, _lm(*p), prec) for r, p in zip(fit[nf:], clear))
    print('flag %s: flagged peak %.3e centre %.3e model residual %.3e; clear side error / tolerance %s' % (
        prec, dpk, dce, res, par))
    record_margin('fit_ell_columns', **{'flagged_%s_peak_rel' % prec: dpk, 'flagged_%s_centre_px' % prec: dce,
                                        'flagged_%s_model_residual' % prec: res})
    record_margin('fit_ell_columns', **{'flag_clear_%s_%s' % (prec, k): x for k, x in par.items()})
    assert np.all((st[:nf] & 4) == 4) and np.all((st[nf:] & 4) == 0), st
    assert np.all((st & 3) == 0), st
    assert np.all(np.isfinite(fit))
    assert dpk < 1e-3 and dce < 1e-3
    assert res < STAMP_TOL[prec], res
    assert max(par.values()) <= 1.0, par


# ---- (d) degenerate stamps between good ones
def degenerate_batch():
    good = [M.stamp(1.0, 19.7, 20.4, 5.0, 0.8, 30.0, 2.5), M.stamp(0.8, 18.2, 21.1, 8.0, 0.6, 75.0, 1.5),
            M.stamp(1.5, 20.9, 19.0, 3.0, 0.9, 140.0, 4.0)]
    hot_mid, hot_corner = np.zeros((40, 40)), np.zeros((40, 40))
    hot_mid[20, 20] = 1.0
    hot_corner[0, 39] = 1.0
    with_nan, with_inf, with_ninf = good[0].copy(), good[0].copy(), good[0].copy()
    with_nan[7, 11] = np.nan
    with_inf[30, 5] = np.inf
    with_ninf[30, 5] = -np.inf
    return [('good0', good[0]), ('zero', np.zeros((40, 40))), ('good1', good[1]), ('constant', np.ones((40, 40))),
            ('negative', -good[0] - 0.1), ('good2', good[2]), ('hot_middle', hot_mid), ('hot_corner', hot_corner),
            ('good0_again', good[0]), ('nan_pixel', with_nan), ('inf_pixel', with_inf), ('minus_inf_pixel', with_ninf),
            ('good1_again', good[1])]


@pytest.mark.parametrize('prec', PRECS)
def test_degenerate_stamps_between_good_ones(ctx, prec):
    """The batch of tests/test_gpu_fit_circular.py with elliptical good stamps and a -inf pixel added: all zero,
    constant 1, all negative, one hot pixel (middle, corner), one NaN, +inf, -inf pixel.  The good rows equal their
    single-stamp fits bit for bit with status 0; every other row has status & 3 != 0, or finite numbers only and a model
    that reproduces the stamp to the stamp tolerance; no row has a non-finite number beside status & 3 == 0.  The
    batch goes through the device form of the call, the single stamps through the host form."""
    rows = degenerate_batch()
    assert len(rows) == 13
    fit = _fit_on_device(ctx, np.array([s for _, s in rows]))
    single = {n: ctx.fit_stamps_elliptical(s[None])[0] for n, s in rows if n.startswith('good')}
    st = _status(fit)
    bad, worst = [], 0.0
    for k, (name, s) in enumerate(rows):
        print('degenerate %s %s: status %d it %d row %s' % (prec, name, st[k], fit[k, 10], fit[k, :10]))
        if (st[k] & 3) == 0 and not np.all(np.isfinite(fit[k])):
            bad.append((name, 'a non-finite number beside status 0', fit[k]))
        if name.startswith('good'):
            if not (np.array_equal(fit[k], single[name]) and st[k] == 0):
                bad.append((name, 'differs from its single-stamp fit', fit[k], single[name]))
            continue
        if (st[k] & 3) == 0:
            res = _model_residual(fit[k], s)
            print('   model residual %.3e of the peak' % res)
            worst = max(worst, res)
            if not res < STAMP_TOL[prec]:
                bad.append((name, 'status 0 without a model that reproduces the stamp', res, fit[k]))
    record_margin('fit_ell_columns', **{'degenerate_%s_model_residual_of_status_0_rows' % prec: min(worst, 1e300),
                                        'degenerate_%s_rows_refused' % prec: int(np.sum((st & 3) != 0))})
    assert not bad, bad


# ---- (e) amplitudes
AMPLITUDE_INSIDE = (-40, -30, -20, -10, 0, 10, 20, 30, 40)
AMPLITUDE_OUTSIDE = (-60, -41, 41, 60)


@pytest.mark.parametrize('prec', PRECS)
def test_amplitude_range(ctx, prec):
    """The three bases of the circular amplitude test made elliptical (b/a 0.7, rot 30): a perturbed Moffat, exact
    ones with steep and with broad wings, brightest pixel 1, times 2^k.  include/mpsfr.h: a brightest pixel in
    [2^-40, 2^40] is fitted -- status 0, the parameters right to TOL with the peak scaled by 2^k, and on the perturbed
    base, where they are no rounding noise, chi2 (scaled by 4^k), flux and err_peak (by 2^k) and the other error
    columns right to 1e-3 against fit_full of the base -- and one outside is refused with status 2.  Nowhere
    status & 3 == 0 on a wrong answer."""
    bases = []
    a = M.stamp(1.0, 19.7, 20.4, 5.0, 0.7, 30.0, 2.5) + M.stamp(1e-3, 20.5, 19.8, 12.0, 1.0, 0.0, 1.8)
    a /= a.max()
    bases.append(('perturbed', a, M.fit(a, _lm(1.0, 19.7, 20.4, 5.0, 0.7, 30.0, 2.5))))
    for name, fw, n in (('steep', 3.0, 4.0), ('broad', 12.0, 1.5)):
        m = M.stamp(1.0, 19.7, 20.4, fw, 0.7, 30.0, n)
        bases.append((name, m / m.max(), _lm(1.0 / m.max(), 19.7, 20.4, fw, 0.7, 30.0, n)))
    ks = AMPLITUDE_INSIDE + AMPLITUDE_OUTSIDE
    assert len(ks) == 13 and len(bases) == 3
    assert sorted(ks) == [-60, -41, -40, -30, -20, -10, 0, 10, 20, 30, 40, 41, 60]
    for name, base, v in bases:
        assert base.max() == 1.0 and M.kappa(v) < 100, name
    fit = ctx.fit_stamps_elliptical(np.array([base * 2.0 ** k for _, base, _ in bases for k in ks]))
    assert fit.shape == (39, 24)
    bad, worst, worst_col = [], 0.0, 0.0
    full = M.fit_full(bases[0][1], bases[0][2])
    assert np.abs(full['v'] - bases[0][2]).max() <= 1e-9
    for b, (name, base, v) in enumerate(bases):
        for j, k in enumerate(ks):
            row = fit[b * len(ks) + j]
            s = int(row[18])
            vk = v.copy()
            vk[0] *= 2.0 ** k
            with np.errstate(all='ignore'):
                w = _param_errors(row, vk, prec)
            right = all(np.isfinite(x) for x in w.values()) and max(w.values()) <= 1.0
            print('amplitude %s %s k=%d: status %d it %d chi2 / 4^k %.4g error / tolerance %.3g' % (
                prec, name, k, s, row[10], row[9] / 4.0 ** k, max(w.values())))
            if (s & 3) == 0 and not (right and np.all(np.isfinite(row))):
                bad.append((name, k, 'status 0 on a wrong answer', row))
            if k in AMPLITUDE_OUTSIDE:
                if (s & 3) != 2:
                    bad.append((name, k, 'outside the range and not refused', s))
                continue
            worst = max(worst, max(w.values()))
            if not (s == 0 and right and row[10] < MAXIT):
                bad.append((name, k, 'inside the range', s, row[10], w))
            if name == 'perturbed':
                unscaled = row.copy()
                unscaled[[11, 19, 20]] /= 2.0 ** k
                unscaled[9] /= 4.0 ** k
                col = max(abs(unscaled[M.COLUMN[c]] / full[c] - 1.0) for c in ERR_COLUMNS)
                worst_col = max(worst_col, col)
                if not col < COLUMN_TOL:
                    bad.append((name, k, 'columns inside the range', col))
    print('amplitude %s: inside the range, parameters %.3g of the tolerance, columns %.3g relative' % (
        prec, worst, worst_col))
    record_margin('fit_ell_columns', **{'amplitude_%s_inside' % prec: worst,
                                        'amplitude_%s_inside_rel_columns' % prec: worst_col})
    assert not bad, bad


# ---- (f) start values
@pytest.mark.parametrize('prec', PRECS)
def test_start_values_through_the_iteration_count(ctx, prec):
    """The start is not an output and the minimum is unique: what the start controls is the iteration count.  Exact
    stamps of FWHM 5, n 2.5 with b/a 1, 0.7, 0.5 at rot 0, 45, 100, 150, in the middle of the stamp and with the
    brightest pixel 6 px from the top edge (the smallest disc the moment start takes), in one call.  With the moment
    start of (e1, e2) an elongated stamp starts as near to its minimum as the round one: it takes at most 3 more
    iterations than the round stamp at the same place, the allowance of the circular test for its hardest class.  A
    start at e = 0, or with a wrong sign of e2, costs more than that."""
    rots, places = (0.0, 45.0, 100.0, 150.0), (('middle', (19.2, 20.3)), ('rm6', (6.2, 20.3)))
    cases = [(where, ba, rot, (1.0, p0, q0, 5.0, ba, rot, 2.5)) for where, (p0, q0) in places for ba in (1.0, 0.7, 0.5)
             for rot in rots]
    assert len(cases) == 24
    stamps = np.array([M.stamp(*p) for _, _, _, p in cases])
    for (where, _, _, _), s in zip(cases, stamps):
        a, b = np.unravel_index(s.argmax(), s.shape)
        assert min(a, 39 - a, b, 39 - b) == (6 if where == 'rm6' else 19)
    fit = ctx.fit_stamps_elliptical(stamps)
    assert np.all(fit[:, 18] == 0), fit[:, 18]
    par = _worst(_param_errors(row, _lm(*p), prec) for row, (_, _, _, p) in zip(fit, cases))
    assert max(par.values()) <= 1.0, par
    it = fit[:, 10].astype(int)
    table = {(where, ba): [int(it[k]) for k, c in enumerate(cases) if c[0] == where and c[1] == ba]
             for where, _ in places for ba in (1.0, 0.7, 0.5)}
    print('start %s: iterations over rot %s: %s' % (prec, rots, table))
    extra = 0
    for where, _ in places:
        round_it = max(table[(where, 1.0)])
        for ba in (0.7, 0.5):
            extra = max(extra, max(table[(where, ba)]) - round_it)
        record_margin('fit_ell_columns', **{'start_%s_%s_round_iterations' % (prec, where): round_it})
    record_margin('fit_ell_columns', **{'start_%s_extra_iterations' % prec: max(extra, 0)})
    assert extra <= 3, table
