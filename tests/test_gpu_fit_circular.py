"""GPU: K_FIT alone, the circular Moffat fit the product's tables come from, through Context.fit_stamps in both
precision modes, on stamps it was not designed on: exact Moffats over the parameter range, off the centre and
off the stamp, sub-pixel ties, perturbed stamps with a known minimum, flagged (ill-conditioned) fits, amplitudes
from 2^-60 to 2^60, degenerate stamps.  References: the truth for exact Moffats, MINPACK (tests/tail_ref.py) else.

Tolerances are the project's (test_fit_kernel_against_minpack_on_golden_stamps, the parity metric): n to 1e-4
(mixed) / 1e-6 (f64), FWHM to the same in arcsec at 0.2 arcsec/px, centre 1e-4 / 1e-6 px, peak 1e-5 / 1e-7
relative.  They apply where the ill-conditioning number tail_ref.kappa is below 100, the header's own threshold
(MPSFR_FIT_ILL_CONDITIONED); every test asserts that premise for the stamps it holds to them.  Worst errors go to
the margins file as error / tolerance.
"""
import numpy as np
import pytest

import psfr_oracle as O
import tail_ref as T
from conftest import record_margin

pytestmark = pytest.mark.gpu

PS = 0.2
TOL = {'mixed': dict(n=1e-4, fwhm=1e-4, centre=1e-4, peak=1e-5, stamp=2e-5),
       'f64': dict(n=1e-6, fwhm=1e-6, centre=1e-6, peak=1e-7, stamp=1e-9)}
MAXIT = 200                                  # MPSFR_FIT_MAXIT: the cap of the LM phase
PRECS = ['mixed', 'f64']


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _fit(api, prec, stamps):
    ctx = api.Context(dim=128, pixscale=PS, precision=prec)
    f = ctx.fit_stamps(np.asarray(stamps, dtype=np.float64))
    ctx.close()
    return f


def _ratios(f, want, prec):
    """error / tolerance of (n, fwhm, centre, peak) per stamp; want: rows (peak, p0, q0, fwhm px, n)"""
    want = np.asarray(want, dtype=np.float64)
    t = TOL[prec]
    return np.stack([np.abs(f[:, 4] - want[:, 4]) / t['n'],
                     np.abs(f[:, 5] - want[:, 3]) * PS / t['fwhm'],
                     np.abs(f[:, 1:3] - want[:, 1:3]).max(axis=1) / t['centre'],
                     np.abs(f[:, 0] / want[:, 0] - 1) / t['peak']], axis=1)


def _report(tag, prec, f, want, names=None):
    r = _ratios(f, want, prec)
    k = int(r.max(axis=1).argmax())
    print('%s %s: worst error / tolerance n %.3g fwhm %.3g centre %.3g peak %.3g; worst stamp %s -> %s status %s it %s'
          % (tag, prec, *r.max(axis=0), (names[k] if names else tuple(want[k])), f[k, :6], f[k, 14], f[k, 7]))
    record_margin('fit_circular', **{'%s_%s_%s' % (tag, prec, c): v for c, v in zip(('n', 'fwhm', 'centre', 'peak'),
                                                                                 r.max(axis=0))})
    return r


def well_posed_grid():
    """FWHM {2, 3, 5, 8, 12, 20, 30, 45} x n {1.1, 1.5, 2, 2.5, 4} and n = 8 at FWHM {5, 8, 12, 20, 30} (kappa <= 63);
    peak in [0.5, 2], centre (19.5, 19.5) + uniform(-2, 2), seeded."""
    rng = np.random.default_rng(50)
    grid = [(fw, n) for fw in (2, 3, 5, 8, 12, 20, 30, 45) for n in (1.1, 1.5, 2, 2.5, 4)]
    grid += [(fw, 8) for fw in (5, 8, 12, 20, 30)]
    return [(rng.uniform(0.5, 2), 19.5 + rng.uniform(-2, 2), 19.5 + rng.uniform(-2, 2), float(fw), float(n))
            for fw, n in grid]


def flagged_grid():
    """n {20, 50} x FWHM {2, 3, 5, 8, 12, 20, 30, 45} and n = 8 at FWHM {1.5, 2}: kappa >= 136"""
    rng = np.random.default_rng(51)
    grid = [(fw, n) for n in (20, 50) for fw in (2, 3, 5, 8, 12, 20, 30, 45)] + [(1.5, 8), (2, 8)]
    return [(rng.uniform(0.5, 2), 19.5 + rng.uniform(-0.5, 0.5), 19.5 + rng.uniform(-0.5, 0.5), float(fw), float(n))
            for fw, n in grid]


@pytest.mark.parametrize('prec', PRECS)
def test_synthetic_recovery_centred(api, prec):
    """Exact Moffats over the parameter range, centre within 2 px of the middle: the truth is the yardstick."""
    truth = well_posed_grid()
    assert len(truth) == 45 and max(T.kappa(*t) for t in truth) < 100
    f = _fit(api, prec, [T.moffat_stamp(*t) for t in truth])
    r = _report('centred', prec, f, truth)
    assert np.all((f[:, 14].astype(int) & 3) == 0), f[:, 14]
    assert np.all(f[:, 14] == 0), f[:, 14]                     # (kappa <= 63: no flag either)
    assert np.all(f[:, 7] < MAXIT), f[:, 7]
    assert r.max() < 1, r


@pytest.mark.parametrize('prec', PRECS)
def test_subpixel_phase_and_ties(api, prec):
    """FWHM 3 and 8, n 2.5, centre (20 + dy, 20 + dx), dy, dx in {0, 0.25, 0.5, 0.75}: at 0.5 two or four
    brightest pixels are exactly equal (the argmax tie rule: the first maximum in C order)."""
    truth = [(1.0, 20 + dy, 20 + dx, fw, 2.5) for fw in (3.0, 8.0) for dy in (0, 0.25, 0.5, 0.75)
             for dx in (0, 0.25, 0.5, 0.75)]
    stamps = [T.moffat_stamp(*t) for t in truth]
    s = stamps[2 * 4 + 2]                                       # (20.5, 20.5): four equal maxima
    assert s[20, 20] == s[20, 21] == s[21, 20] == s[21, 21] == s.max()
    # two equal Moffats at (10, 10) and (29, 29): two exactly equal maxima 19 pixels apart, each with a minimum of its
    # own.  The start is the first maximum in C order (np.argmax, as in the reference's fit), so the fit lands on the
    # first one; with any other tie rule the centre is off by 19 px.  Yardstick: MINPACK from the first peak.
    two = T.moffat_stamp(1.0, 10.0, 10.0, 3.0, 2.5) + T.moffat_stamp(1.0, 29.0, 29.0, 3.0, 2.5)
    assert two[10, 10] == two[29, 29] == two.max() and np.argmax(two) == 10 * 40 + 10
    a = T.fit(two, (1.0, 10.0, 10.0, 3.0, 2.5))
    assert abs(a['p0'] - 10) < 0.1 and abs(a['q0'] - 10) < 0.1
    stamps.append(two)
    truth.append((a['peak'], a['p0'], a['q0'], a['fwhm'], a['n']))
    assert T.kappa(*truth[-1]) < 100
    f = _fit(api, prec, stamps)
    r = _report('ties', prec, f, truth)
    assert np.all(f[:, 14] == 0) and np.all(f[:, 7] < MAXIT)
    assert r.max() < 1, r


def off_centre_cases():
    cases = []
    for fw in (3.0, 8.0):
        for rm in (0, 1, 3, 5, 6, 7, 12):
            cases.append(('edge_rm%d_fwhm%g' % (rm, fw), (1.0, rm + 0.2, 20.3, fw, 2.5)))
            cases.append(('corner_rm%d_fwhm%g' % (rm, fw), (1.0, rm + 0.2, 39 - rm - 0.3, fw, 2.5)))
        cases.append(('outside_fwhm%g' % fw, (1.0, -0.4, 12.0, fw, 2.5)))
    return cases


@pytest.mark.parametrize('prec', PRECS)
def test_off_centre_and_off_the_stamp(api, prec):
    """The same two profiles with the brightest pixel at distance rm = 0, 1, 3, 5, 6, 7, 12 from one edge, from two
    edges (a corner), and with the centre half a pixel outside the stamp.  rm = 5 / 6 straddles the switch between the
    fallback start (half-maximum area, eta 0.4) and the moment start.  Yardstick: the truth (kappa <= 30).

    The minimum is unique, so the converged parameters say nothing about the start; what the start controls is the
    iteration count, and that is what pins it here, against the same profile in the middle of the stamp, fitted in
    the same call.  Both start recipes are invariant under translation as long as the core of the profile is on the
    stamp: the half-maximum pixel count of the fallback does not change, and the moment start corrects for its disc
    radius (T1, T2).  So with the brightest pixel three pixels or more from every edge (the half-maximum radius of the
    wider profile is 4 px) the fit takes no more iterations than in the middle.  Nearer to the edge the half-maximum
    area is cut, down to a quarter at a corner, so the fallback's FWHM is off by a factor of up to two; LM from a
    width wrong by that factor reaches the 1e-3 of its convergence test in three more iterations than from a start
    within ten per cent (relative error 1 -> 0.3 -> 0.05 -> 1e-3, quadratic at the end): at most three more.  A
    fallback with eta0 = 0.04 instead of 0.4, or the moment start taken at rm < 6 where its disc holds a handful of
    pixels, breaks the first bound (and the second: 13 iterations at rm = 0)."""
    cases = off_centre_cases()
    truth = [t for _, t in cases]
    assert len(cases) == 30 and max(T.kappa(*t) for t in truth) < 100
    middle = {3.0: (1.0, 19.2, 20.3, 3.0, 2.5), 8.0: (1.0, 19.2, 20.3, 8.0, 2.5)}       # same sub-pixel phase
    stamps = [T.moffat_stamp(*t) for t in truth] + [T.moffat_stamp(*middle[fw]) for fw in (3.0, 8.0)]
    for (name, t), s in zip(cases, stamps):
        if not name.startswith('outside'):
            a, b = np.unravel_index(s.argmax(), s.shape)
            rm = int(name.split('_rm')[1].split('_')[0])
            assert min(a, 39 - a, b, 39 - b) == rm, name
    f = _fit(api, prec, stamps)
    r = _report('off_centre', prec, f, truth + [middle[3.0], middle[8.0]], [n for n, _ in cases] + ['middle3', 'middle8'])
    assert np.all(f[:, 14] == 0), f[:, 14]
    assert np.all(f[:, 7] < MAXIT), f[:, 7]
    assert r.max() < 1, [(cases[k][0], r[k]) for k in range(len(cases)) if r[k].max() >= 1]
    it_mid = {3.0: f[-2, 7], 8.0: f[-1, 7]}
    print('off_centre %s iterations: middle %s; %s' % (prec, it_mid, [(n, int(f[k, 7])) for k, (n, _) in enumerate(cases)]))
    slow = []
    for k, (name, t) in enumerate(cases):
        on_stamp = not name.startswith('outside') and int(name.split('_rm')[1].split('_')[0]) >= 3
        if f[k, 7] > it_mid[t[3]] + (0 if on_stamp else 3):
            slow.append((name, int(f[k, 7]), int(it_mid[t[3]])))
    assert not slow, slow


@pytest.mark.parametrize('prec', PRECS)
def test_perturbed_stamps_against_minpack(api, prec):
    """Moffat + a fixed perturbation of 1e-3 of the peak (a second, wider Moffat; a seeded noise field), centred and
    with the brightest pixel four pixels from an edge: the minimum is not the truth, and MINPACK finds it from two
    starts to 1e-9 (held on the CPU by tests/test_tail_ref.py; the count is asserted here: no case is dropped).
    Parameters to the tolerances of this file; err_*, flux and chi2 against the covariance recipe of
    oracle.moffat_fit(errors=True) (tail_ref.fit evaluates the same recipe) at 1e-3 relative."""
    cases = T.perturbed_cases()
    assert len(cases) == 8
    refs = []
    for name, truth, stamp in cases:
        a, b = T.fit(stamp, truth), T.fit(stamp, tuple(1.05 * x for x in truth))
        assert all(abs(a[k] - b[k]) < 1e-9 * max(abs(a[k]), 1.0) for k in ('peak', 'p0', 'q0', 'fwhm', 'n')), name
        assert T.kappa(a['peak'], a['p0'], a['q0'], a['fwhm'], a['n']) < 100
        refs.append(a)
    assert len(refs) == 8
    f = _fit(api, prec, [s for _, _, s in cases])
    want = [(a['peak'], a['p0'], a['q0'], a['fwhm'], a['n']) for a in refs]
    r = _report('perturbed', prec, f, want, [n for n, _, _ in cases])
    cols = dict(err_peak=8, err_p0=9, err_q0=10, err_alpha=11, err_n=12, err_fwhm=13, flux=15, chi2=6)
    worst = {c: max(abs(f[k, j] / refs[k][c] - 1) for k in range(len(refs))) for c, j in cols.items()}
    print('perturbed %s: relative errors of the columns %s' % (prec, worst))
    record_margin('fit_circular', **{'perturbed_%s_rel_%s' % (prec, c): v for c, v in worst.items()})
    assert np.all(f[:, 14] == 0) and np.all(f[:, 7] < MAXIT)
    assert r.max() < 1, r
    assert max(worst.values()) < 1e-3, worst


@pytest.mark.parametrize('prec', PRECS)
def test_ill_conditioned_flag_and_flagged_fits(api, prec):
    """The status bit MPSFR_FIT_ILL_CONDITIONED equals kappa >= 100, on stamps away from the threshold (flagged side
    kappa >= 136, unflagged side kappa <= 63).  Flagged fits are not left unchecked: they converge
    (status & 3 == 0), the peak is right to 1e-3 relative and the centre to 1e-3 px, and the fitted model, evaluated
    here in fp64, reproduces the stamp in the max norm to the project's stamp tolerance (2e-5 of the peak mixed, 1e-9
    f64): the valley is flat in (w, n), not in the residual.  The residual MINPACK leaves from the oracle's fixed
    start on the same stamp goes to the margins file beside the kernel's."""
    flagged, clear = flagged_grid(), well_posed_grid()
    kf, kc = [T.kappa(*t) for t in flagged], [T.kappa(*t) for t in clear]
    assert len(flagged) == 18 and min(kf) >= 130 and max(kc) <= 65, (min(kf), max(kc))
    stamps = [T.moffat_stamp(*t) for t in flagged + clear]
    f = _fit(api, prec, stamps)
    st = f[:, 14].astype(int)
    nf = len(flagged)
    print('flag %s: flagged side status %s, unflagged side status %s' % (prec, st[:nf], st[nf:]))
    res, res_ref = [], []
    for k, t in enumerate(flagged):
        model = T.moffat_stamp(f[k, 0], f[k, 1], f[k, 2], f[k, 5], f[k, 4])
        res.append(np.abs(model - stamps[k]).max() / t[0])
        o = O.moffat_fit(stamps[k], 1.0)
        res_ref.append(np.abs(T.moffat_stamp(*o) - stamps[k]).max() / t[0])
    res, res_ref = np.array(res), np.array(res_ref)
    tr = np.array(flagged)
    dpk = np.abs(f[:nf, 0] / tr[:, 0] - 1).max()
    dce = np.abs(f[:nf, 1:3] - tr[:, 1:3]).max()
    print('flagged %s: peak %.3e centre %.3e residual of the fitted model %s; MINPACK leaves %s; fitted (fwhm, n) %s'
          % (prec, dpk, dce, res, res_ref, f[:nf, 4:6]))
    record_margin('fit_circular', **{'flagged_%s_peak_rel' % prec: dpk, 'flagged_%s_centre_px' % prec: dce,
                                     'flagged_%s_model_residual' % prec: res.max(),
                                     'flagged_%s_minpack_residual' % prec: res_ref.max()})
    assert np.all((st[:nf] & 4) == 4) and np.all((st[nf:] & 4) == 0), st
    assert np.all((st & 3) == 0), st
    assert dpk < 1e-3 and dce < 1e-3
    assert res.max() < TOL[prec]['stamp'], res


# Amplitudes (include/mpsfr.h, mpsfr_fit_stamps): brightest pixels of 2^-40 .. 2^40 are fitted, bit for bit alike
# from 2^-20 up; anything else is refused.
AMPLITUDE_EXACT = (-20, -10, 0, 10, 20, 30, 40)
AMPLITUDE_TOLERANCE = (-40, -30)
AMPLITUDE_OUTSIDE = (-60, -41, 41, 60)


@pytest.mark.parametrize('prec', PRECS)
def test_amplitude_range(api, prec):
    """Three well-posed stamps (a perturbed Moffat; exact ones with steep and with broad wings), brightest pixel 1,
    times 2^k.  For k in [-20, 40] every column is that of k = 0 bit for bit, with peak, flux, err_peak scaled by 2^k
    and chi2 by 4^k exactly: a power of two changes no mantissa while every term of the fp32 sums is a normal number.
    For k in [-40, -20) the squared residuals of a nearly exact fit are subnormal in fp32: status and iterations are
    those of k = 0 and (n, fwhm, centre, peak) are right to the tolerances of this file; chi2 and the err_* columns
    are not claimed.  Outside [-40, 40] the stamp is refused: status & 3 != 0 (or a right answer), never status 0 on a
    wrong one."""
    bases = []
    a = T.moffat_stamp(1.0, 19.7, 20.4, 5.0, 2.5) + T.moffat_stamp(1e-3, 20.5, 19.8, 12.0, 1.8)
    a /= a.max()
    ref = T.fit(a, (1.0, 19.7, 20.4, 5.0, 2.5))
    bases.append(('perturbed', a, (ref['peak'], ref['p0'], ref['q0'], ref['fwhm'], ref['n'])))
    for name, fw, n in (('steep', 3.0, 4.0), ('broad', 12.0, 1.5)):
        m = T.moffat_stamp(1.0, 19.7, 20.4, fw, n)
        bases.append((name, m / m.max(), (1.0 / m.max(), 19.7, 20.4, fw, n)))
    ks = AMPLITUDE_EXACT + AMPLITUDE_TOLERANCE + AMPLITUDE_OUTSIDE
    bad = []
    for name, base, want0 in bases:
        assert base.max() == 1.0 and T.kappa(*want0) < 100
        f = _fit(api, prec, [base * 2.0 ** k for k in ks])
        f0 = f[ks.index(0)]
        for row, k in zip(f, ks):
            sc = 2.0 ** k
            unscaled = row.copy()
            unscaled[[0, 8, 15]] /= sc
            unscaled[6] /= sc * sc
            bit = np.array_equal(unscaled, f0)
            r = _ratios(np.array([unscaled]), [want0], prec)[0]
            print('amplitude %s %s k=%d: status %d it %d bit-equal to k=0: %s; error / tolerance %s' %
                  (prec, name, k, row[14], row[7], bit, r))
            if k in AMPLITUDE_OUTSIDE:
                if not ((int(row[14]) & 3) != 0 or (np.all(np.isfinite(r)) and r.max() < 1)):
                    bad.append((name, k, 'outside the range: status 0 on a wrong answer', row))
                continue
            record_margin('fit_circular', **{'amplitude_%s_inside' % prec: r.max()})
            if not (row[14] == 0 and row[7] == f0[7] and r.max() < 1):
                bad.append((name, k, 'inside the range', row[14], row[7], r))
            if k in AMPLITUDE_EXACT and not bit:
                bad.append((name, k, 'not bit-equal to k = 0', unscaled - f0))
    assert not bad, bad


def degenerate_batch():
    good = [T.moffat_stamp(1.0, 19.7, 20.4, 5.0, 2.5), T.moffat_stamp(0.8, 18.2, 21.1, 8.0, 1.5),
            T.moffat_stamp(1.5, 20.9, 19.0, 3.0, 4.0)]
    hot_mid, hot_corner = np.zeros((40, 40)), np.zeros((40, 40))
    hot_mid[20, 20] = 1.0
    hot_corner[0, 39] = 1.0
    with_nan, with_inf = good[0].copy(), good[0].copy()
    with_nan[7, 11] = np.nan
    with_inf[30, 5] = np.inf
    rows = [('good0', good[0]), ('zero', np.zeros((40, 40))), ('good1', good[1]), ('constant', np.ones((40, 40))),
            ('negative', -good[0] - 0.1), ('good2', good[2]), ('hot_middle', hot_mid), ('hot_corner', hot_corner),
            ('good0_again', good[0]), ('nan_pixel', with_nan), ('inf_pixel', with_inf), ('good1_again', good[1])]
    return rows


@pytest.mark.parametrize('prec', PRECS)
def test_degenerate_stamps_between_good_ones(api, prec):
    """All zero, constant 1, all negative, one hot pixel (middle, corner), a Moffat with one NaN pixel and one with a
    +inf pixel, in one batch between good stamps: data the entry point accepts.  The call returns; the good stamps
    equal their single-stamp fits bit for bit (a wave per stamp: no neighbour is touched); every degenerate row has
    status & 3 != 0, or finite outputs whose model reproduces the stamp to the stamp tolerance; no row has a NaN
    beside status 0 (the rule of include/mpsfr.h next to the status codes)."""
    rows = degenerate_batch()
    ctx = api.Context(dim=128, pixscale=PS, precision=prec)
    f = ctx.fit_stamps(np.array([s for _, s in rows]))
    single = {n: ctx.fit_stamps(s[None])[0] for n, s in rows if n.startswith('good')}
    ctx.close()
    bad = []
    for k, (name, s) in enumerate(rows):
        st = int(f[k, 14])
        print('degenerate %s %s: status %d it %d row %s' % (prec, name, st, f[k, 7], f[k, :7]))
        if name.startswith('good'):
            if not (np.array_equal(f[k], single[name]) and st == 0):
                bad.append((name, 'differs from its single-stamp fit', f[k], single[name]))
            continue
        if (st & 3) == 0:
            ok = bool(np.all(np.isfinite(f[k])))
            if ok:
                model = T.moffat_stamp(f[k, 0], f[k, 1], f[k, 2], f[k, 5], f[k, 4])
                res = np.abs(model - s).max() / np.abs(s).max()
                print('   model residual %.3e of the peak' % res)
                ok = res < TOL[prec]['stamp']
            if not ok:
                bad.append((name, 'status 0 without a model that reproduces the stamp', f[k]))
    assert not bad, bad


def test_the_float_stamp_instantiation_inside_a_call(api):
    """k_fit<float, float> is reached only through a reconstruct that keeps its final stamps on the device as floats
    (no stamps asked for).  A 512^2 mixed call: the fit rows of a call with stamps (k_fit<float, double>) and of a call
    without (k_fit<float, float>) against fit_stamps of the returned stamps (float values carried in doubles):
    parameters to the mixed tolerances, status equal."""
    see, gl, l0 = api.synthetic_rows(6, seed=5)
    lb = np.array([465.0, 600.0, 700.0, 930.0])
    ctx = api.Context(dim=512, pixscale=api.grid_pixscale(512), precision='mixed')
    a = ctx.reconstruct(lb, see, gl, l0)
    b = ctx.reconstruct(lb, see, gl, l0, want_psf=False)
    alone = ctx.fit_stamps(a['psf'])
    ctx.close()
    assert np.array_equal(a['psf'].astype(np.float32).astype(np.float64), a['psf'])
    want = alone[:, [0, 1, 2, 5, 4]]
    for tag, r in (('in_call_double_stamps', a), ('in_call_float_stamps', b)):
        f = r['fit'].reshape(-1, alone.shape[1])
        q = _report(tag, 'mixed', f, want)
        assert np.array_equal(f[:, 14], alone[:, 14]) and np.all(f[:, 14] == 0)
        assert q.max() < 1, q
