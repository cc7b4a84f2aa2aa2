"""CPU: the fp64 oracle as the yardstick of Cn2-profile calls (oracle/psfr_oracle.py with per-layer winds and
arbitrary directions; the cases of tests/profile_cases.py).

1. The extended oracle against the reference's profile goldens a-d (tests/golden/g9_profile*.npz): corrected zones
   below 1e-13, and for the 512^2 cases a and d the stamps before / after the convolutions (1e-12) and the fit (2e-7
   relative), the bounds tests/test_oracle.py holds the oracle to.
2. With the new arguments left out the oracle returns the bits it returned before.
3. The oracle's own error on the profile at the header's limits (PX), against one evaluation of the layer tables in
   long double written here: below 1e-13 of a table's maximum, ten times under the bound of the GPU test.
4. The inputs discriminate: each of the mistakes a mixing kernel can make moves the structure function of every
   multi-row case by at least 2e-5 of its maximum, 100 times the mixed-precision bound.
5. The oracle's own fits of the cases at 512^2 and above are well-posed, so the GPU test compares all of them.
"""
import numpy as np
import pytest

import profile_cases as PC
import psfr_oracle as O
from conftest import rel_err


# ---- 1. goldens
def _golden_case(golden, case):
    g = golden('g9_profile_field' if case == 'd' else 'g9_profile')
    return {k[2:]: g[k] for k in g.files if k.startswith(case + '_')}


def _golden_psd(c, ref_masks):
    return O.residual_psd(c['cn2'], c['h'], float(c['seeing']), float(c['L0']), 1, int(c['dim']), bool(c['three']),
                          wind_speed=c['ws'], wind_dir=c['wd'], directions=c['dirs'],
                          tables=O.ao_tables(c['h'], bool(c['three']), 1, masks=ref_masks, wind_speed=c['ws'],
                                             wind_dir=c['wd'], directions=c['dirs']))


@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd'])
def test_oracle_reproduces_the_profile_goldens(golden, ref_masks, case):
    c = _golden_case(golden, case)
    dim = int(c['dim'])
    psd = _golden_psd(c, ref_masks)
    sl = slice(dim // 2 - 40, dim // 2 + 40)
    assert psd.shape == (c['dirs'].shape[1], dim, dim)
    err = rel_err(psd[:, sl, sl], c['zone'])
    print('case %s: zone %.2e' % (case, err))
    assert err < 1e-13
    if case not in 'ad':
        return
    ps = PC.grid_pixscale(dim)
    lb = c['lbda']
    see, gl, l0 = float(c['seeing']), float(c['gl']), float(c['L0'])
    groups = [psd] if int(c['npsflin']) else list(psd)             # (d: one PSF per position)
    gpre, gfin = c['pre'].reshape(len(groups), lb.size, 40, 40), c['fin'].reshape(len(groups), lb.size, 40, 40)
    gfit = c['fit'].reshape(len(groups), lb.size, 5)
    for k, p in enumerate(groups):
        pre = O.psf_stamps_refshaped(p, lb, 40, ps)
        assert rel_err(pre, gpre[k]) < 1e-12
        fin = O.convolve_final_psf(lb, see, gl, l0, pre, ps)
        assert rel_err(fin, gfin[k]) < 1e-12
        np.testing.assert_allclose(O.fit_psf_cube(fin, ps)[:, 3:], gfit[k][:, 3:], rtol=2e-7)


def test_ao_zone_psd_builds_profile_tables_itself(golden, ref_masks):
    """ao_zone_psd and residual_psd pass the three arguments through when they are given no tables (numpy_cutoff_masks
    of this interpreter may differ from the goldens' on the |k| = 24 lines: compared with the oracle's own tables)."""
    c = _golden_case(golden, 'a')
    kw = dict(wind_speed=c['ws'], wind_dir=c['wd'], directions=PC.POS2.T)
    tabs = O.ao_tables(c['h'], False, 1, **kw)
    a = O.residual_psd(c['cn2'], c['h'], 0.9, 22.0, 1, 128, False, **kw)
    b = O.residual_psd(c['cn2'], c['h'], 0.9, 22.0, 1, 128, False, tables=tabs)
    assert a.shape == (2, 128, 128) and np.array_equal(a, b)
    assert not np.array_equal(a[0], a[1])
    # a scalar wind speed applies to every layer
    t1 = O.ao_tables(c['h'], True, 1, wind_speed=9.0, wind_dir=c['wd'])
    t3 = O.ao_tables(c['h'], True, 1, wind_speed=[9.0, 9.0, 9.0], wind_dir=c['wd'])
    assert all(np.array_equal(x, y) for x, y in zip(t1, t3))


# ---- 2. defaults
@pytest.mark.parametrize('h,speed', [((100, 10000), 12.0), ((100.0, 10000.0), 12.5)])
@pytest.mark.parametrize('three', [False, True])
def test_defaults_return_the_same_bits(h, speed, three):
    """The two-layer call with the reference's winds and directions passed explicitly is the call with none -- and the
    wind_speed_for quirk stays: 12 m/s for integer altitudes, 12.5 for float ones (psfrec.py:61)."""
    assert np.all(O.wind_speed_for(np.array(h)) == speed)
    explicit = dict(wind_speed=(speed, speed), wind_dir=O.WIND_DIR, directions=O.eval_directions(3))
    a = O.ao_tables(h, three, 3, exact_masks=True)
    b = O.ao_tables(h, three, 3, exact_masks=True, **explicit)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    r0 = O.seeing_to_r0(0.8)
    assert np.array_equal(O.ao_zone_psd([0.7, 0.3], h, 20.0, r0, three, 3),
                          O.ao_zone_psd([0.7, 0.3], h, 20.0, r0, three, 3, **explicit))
    assert np.array_equal(O.residual_psd([0.7, 0.3], h, 0.8, 20.0, 3, 128, three),
                          O.residual_psd([0.7, 0.3], h, 0.8, 20.0, 3, 128, three, **explicit))
    other = O.ao_tables(h, three, 3, exact_masks=True, wind_speed=(speed, speed + 0.5), wind_dir=O.WIND_DIR)
    assert not np.array_equal(a[0], other[0])


# ---- 3. the yardstick's own error at the header's limits
def _tables_long_double(prof, three, dirs):
    """T[layer][dir][80][80] and noise[dir][80][80] of dsp4muse (psfrec.py:218-364, :367-528, LSE, tempo) in long
    double, with the intended cut-off rule (exact_masks).  Written out on its own: phases as cos + i sin of long-double
    arguments, sinc as sin(pi x) / (pi x); nothing of oracle/psfr_oracle.py is called."""
    ld = np.longdouble
    pi = 4 * np.arctan(ld(1))
    k = np.fft.fftfreq(80, 1 / 80).astype(int)
    fx = (ld(1) * k / 16)[:, None] * np.ones((1, 80), ld)          # fftfreq(80, 8 / 40): k / 16 m^-1, exact
    fy = fx.T.copy()
    f = np.sqrt(fx * fx + fy * fy)
    with np.errstate(all='ignore'):
        arg = fy / fx
    arg[0, 0] = 0
    arg = np.arctan(arg)
    f_x, f_y = f * np.cos(arg), f * np.sin(arg)                     # psfrec.py:241-242

    def cis(x):
        return np.cos(x) + 1j * np.sin(x)

    def sinc(x):
        px = pi * x
        with np.errstate(all='ignore'):
            return np.where(x == 0, ld(1), np.sin(px) / np.where(x == 0, ld(1), px))

    pitch = ld(8) / 24
    arcmin_h = ld(60) / 206265
    lgs = [(1, 1), (-1, -1), (-1, 1)] if three else [(1, 1), (-1, -1), (-1, 1), (1, -1)]
    pos = np.array(lgs, ld) * 63 / 60
    ak = np.abs(k)
    wfs0 = 2j * pi * f * sinc(pitch * f_x) * sinc(pitch * f_y)
    w_rec = np.where((ak[:, None] >= 24) | (ak[None, :] >= 24), 0, wfs0)
    w_res = np.where((ak[:, None] > 24) | (ak[None, :] > 24), 0, wfs0)
    Mr = np.array([w_rec * cis(2 * pi * (f_x * p[0] + f_y * p[1]) * arcmin_h) for p in pos])     # DM at 1 m
    MAP = np.sum(Mr.conj() * Mr, axis=0)
    with np.errstate(all='ignore'):
        inv = np.where(MAP != 0, 1 / np.where(MAP != 0, MAP, 1), 0)
    inv[0, 0] = 0
    W = inv * Mr.conj()
    h = np.array(prof['h'], ld)
    ws, wd = np.array(prof['wind_speed'], ld), np.array(prof['wind_dir'], ld)
    vx, vy = ws * np.cos(wd), ws * np.sin(wd)
    ti, dt = ld(1) / 1000, ld(1) / 1000 + ld(25) / 10000
    dirs = np.array(dirs, ld) / 60
    T = np.zeros((h.size, dirs.shape[1], 80, 80), ld)
    noise = np.zeros((dirs.shape[1], 80, 80), ld)
    for d in range(dirs.shape[1]):
        bx, by = dirs[:, d]
        ptmp = cis(2 * pi * arcmin_h * (bx * f_x + by * f_y)) * W
        for i in range(h.size):
            mv = np.array([sinc(vx[i] * ti * f_x + vy[i] * ti * f_y) * w_res *
                           cis(2 * pi * h[i] * arcmin_h * (f_x * p[0] + f_y * p[1])) for p in pos])
            proj = cis(2 * pi * (h[i] * arcmin_h * (bx * f_x + by * f_y) - dt * (vx[i] * f_x + vy[i] * f_y))) \
                - np.sum(ptmp * mv, axis=0)
            T[i, d] = proj.real ** 2 + proj.imag ** 2
        noise[d] = np.sum(ptmp.real ** 2 + ptmp.imag ** 2, axis=0)
        noise[d, 0, 0] = 0
    return T, noise


@pytest.mark.parametrize('three', [False, True])
def test_oracle_tables_at_the_limits_against_long_double(three):
    dirs = np.array([(0.0, 0.0), (60.0, 60.0), (-60.0, 60.0), (60.0, -60.0), (-60.0, -60.0)]).T
    T, noise = O.ao_tables(PC.PX['h'], three, 1, exact_masks=True, wind_speed=PC.PX['wind_speed'],
                           wind_dir=PC.PX['wind_dir'], directions=dirs)
    Tl, nl = _tables_long_double(PC.PX, three, dirs)
    errs = [float(np.abs(T[i] - Tl[i]).max() / np.abs(Tl[i]).max()) for i in range(T.shape[0])]
    en = float(np.abs(noise - nl).max() / np.abs(nl).max())
    print('fp64 oracle vs long double, per layer:', ' '.join('%.1e' % e for e in errs), 'noise %.1e' % en)
    assert max(errs) < 1e-13 and en < 1e-13
    # (the comparison is not vacuous: tables of the order of 1, and the winds and altitudes of PX all matter)
    assert all(0.5 < float(Tl[i].max()) < 50 for i in range(T.shape[0]))


# ---- 4. the inputs discriminate
MOVE_MIN = 100 * 2e-7         # 100 x the mixed-precision bound on the structure function, of its maximum


def _d0_rows(inp, dim, tabs, cn2, normalise=True):
    """Structure functions [row][dir][..] of the rows with weights cn2 on tables tabs."""
    out = []
    for r, (s, l, th) in enumerate(zip(inp['seeing'], inp['l0'], inp['three'])):
        w = np.array(cn2[r], float)
        out.append(PC.oracle_d0(O.residual_psd(w, inp['h'], s, l, 1, dim, bool(th), tables=tabs[int(th)])))
    return np.array(out)


def _mistakes(inp, tabs, prof):
    """name -> (weights, tables) of a wrong mixing or of wrong tables."""
    w = inp['cn2'] / inp['cn2'].sum(axis=1, keepdims=True)
    n = w.shape[1]
    out = {'roll': (np.roll(w, 1, axis=1), tabs), 'next_row': (np.roll(w, -1, axis=0), tabs),
           'row0_for_all': (np.repeat(w[:1], len(w), axis=0), tabs)}
    for l in range(n - 1):
        s = w.copy()
        s[:, [l, l + 1]] = s[:, [l + 1, l]]
        out['swap%d%d' % (l, l + 1)] = (s, tabs)
    # (the last layer left out: its table zeroed, the weights as they were -- residual_psd normalises what it is given)
    out['last_out'] = (w, {g: (np.concatenate([T[:-1], 0 * T[-1:]]), nz) for g, (T, nz) in tabs.items()})
    wd = np.array(prof['wind_dir'])
    out['wind_xy'] = (w, PC.oracle_tables(dict(prof, wind_dir=np.pi / 2 - wd), inp['dirs']))     # cos <-> sin
    out['speeds_reversed'] = (w, PC.oracle_tables(dict(prof, wind_speed=prof['wind_speed'][::-1]), inp['dirs']))
    return out


@pytest.mark.parametrize('cid', PC.MULTI_ROW)
def test_the_inputs_tell_a_wrong_mixing_from_a_right_one(cid):
    c = PC.CASES[cid]
    inp = PC.case_inputs(cid)
    prof = PC.PROFILES[c['profile']]
    tabs = PC.oracle_case(cid)['tabs']
    good = PC.oracle_case(cid)['d0']
    scale = np.abs(good).max(axis=(1, 2, 3))
    # (the helper reproduces the case's oracle, so a movement is the mistake's)
    assert np.array_equal(_d0_rows(inp, c['dim'], tabs, inp['cn2']), good)
    worst = {}
    for name, (w, t) in _mistakes(inp, tabs, prof).items():
        bad = _d0_rows(inp, c['dim'], t, w)
        move = np.abs(bad - good).max(axis=(1, 2, 3)) / scale          # per row
        worst[name] = move
        # the mistake shows in the case (a kernel makes it in every row; one failing row fails the test) ...
        assert move.max() >= MOVE_MIN, (name, move)
        # ... and in row 0, whose weights all differ, by itself
        if name != 'row0_for_all':
            assert move[0] >= MOVE_MIN, (name, move)
    # rows 1 and 2 each tell their own weights from their neighbour's and from row 0's
    assert np.all(worst['next_row'] >= MOVE_MIN) and np.all(worst['row0_for_all'][1:] >= MOVE_MIN)
    print(cid, ' '.join('%s %.1e' % (k, v.max()) for k, v in worst.items()))


# ---- 5. fits are well-posed
@pytest.mark.parametrize('cid', [k for k, c in PC.CASES.items() if c['dim'] >= 512])
def test_the_oracle_fits_are_well_posed(cid):
    kap = PC.oracle_case(cid)['kappa']
    lim = PC.WELL_POSED_LIMIT[PC.CASES[cid]['dim']]
    print(cid, 'err_n peak / sqrt(chi2 / dof): max %.2f (limit %g)' % (kap.max(), lim))
    assert np.all(np.isfinite(kap)) and kap.max() < lim


def test_the_case_matrix_is_what_the_tests_assume():
    for cid, c in PC.CASES.items():
        inp = PC.case_inputs(cid)
        n = len(PC.PROFILES[c['profile']]['h'])
        assert inp['cn2'].shape == (len(c['rows']), n) and np.all(inp['cn2'].sum(axis=1) > 0)
        assert inp['dirs'].shape[0] == 2 and len(inp['lbda']) == 2
        assert O.npix_crop(inp['lbda'], 40, PC.grid_pixscale(c['dim'])).max() <= c['dim']
    assert len(PC.PX['h']) == 8 and max(PC.PX['h']) == 50000.0 and min(PC.PX['h']) == 0.0
    assert max(PC.PX['wind_speed']) == 100.0 and min(PC.PX['wind_speed']) == 0.0
    assert PC.POS25.shape == (25, 2) and np.abs(PC.POS25).max() == 60.0
    assert {(60.0, 60.0), (60.0, -60.0), (-60.0, 60.0), (-60.0, -60.0), (0.0, 0.0)} <= {tuple(p) for p in PC.POS25}
    assert len({tuple(p) for p in PC.POS25}) == 25
    # row 1 holds exact zeros in layers the others use, row 2 all its weight in one layer
    for w in (PC.W8, PC.W5, PC.W3):
        assert np.any((w[1] == 0) & (w[0] > 0)) and np.count_nonzero(w[2]) == 1 and np.all(w[0] > 0)
        assert np.all(w.sum(axis=0) > 0)                # no layer is dropped by the host
