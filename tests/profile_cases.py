"""Shared cases of the Cn2-profile tests (tests/test_profile_oracle_host.py on the CPU, tests/test_gpu_profile_oracle.py
on the GPU): profiles, rows, positions, the case matrix, and the fp64 oracle of a case.  No GPU code.

The oracle (oracle/psfr_oracle.py, extended to per-layer winds and arbitrary directions) is the yardstick of every case;
the CPU tests hold it to the reference's goldens a-d, to a long-double evaluation on the profile at the header's limits,
and show that the inputs below tell a wrong mixing from a right one.

Profiles.  P8 is B8 of tests/test_gpu_profile.py (0 ... 18 000 m), P5 / P3 / P1 have 5 / 3 / 1 layers, PX has 8 layers at
the limits include/mpsfr.h grants: altitudes 0 and 50 000 m (twice), speeds 0 and 100 m/s (twice each, a layer with no
wind at altitude, a layer with the fastest wind at the top), directions of any size and sign (pi and -pi, 7 pi, 1000 rad).

Rows.  Three per multi-row case: 4-LGS, 3-LGS, 4-LGS; seeing, ground-layer fraction (the tip-tilt kernel's only) and L0
differ.  Row 0's weights alternate large and small, row 1 holds exact zeros in layers the others use and does not sum to
1 (the library normalises per row, psfrec.py:57-58), row 2 holds all its weight in one layer.  The rows were chosen so
that the oracle's own Moffat fits are well-posed on every grid from 512^2 on (test_profile_oracle_host.py asserts it).
"""
import numpy as np

import psfr_oracle as O
from muse_psfr_amd.synthetic import grid_pixscale

PI = np.pi

P8 = dict(h=[0.0, 300.0, 1000.0, 2500.0, 5000.0, 9000.0, 13000.0, 18000.0],
          wind_speed=[5.0, 8.0, 10.0, 14.0, 20.0, 30.0, 25.0, 12.0],
          wind_dir=[0.0, 0.4, -0.8, 1.2, 2.5, -2.0, 3.0, -0.3])
P5 = dict(h=[0.0, 500.0, 2000.0, 6000.0, 14000.0], wind_speed=[6.0, 9.0, 15.0, 28.0, 18.0],
          wind_dir=[0.2, -0.9, 1.7, 2.8, -2.2])
P3 = dict(h=[0.0, 1000.0, 10000.0], wind_speed=[8.0, 15.0, 30.0], wind_dir=[0.3, -1.0, 2.0])
P1 = dict(h=[0.0], wind_speed=[10.0], wind_dir=[1.2])
PX = dict(h=[0.0, 50000.0, 17.0, 25000.5, 50000.0, 3000.0, 1.0, 12345.678],
          wind_speed=[0.0, 100.0, 100.0, 0.0, 37.3, 1e-3, 99.9, 50.0],
          wind_dir=[0.0, PI, -PI, 7 * PI, 1000.0, -2.5, PI / 2, 1.0])
PROFILES = {'P8': P8, 'P5': P5, 'P3': P3, 'P1': P1, 'PX': PX}

# per-row weights [row][layer], as handed to the library (not normalised)
W8 = np.array([[0.45, 0.05, 0.15, 0.03, 0.12, 0.02, 0.14, 0.04],
               [0.90, 0.00, 0.75, 0.00, 0.15, 0.60, 0.00, 0.60],
               [0.00, 0.00, 1.00, 0.00, 0.00, 0.00, 0.00, 0.00]])
W5 = np.array([[0.40, 0.05, 0.30, 0.05, 0.20],
               [1.00, 0.00, 0.20, 0.80, 0.00],
               [0.00, 0.00, 1.00, 0.00, 0.00]])
W3 = np.array([[0.60, 0.10, 0.30],
               [0.50, 0.00, 1.50],
               [0.00, 1.00, 0.00]])
W1 = np.array([[1.0]])
WEIGHTS = {'P8': W8, 'P5': W5, 'P3': W3, 'P1': W1, 'PX': W8}

# rows: seeing [arcsec], ground-layer fraction, L0 [m], three-laser mode
SEE = np.array([0.6, 0.9, 0.75])
GL = np.array([0.7, 0.9, 0.8])
L0 = np.array([16.0, 9.0, 24.0])
THREE = np.array([0, 1, 0], np.uint8)

# positions [npos][2] arcsec
POS5 = np.array([(0.0, 0.0), (30.0, 0.0), (-30.0, 0.0), (0.0, 45.0), (-50.0, -50.0)])      # golden case d
POS2 = np.array([(0.0, 0.0), (37.0, -52.0)])


def _pos25():
    rng = np.random.default_rng(25)
    fixed = [(60.0, 60.0), (60.0, -60.0), (-60.0, 60.0), (-60.0, -60.0), (0.0, 0.0)]
    rest = np.round(rng.uniform(-60.0, 60.0, (20, 2)), 3)
    return np.concatenate([np.array(fixed), rest])


POS25 = _pos25()


def lbda(dim):
    """Two wavelengths per case, the ends of the range the grid can run (tests/test_gpu_series_hermitian.py)."""
    return np.array([490.0, 930.0]) if dim == 1280 else np.array([465.0, 930.0])


def _case(dim, form, profile, rows=(0, 1, 2), stage_a=1, npsflin=1, positions=None, l0=None):
    return dict(dim=dim, form=form, profile=profile, rows=tuple(rows), stage_a=stage_a, npsflin=npsflin,
                positions=positions, l0=l0)


# id -> case: grid, the form of stage A it must take, profile, rows; how the form is chosen -- stage_a: the option
# (0 full-size, 1 automatic, 2 series), npsflin or positions (several directions: series from 256^2 on), l0: per-row
# override of L0 (a row below 7 m: full-size).  Two wavelengths; one row, one direction on 1024^2 and 1280^2.
CASES = {
    'F1': _case(128, 'full', 'P8'),
    'F2': _case(256, 'full', 'P3'),
    'F3': _case(512, 'full', 'P8', l0=(16.0, 5.0, 24.0)),
    'F4': _case(1024, 'full', 'P5', rows=(0,), stage_a=0),
    'F5': _case(1280, 'full', 'P8', rows=(0,), stage_a=0),
    'S1': _case(128, 'series', 'P8', stage_a=2),
    'S2': _case(256, 'series', 'P3', npsflin=2),
    'S3': _case(512, 'series', 'P8', positions=POS5),
    'S4': _case(1024, 'series', 'P1', rows=(0,)),
    'S5': _case(1280, 'series', 'P8', rows=(0,)),
    # (two positions are two directions, and from two directions on a 256^2 call takes the series form by itself: the
    # full-size form has to be asked for here)
    'X1': _case(256, 'full', 'PX', positions=POS2, stage_a=0),
    'X2': _case(512, 'series', 'PX', positions=POS2),
}
MULTI_ROW = [k for k, c in CASES.items() if len(c['rows']) > 1]

# Well-posedness of a Moffat fit: err_n * peak / sqrt(chi2 / dof) of the oracle's own fit, the limits per grid of
# tests/test_gpu_series_hermitian.py (the kernel flags a fit from 100 on, include/mpsfr.h).  1024^2 has none there: the
# number grows with the pixel scale (a PSF of fewer pixels pins n less), 5 at 0.076 arcsec (512^2) and 14 at 0.2 arcsec
# (1280^2), i.e. as pixel scale^1.06; grid_pixscale(1024) = 0.152 arcsec gives 5 * 2^1.06 = 10.4, rounded up to 11.
WELL_POSED_LIMIT = {512: 5.0, 1024: 11.0, 1280: 14.0}


def case_inputs(cid):
    """What a case hands to reconstruct_profile: dict(lbda, seeing, gl, l0, three, cn2, h, wind_speed, wind_dir,
    dirs ([2][ndir] arcsec, what the oracle evaluates), kw (npsflin= or positions=))."""
    c = CASES[cid]
    rows = list(c['rows'])
    prof = PROFILES[c['profile']]
    l0 = np.array(c['l0'] if c['l0'] is not None else L0)[rows]
    if c['positions'] is not None:
        dirs, kw = np.asarray(c['positions']).T, dict(positions=c['positions'])
    else:
        dirs, kw = O.eval_directions(c['npsflin']), dict(npsflin=c['npsflin'])
    return dict(lbda=lbda(c['dim']), seeing=SEE[rows], gl=GL[rows], l0=l0, three=THREE[rows],
                cn2=WEIGHTS[c['profile']][rows], dirs=dirs, kw=kw, **prof)


def oracle_tables(prof, dirs):
    """{geometry: (T[layer][dir][80][80], noise[dir][80][80])} of a profile at the directions `dirs` ([2][ndir])."""
    return {g: O.ao_tables(prof['h'], bool(g), 1, exact_masks=True, wind_speed=prof['wind_speed'],
                           wind_dir=prof['wind_dir'], directions=dirs) for g in (0, 1)}


def oracle_d0(psd):
    """Structure functions of PSDs [dir][dim][dim] in the library's layout [dir][y <= dim/2][x]."""
    dim = psd.shape[-1]
    d = np.array([O.structure_function0(p) for p in psd])
    return np.swapaxes(d, -1, -2)[:, :dim // 2 + 1, :]


def oracle_rows(inp, dim, tabs, fit=True):
    """The oracle of rows `inp` (case_inputs, or the same keys) on a grid: dict(d0 [row][dir][dim/2 + 1][dim],
    pre, fin ([row][nl][40][40] for the averaged npsflin grid, [row][npos][nl][40][40] for positions),
    fit (the same leading shape x 5; None without `fit`), kappa (well-posedness number of every fit))."""
    ps = grid_pixscale(dim)
    lb = inp['lbda']
    field = 'positions' in inp['kw']
    out = dict(d0=[], pre=[], fin=[], fit=[], kappa=[])
    for s, g, l, th, w in zip(inp['seeing'], inp['gl'], inp['l0'], inp['three'], inp['cn2']):
        psd = O.residual_psd(w, inp['h'], s, l, 1, dim, bool(th), tables=tabs[int(th)])
        out['d0'].append(oracle_d0(psd))
        groups = [p for p in psd] if field else [psd]
        pre = [O.psf_stamps_refshaped(p, lb, 40, ps) for p in groups]
        fin = [O.convolve_final_psf(lb, s, g, l, p, ps) for p in pre]
        out['pre'].append(pre if field else pre[0])
        out['fin'].append(fin if field else fin[0])
        if fit:
            fits = [[O.moffat_fit(f, ps, errors=True) for f in stamps] for stamps in fin]
            cols = [[[e['peak'], e['center'][0], e['center'][1], e['fwhm'], e['n']] for e in ff] for ff in fits]
            kap = [[e['err_n'] * e['peak'] / np.sqrt(e['chi2'] / e['dof']) for e in ff] for ff in fits]
            out['fit'].append(cols if field else cols[0])
            out['kappa'].append(kap if field else kap[0])
    return {k: (np.array(v) if len(v) else None) for k, v in out.items()}


_cache = {}


def oracle_case(cid):
    """The oracle of a case of the matrix, computed once: dict(tabs, d0, pre, fin, fit, kappa)."""
    c = CASES[cid]
    inp = case_inputs(cid)
    key = (c['dim'], c['profile'], c['rows'], tuple(inp['l0']), 'positions' in inp['kw'],
           inp['dirs'].tobytes())                                                       # (the form is no input)
    if key not in _cache:
        tabs = oracle_tables(PROFILES[c['profile']], inp['dirs'])
        _cache[key] = dict(tabs=tabs, **oracle_rows(inp, c['dim'], tabs))
    return _cache[key]
