"""CPU: band-integrated PSFs -- band_weights, the refusals of compute_band_psf / compute_psf_from_sparta(bands=...) /
Context.reconstruct_band before any GPU context exists or the library is called, the CLI's band grid, and the header
declarations the binding relies on."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from muse_psfr_amd import _lib, psfrec
from muse_psfr_amd.psfrec import band_weights, _band_columns

LB = np.arange(490.0, 931.0, 5.0)        # 89 wavelengths


@pytest.fixture
def no_context(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('a GPU context was requested before the arguments were checked')
    monkeypatch.setattr(psfrec, 'get_context', refuse)


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError('the library was called before the arguments were checked')


@pytest.fixture
def bare_context():
    ctx = object.__new__(_lib.Context)
    ctx.lib = _NoLib()
    ctx.dim, ctx.pixscale, ctx.dimpsf, ctx.precision = 512, 0.2, 40, 'mixed'
    ctx._pending = {}
    return ctx


# ---- band_weights
def test_full_top_hat_gives_the_trapezoid_weights():
    w = band_weights(LB, [(490.0, 930.0)])
    want = np.full(LB.size, 5.0)
    want[0] = want[-1] = 2.5
    assert w.shape == (1, LB.size)
    np.testing.assert_allclose(w[0], want, rtol=1e-14)
    # a sub-band with its edges on nodes: the trapezoid weights of its own nodes (edge nodes half an interval), zero
    # elsewhere; one band may be given bare
    w2 = band_weights(LB, (600.0, 700.0))
    inside = (LB >= 600) & (LB <= 700)
    want2 = np.where(inside, 5.0, 0.0)
    want2[LB == 600] = want2[LB == 700] = 2.5
    np.testing.assert_allclose(w2[0], want2, rtol=1e-14, atol=1e-14)
    # an edge between two nodes shares its interval linearly: [601, 604] lies in [600, 605]
    w3 = band_weights(LB, (601.0, 604.0))[0]
    assert np.all(w3[(LB < 600) | (LB > 605)] == 0)
    np.testing.assert_allclose(w3[(LB == 600) | (LB == 605)], [1.5, 1.5], rtol=1e-14)
    # a non-uniform grid: (d_{l-1} + d_l) / 2
    g = np.array([500.0, 510.0, 530.0, 560.0])
    np.testing.assert_allclose(band_weights(g, [(0.0, 1000.0)])[0], [5.0, 15.0, 25.0, 15.0], rtol=1e-14)


def test_disjoint_bands_on_a_union_grid_equal_each_band_alone():
    """A gap between two bands on one grid gives neither band weight: each band's normalised weights are those it has
    on its own grid (the CLI builds the union grid of several --band options)."""
    from muse_psfr_amd.cli import band_grid
    bands = [(500.0, 520.0), (800.0, 820.0), (600.0, 612.0)]
    grid = band_grid(bands, 5.0).astype(float)
    w = band_weights(grid, bands)
    for k, (lo, hi) in enumerate(bands):
        own = band_grid([(lo, hi)], 5.0).astype(float)
        alone = band_weights(own, [(lo, hi)])[0]
        full = np.zeros(grid.size)
        full[np.searchsorted(grid, own)] = alone / alone.sum()
        np.testing.assert_allclose(w[k] / w[k].sum(), full, rtol=1e-14, atol=1e-16)
    np.testing.assert_allclose(w[0] / w[0].sum(), [0.125, 0.25, 0.25, 0.25, 0.125] + [0.0] * (grid.size - 5),
                               rtol=1e-14, atol=1e-16)
    # the same for throughput curves that end inside the gap
    c0 = (np.array([500.0, 520.0]), np.array([1.0, 1.0]))
    np.testing.assert_allclose(band_weights(grid, [c0])[0], w[0], rtol=1e-14, atol=1e-16)


def test_curve_and_sed_multiply():
    curve = (np.array([550.0, 650.0, 750.0]), np.array([0.0, 2.0, 0.0]))
    sed = (np.array([400.0, 1000.0]), np.array([1.0, 3.0]))
    d = band_weights(LB, [(490.0, 930.0)])[0]
    t = np.interp(LB, curve[0], curve[1], left=0, right=0)
    f = np.interp(LB, sed[0], sed[1])
    w = band_weights(LB, [curve, (600.0, 700.0)], sed=sed)
    np.testing.assert_allclose(w[0], band_weights(LB, [curve])[0] * f, rtol=1e-15, atol=0)
    np.testing.assert_allclose(w[1], band_weights(LB, [(600.0, 700.0)])[0] * f, rtol=1e-15, atol=0)
    # where the throughput is linear across a node's two intervals the weight is the trapezoid one, D_l T(lbda_l)
    lin = (LB > 550) & (LB < 750) & (LB != 650)
    np.testing.assert_allclose(w[0][lin], (d * t * f)[lin], rtol=1e-13)
    # a throughput curve is zero outside its range
    assert np.all(w[0][(LB < 550) | (LB > 750)] == 0)
    # the weights are the integral of T times each node's hat function (a fine trapezoid sum here)
    xf = np.linspace(490.0, 930.0, 88001)
    tf = np.interp(xf, curve[0], curve[1], left=0, right=0)
    for l in (10, 20, 31, 40):
        hat = np.interp(xf, LB, np.eye(LB.size)[l])
        y = tf * hat
        ref = float(np.sum((y[1:] + y[:-1]) * np.diff(xf)) / 2)
        assert abs(band_weights(LB, [curve])[0][l] - ref) < 1e-5, l


def test_symmetric_band_has_its_centre_as_lbda_eff():
    for lo, hi in ((600.0, 700.0), (490.0, 930.0), (702.5, 802.5)):
        w = band_weights(LB, [(lo, hi)])
        eff, bmin, bmax = _band_columns(LB, w)
        assert abs(eff[0] - (lo + hi) / 2) < 1e-9
        # (an edge between two nodes gives weight to the node just outside it)
        assert bmin[0] == LB[LB <= lo][-1] and bmax[0] == LB[LB >= hi][0]
    tri = (np.array([600.0, 650.0, 700.0]), np.array([0.0, 1.0, 0.0]))
    assert abs(_band_columns(LB, band_weights(LB, [tri]))[0][0] - 650.0) < 1e-9


@pytest.mark.parametrize('lbda, bands, sed', [
    (np.array([500.0, 600.0, 590.0]), [(490.0, 930.0)], None),                 # not increasing
    (np.array([500.0, 600.0, 600.0]), [(490.0, 930.0)], None),                 # repeated node
    (np.array([600.0]), [(490.0, 930.0)], None),                               # one node
    (LB, [(940.0, 960.0)], None),                                              # no node in the band
    (LB, [(np.array([950.0, 960.0]), np.array([1.0, 1.0]))], None),            # curve beyond the grid
    (LB, [(700.0, 600.0)], None),                                              # lo > hi
    (LB, [(-10.0, 600.0)], None),                                              # negative lo
    (LB, [(np.array([500.0, 600.0]), np.array([1.0, -0.5]))], None),           # negative throughput
    (LB, [(600.0, 700.0)], (np.array([400.0, 1000.0]), np.array([1.0, -1.0]))),  # negative SED
    (LB, [(600.0, 700.0)], (np.array([650.0, 1000.0]), np.array([1.0, 1.0]))),   # SED misses 600..645
    (LB, [(600.0, 700.0)], (np.array([400.0, 690.0]), np.array([1.0, 1.0]))),    # SED misses 695..700
    (LB, [], None),                                                            # no band
    (LB, [(600.0, 700.0, 800.0)], None),                                       # not a pair
    (LB, [(np.array([600.0, 500.0]), np.array([1.0, 1.0]))], None),            # curve not increasing
])
def test_band_weights_refusals(lbda, bands, sed):
    with pytest.raises(ValueError):
        band_weights(lbda, bands, sed)


def test_sed_beyond_a_band_and_zero_bands_outside_it_are_accepted():
    sed = (np.array([590.0, 710.0]), np.array([1.0, 1.0]))
    w = band_weights(LB, [(600.0, 700.0)], sed=sed)
    np.testing.assert_array_equal(w, band_weights(LB, [(600.0, 700.0)]))


# ---- refusals before any context / library call
def test_compute_band_psf_refusals(no_context):
    good = dict(lbda=LB, seeing=1.0, GL=0.7, L0=25.0, bands=[(600.0, 700.0)])
    bad = [dict(bands=[(940.0, 960.0)]), dict(lbda=LB[::-1]), dict(seeing=-1.0), dict(GL=1.5), dict(L0=0.0),
           dict(h=(100, 1000, 10000)), dict(precision='f32'), dict(npsflin=0), dict(npsflin=6),
           dict(positions=[(70.0, 0.0)]), dict(positions=[(np.nan, 0.0)]), dict(circular=1),
           dict(sed=(np.array([650.0, 900.0]), np.array([1.0, 1.0])))]
    for kw in bad:
        args = dict(good, **kw)
        with pytest.raises(ValueError):
            psfrec.compute_band_psf(args.pop('lbda'), args.pop('seeing'), args.pop('GL'), args.pop('L0'),
                                    args.pop('bands'), verbose=False, **args)


def test_sparta_band_refusals(no_context):
    hdul = [psfrec._minifits.PrimaryHDU(), psfrec.create_sparta_table(nlines=2)]
    hdul = psfrec._minifits.HDUList(hdul)
    for kw in (dict(bands=[(940.0, 960.0)]), dict(bands=[(600.0, 700.0)], band_lbda=[700.0, 600.0]),
               dict(band_sed=(np.array([400.0, 1000.0]), np.array([1.0, 1.0]))), dict(band_lbda=LB),
               dict(bands=[(600.0, 700.0)], band_lbda=LB,
                    band_sed=(np.array([650.0, 900.0]), np.array([1.0, 1.0])))):
        with pytest.raises(ValueError):
            psfrec.compute_psf_from_sparta(hdul, verbose=False, **kw)


@pytest.mark.parametrize('weights', [
    np.zeros((0, 3)), np.ones((17, 3)), [[1.0, np.nan, 1.0]], [[1.0, -1.0, 1.0]], [[0.0, 0.0, 0.0]],
    [[1.0, 1.0]], [[np.inf, 1.0, 1.0]]])
def test_reconstruct_band_refusals(bare_context, weights):
    lb = np.array([500.0, 700.0, 900.0])
    with pytest.raises(ValueError):
        bare_context.reconstruct_band(lb, weights, [1.0], [0.7], [25.0])


def test_reconstruct_band_positions_take_the_default_npsflin(bare_context):
    """positions with npsflin left at its default pass the checks (the bare context's library is then reached)."""
    with pytest.raises(AssertionError, match='library was called'):
        bare_context.reconstruct_band(np.array([500.0, 700.0, 900.0]), np.ones((1, 3)), [1.0], [0.7], [25.0],
                                      positions=[(10.0, 0.0)])


def test_reconstruct_band_position_rules(bare_context):
    lb = np.array([500.0, 700.0, 900.0])
    w = np.ones((1, 3))
    for kw in (dict(npsflin=0), dict(npsflin=6), dict(npsflin=2, positions=[(0.0, 0.0)]),
               dict(npsflin=None, positions=np.zeros((26, 2))), dict(npsflin=0, positions=[(61.0, 0.0)])):
        with pytest.raises(ValueError):
            bare_context.reconstruct_band(lb, w, [1.0], [0.7], [25.0], **kw)


# ---- the CLI's band grid
def test_cli_band_grid():
    from muse_psfr_amd.cli import band_grid
    np.testing.assert_array_equal(band_grid([(500.0, 520.0)], 5.0), [500, 505, 510, 515, 520])
    np.testing.assert_array_equal(band_grid([(500.0, 512.0), (510.0, 520.0)], 5.0),
                                  [500, 505, 510, 512, 515, 520])


def test_cli_refuses_bad_bands():
    from muse_psfr_amd import cli
    for bad in (['--band', '700:600'], ['--band', '600'], ['--band', 'a:b'], ['--band', '600:700', '--band-step', '0']):
        with pytest.raises(SystemExit):
            cli.main(['--values', '1.0,0.7,25'] + bad)


# ---- header
def test_header_declares_the_band_call():
    import ctypes as C
    src = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    assert int(re.search(r'#define MPSFR_MAX_BANDS\s+(\d+)', src).group(1)) == _lib.MAX_BANDS == 16
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'int mpsfr_reconstruct_band\((.*?)\);', code, re.S)
    assert m, 'mpsfr_reconstruct_band is not declared'
    args = [a.strip() for a in m.group(1).split(',')]
    assert 'mpsfr_reconstruct_band' in _lib.EXPORTS
    argtypes = _lib.load().mpsfr_reconstruct_band.argtypes
    assert len(argtypes) == len(args) == 21
    ints = [k for k, a in enumerate(args) if re.match(r'int\s', a)]
    assert ints == [1, 8, 9, 11, 13, 20]
    assert all(argtypes[k] is C.c_int for k in ints)
    # nband precedes its [nband][nl] weights; the three outputs are the last pointers
    assert args[13].split()[-1] == 'nband' and args[14].split()[-1] == 'weights'
    assert [a.split()[-1] for a in args[17:20]] == ['band_out', 'band_sum_out', 'band_fit_out']
