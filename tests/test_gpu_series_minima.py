"""GPU: the line minima of stage A's series form (K_DPHI_SERIES, stage_a2.hip) against the plane it stored.

While a line's values are in registers the kernel takes the minimum of max(D, 0) over each block of 32 columns
(debug fetch `dlin`, [task][dir][dim/2+1][dim/32]); the per-wavelength stage prunes on them.  The yardstick
is the stored plane (debug fetch `dphi0`) reduced by NumPy, never the kernel's own minima, and the comparison
is exact: a minimum rounds nothing (in f64 mode the kernel rounds each value DOWN to float first, so the
expected value is the largest float not above the minimum).

A line is cut into pieces of L columns (L = 16 up to 256^2, 32 at 512^2, 64 above); a piece where the
telescope OTF is identically zero is neither evaluated nor stored (`dphi0` is 0 there) and does not enter a
minimum: a block none of whose pieces is kept holds a value >= 3e38, a block that straddles the edge of the
support (L = 16: two pieces per block) the minimum over its kept piece alone.

The cases are the smallest that reach every lane layout of the kernel and a ragged last unit (a wave takes
64 / L lines at a time): 256^2 with four directions and 5 rows (L = 16, four lines per wave), 512^2 with
3 rows (two lines per wave, the last unit half empty), 1024^2 with one row and 1280^2 with 2 rows (one line per
wave; 16 and 20 pieces), two wavelengths each; mixed precision everywhere, f64 at 256^2 and 512^2.
"""
import numpy as np
import pytest

from conftest import H

pytestmark = pytest.mark.gpu

LANES = {256: 16, 512: 32, 1024: 64, 1280: 64}          # series_lanes() of stage_a2.hip
CASES = [(256, 2, 5, 'mixed'), (256, 2, 5, 'f64'), (512, 1, 3, 'mixed'), (512, 1, 3, 'f64'),
         (1024, 1, 1, 'mixed'), (1280, 1, 2, 'mixed')]  # dim, npsflin, rows, precision


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _round_down_to_float(v):
    f = v.astype(np.float32)
    up = f.astype(np.float64) > v
    f[up] = np.nextafter(f[up], np.float32(-np.inf))
    return f.astype(np.float64)


@pytest.mark.parametrize('dim,npl,rows,prec', CASES)
def test_line_minima_equal_the_minima_of_the_stored_plane(api, dim, npl, rows, prec):
    ps = api.grid_pixscale(dim)
    lb = np.array([490.0, 930.0]) if dim == 1280 else np.array([465.0, 930.0])
    ndir, h1, L = npl * npl, dim // 2 + 1, LANES[dim]
    see = np.linspace(0.5, 1.1, rows)
    gl = np.linspace(0.9, 0.5, rows)
    l0 = np.linspace(9.0, 25.0, rows)
    three = (np.arange(rows) % 2).astype(np.uint8)
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    ctx.set_option('stage_a', 2)
    ctx.reconstruct(lb, see, gl, l0, three, H, npsflin=npl)
    d0 = ctx.debug_fetch('dphi0', (rows, ndir, h1, dim))
    dlin = ctx.debug_fetch('dlin', (rows, ndir, h1, dim // 32))
    tel = ctx.debug_fetch('tel', (h1, dim))
    ctx.close()

    kept_piece = (tel.reshape(h1, dim // L, L) > 0).any(axis=-1)          # [line][piece]
    kept = np.repeat(kept_piece, L, axis=1)                               # [line][column]
    assert np.all(d0[:, :, ~kept] == 0)                                   # a skipped piece is never stored
    v = np.maximum(d0, 0.0)
    if prec == 'f64':
        v = _round_down_to_float(v)
    v = np.where(kept, v, np.inf)
    want = v.reshape(rows, ndir, h1, dim // 32, 32).min(axis=-1)
    some = kept.reshape(h1, dim // 32, 32).any(axis=-1)                   # blocks with a kept piece
    every = kept.reshape(h1, dim // 32, 32).all(axis=-1)
    assert some.any() and (~some).any()                                   # both kinds of block occur
    if L < 32:
        assert (some & ~every).any()                                      # and blocks that straddle the edge
    n_bad = int(np.sum(dlin[:, :, some] != want[:, :, some]))
    print('dim %d %s: %d blocks compared, %d differ; %d blocks outside the support' % (
        dim, prec, rows * ndir * int(some.sum()), n_bad, rows * ndir * int((~some).sum())))
    assert n_bad == 0
    assert np.all(dlin[:, :, ~some] >= 3e38)
