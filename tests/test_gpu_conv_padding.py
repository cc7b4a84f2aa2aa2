"""GPU: the edges of k_conv_fft's zero padding and of its in-register mirror, through Context.convolve_stamps.

The 40-wide stamps sit on 64-wide frames, so a thread's line elements t + 8 e, e >= 5, are structurally zero (a first
pass that skips them was measured and not kept, profiles/conv_padding_rows.md; whichever form runs, these cases hold);
the float kernels pair spectrum element k with its mirror 64 - k by two DPP moves inside a slot's 8 lanes (lane 8 - t,
lane 0 its own register).  The stamps here are the ones that touch those edges first:

* all +0.0 and all -0.0 (x + 0.0 and x differ for x = -0.0 only): every output is zero and finite;
* zero except row 39 and column 39, the last line elements before the padding;
* a single row of ones, r in {0, 1, 38, 39} (both rows of the first and of the last packed pair), and a single column
  of ones, c in {0, 7, 8, 39} (lane 0's own-register case, lane 7, the second register of lane 0, the last column);
* eight different stamps convolved in one call and each alone: the bytes are the same (slots share waves).

A dim = 128 context at grid_pixscale(512), two tasks x 465 / 930 nm, both precisions.  Reference and bound are those of
tests/test_gpu_conv.py: the fp64 'same' convolutions of tests/tail_ref.py, 2e-5 (mixed) / 1e-9 (f64) of the peak of
the expected stamp.
"""
import numpy as np
import pytest

import tail_ref as T
from test_gpu_conv import TASKS, TOL, _errors

pytestmark = pytest.mark.gpu

LB = np.array([465.0, 930.0])
ROWS = (0, 1, 38, 39)
COLS = (0, 7, 8, 39)
_cache = {}


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _convolve(api, prec, par, pre, lb=LB):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(512), precision=prec)
    out = ctx.convolve_stamps(lb, par[:, 0], par[:, 1], par[:, 2], pre)
    ctx.close()
    return out


def line_stamps():
    """(name, stamp): the cross at 39, the single rows, the single columns"""
    cross = np.zeros((40, 40))
    cross[39, :] = 1.0
    cross[:, 39] = 1.0
    out = [('cross39', cross)]
    for r in ROWS:
        s = np.zeros((40, 40))
        s[r, :] = 1.0
        out.append(('row%d' % r, s))
    for c in COLS:
        s = np.zeros((40, 40))
        s[:, c] = 1.0
        out.append(('col%d' % c, s))
    return out


def _line_case(api):
    """inputs (class 2 i + j is stamp i with the parameters of TASKS[j]) and the fp64 reference, computed once"""
    if 'lines' not in _cache:
        classes = line_stamps()
        pre = np.array([np.broadcast_to(s, (LB.size, 40, 40)) for _, s in classes for _ in range(2)])
        par = np.tile(TASKS, (len(classes), 1))
        want = T.final_stamps(LB, par[:, 0], par[:, 1], par[:, 2], pre, api.grid_pixscale(512))
        _cache['lines'] = (classes, pre, par, want)
    return _cache['lines']


@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_zero_stamps_give_zero(api, prec):
    par = np.tile(TASKS, (2, 1))
    pre = np.zeros((4, LB.size, 40, 40))
    pre[2:] = -0.0
    assert not np.signbit(pre[:2]).any() and np.signbit(pre[2:]).all()
    got = _convolve(api, prec, par, pre)
    assert got.shape == pre.shape
    assert np.all(np.isfinite(got))
    assert np.all(got[:2] == 0.0), np.abs(got[:2]).max()
    assert np.all(got[2:] == 0.0), np.abs(got[2:]).max()


@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_last_row_and_column_before_the_padding(api, prec):
    classes, pre, par, want = _line_case(api)
    assert classes[0][0] == 'cross39'
    got = _convolve(api, prec, par[:2], pre[:2])
    assert np.all(np.isfinite(got))
    err = _errors(got, want[:2])
    print('cross39 %s: worst %.3e' % (prec, err.max()))
    assert err.max() < TOL[prec], err


@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_single_rows_and_columns_reach_every_mirror_lane(api, prec):
    classes, pre, par, want = _line_case(api)
    got = _convolve(api, prec, par, pre)
    assert np.all(np.isfinite(got))
    err = _errors(got, want)
    bad = []
    for k, (name, _) in enumerate(classes):
        e = err[2 * k:2 * k + 2].max()
        print('%s %s: worst %.3e' % (name, prec, e))
        if not e < TOL[prec]:
            bad.append((name, e))
    assert not bad, bad


@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_a_stamp_does_not_depend_on_its_neighbours(api, prec):
    """four tasks x two wavelengths = 8 stamps in one call, and each of them in a call of its own: the same bytes"""
    rng = np.random.default_rng(44)
    pre = rng.random((4, LB.size, 40, 40)) - 0.25
    pre[1, 0, :, 39] = 3.0          # something at the edges the slots share
    pre[2, 1, 39, :] = -2.0
    par = np.array([TASKS[0], TASKS[1], (1.1, 0.5, 15.0), (0.4, 0.3, 28.0)])
    together = _convolve(api, prec, par, pre)
    assert np.all(np.isfinite(together)) and np.abs(together).max() > 0
    bad = []
    for k in range(4):
        for l in range(LB.size):
            alone = _convolve(api, prec, par[k:k + 1], pre[k:k + 1, l:l + 1], lb=LB[l:l + 1])
            assert alone.shape == (1, 1, 40, 40) and alone.dtype == together.dtype
            if alone[0, 0].tobytes() != np.ascontiguousarray(together[k, l]).tobytes():
                bad.append((k, l, int((alone[0, 0] != together[k, l]).sum())))
    assert not bad, ('(task, wavelength, elements that differ)', bad)
