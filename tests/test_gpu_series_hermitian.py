"""GPU: the Hermitian fold of stage A's series form (stage_a2.hip) against the CPU oracle.

K_PATCH_ROWS stores the Hermitian half of every line of the patch's row transforms (41 values, the edge
row su = -40 as its own pair) and K_DPHI_SERIES folds it into the classes r = 0 .. Q/2 and finishes with a
complex-to-real transform in registers.  One small call (2 rows x 2 wavelengths) per in-lane transform:

  128^2, series form forced : Q = 8, the smallest transform (edge term in class 0)
  256^2, npsflin = 2        : Q = 16, several directions share a patch generation
  512^2                     : Q = 16, two lines per wave, edge term in class Q/2
  1280^2                    : Q = 20, radix 5, edge term in class 0

in both precisions.  The structure function (debug fetch `dphi0`) is held against the oracle at the
tolerances of the stage-level parity test (1e-12 of its maximum in f64 mode, 2e-7 in mixed mode, on the
support of the telescope OTF), the final stamps at 1e-9 / 2e-5 of their maximum and the final Moffat fit
columns (fwhm in arcsec, beta) at 1e-6 / 1e-4 against the oracle's fit of its own stamps, as there, on
every grid.

The rows.  On 128^2 / 256^2 the 40 px stamp can be narrower than the PSF core, and then (fwhm, beta) are not
pinned to 1e-4 by stamps known to a few 1e-7 of their peak; the fit kernel flags such fits
(MPSFR_FIT_ILL_CONDITIONED: n^2 sqrt(cov) peak >= 100, test_gpu_parity.py).  The two rows below are chosen
from the oracle alone -- its own fit gives that sensitivity as err_n peak / sqrt(chi2 / dof) < 7 at
128^2, < 5 at 256^2 and 512^2 and < 14 at 1280^2 -- so that every fit of every grid is
well-conditioned: the test asserts that no fit is flagged and compares all of them.  They cover both laser
geometries and outer scales near the edge of the expansion in 1/L0^2 (9 m) and inside it (22 m).
"""
import numpy as np
import pytest

import psfr_oracle as O
from conftest import H, rel_err

pytestmark = pytest.mark.gpu

EPS_D = {'f64': 1e-12, 'mixed': 2e-7}
TOL_FIT = {'f64': 1e-6, 'mixed': 1e-4}
TOL_STAMP = {'f64': 1e-9, 'mixed': 2e-5}         # of the stamp maximum (test_gpu_parity.py)

SEE = np.array([0.5, 0.55])
GL = np.array([0.9, 0.92])
L0 = np.array([9.0, 22.0])
THREE = np.array([0, 1], np.uint8)

CASES = [(128, 1, 2), (256, 2, 1), (512, 1, 1), (1280, 1, 1)]          # dim, npsflin, stage_a option


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


_oracle_cache = {}


def _oracle(api, dim, npl, l0):
    """Structure functions [task][dir][y][x], final stamps and their fits of the oracle, once per grid."""
    key = (dim, npl, tuple(l0))
    if key not in _oracle_cache:
        ps = api.grid_pixscale(dim)
        lb = _lbda(dim)
        tabs = {g: O.ao_tables(H, bool(g), npl, exact_masks=True) for g in (0, 1)}
        d0, fin, fit = [], [], []
        for s, g, l, th in zip(SEE, GL, l0, THREE):
            psd = O.residual_psd([g, 1 - g], H, s, l, npl, dim, bool(th), tables=tabs[int(th)])
            od = np.array([O.structure_function0(p) for p in psd])
            d0.append(np.swapaxes(od, -1, -2)[:, :dim // 2 + 1, :])
            fin.append(O.convolve_final_psf(lb, s, g, l, O.psf_stamps_refshaped(psd, lb, 40, ps), ps))
            fit.append(O.fit_psf_cube(fin[-1], ps))
        _oracle_cache[key] = (np.array(d0), np.array(fin), np.array(fit))
    return _oracle_cache[key]


def _lbda(dim):
    return np.array([490.0, 930.0]) if dim == 1280 else np.array([465.0, 930.0])


def _check_d0(d0, od0, tel, eps):
    worst = 0.0
    for k in range(d0.shape[0]):
        inside = np.broadcast_to(tel > 0, d0[k].shape)
        scale = np.abs(od0[k]).max()
        worst = max(worst, np.abs(d0[k] - od0[k])[inside].max() / scale)
        out = d0[k][~inside]        # whole pieces of a line outside the support are skipped, the others computed
        assert np.all((out == 0) | (np.abs(out - od0[k][~inside]) / scale < eps))
    print('dphi0 vs oracle: %.3e (bound %.1e)' % (worst, eps))
    assert worst < eps


def _check_stamps_and_fits(r, ofin, ofit, ps, prec):
    fit = np.asarray(r['fit'])
    assert np.all(fit[..., 14] == 0)                    # no fit is ill-conditioned: all of them are compared
    e_stamp = max(rel_err(np.asarray(r['psf'][k], float), ofin[k]) for k in range(len(ofin)))
    e_fwhm = np.abs(fit[..., 5] * ps - ofit[..., 3]).max()
    e_beta = np.abs(fit[..., 4] - ofit[..., 4]).max()
    print('stamps vs oracle: %.3e (bound %.1e); fit: fwhm %.3e beta %.3e (bound %.1e)' % (
        e_stamp, TOL_STAMP[prec], e_fwhm, e_beta, TOL_FIT[prec]))
    assert e_stamp < TOL_STAMP[prec]
    assert e_fwhm < TOL_FIT[prec]
    assert e_beta < TOL_FIT[prec]


@pytest.mark.parametrize('prec', ['f64', 'mixed'])
@pytest.mark.parametrize('dim,npl,stage_a', CASES)
def test_hermitian_fold_against_the_oracle(api, dim, npl, stage_a, prec):
    ps = api.grid_pixscale(dim)
    lb = _lbda(dim)
    ndir = npl * npl
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    ctx.set_option('stage_a', stage_a)
    r = ctx.reconstruct(lb, SEE, GL, L0, THREE, H, npsflin=npl)
    d0 = ctx.debug_fetch('dphi0', (SEE.size, ndir, dim // 2 + 1, dim))
    tel = ctx.debug_fetch('tel', (dim // 2 + 1, dim))
    # The series form did run.  From 256^2 on it leaves whole pieces of a line outside the telescope's support
    # untouched; on the small grids, where it is not the default everywhere, its structure function must also differ
    # in some bit from that of the full-size transforms (two summation orders; fp32 series terms in mixed mode).
    if dim >= 256:
        assert np.any(np.all(d0 == 0, axis=(0, 1)) & ~(tel > 0))
    if dim < 512:
        ctx.set_option('stage_a', 0)
        ctx.reconstruct(lb, SEE, GL, L0, THREE, H, npsflin=npl)
        d0_full = ctx.debug_fetch('dphi0', (SEE.size, ndir, dim // 2 + 1, dim))
        assert not np.array_equal(d0, d0_full)
    ctx.close()
    od0, ofin, ofit = _oracle(api, dim, npl, L0)
    _check_d0(d0, od0, tel, EPS_D[prec])
    _check_stamps_and_fits(r, ofin, ofit, ps, prec)


@pytest.mark.parametrize('prec', ['f64', 'mixed'])
def test_short_outer_scale_still_takes_the_full_size_form(api, prec):
    """A task with L0 < 7 m lies outside the expansion of the fitting term: the call takes the full-size
    transforms by itself -- bit for bit what the option stage_a = 0 gives -- and agrees with the oracle."""
    dim = 512
    ps = api.grid_pixscale(dim)
    lb = _lbda(dim)
    l0 = np.array([25.0, 5.0])
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    r = ctx.reconstruct(lb, SEE, GL, l0, THREE, H, npsflin=1)
    d0 = ctx.debug_fetch('dphi0', (SEE.size, 1, dim // 2 + 1, dim))
    tel = ctx.debug_fetch('tel', (dim // 2 + 1, dim))
    ctx.close()
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    ctx.set_option('stage_a', 0)
    r0 = ctx.reconstruct(lb, SEE, GL, l0, THREE, H, npsflin=1)
    d00 = ctx.debug_fetch('dphi0', (SEE.size, 1, dim // 2 + 1, dim))
    ctx.close()
    np.testing.assert_array_equal(d0, d00)
    np.testing.assert_array_equal(r['psf'], r0['psf'])
    od0, ofin, ofit = _oracle(api, dim, 1, l0)
    _check_d0(d0, od0, tel, EPS_D[prec])
    _check_stamps_and_fits(r, ofin, ofit, ps, prec)
