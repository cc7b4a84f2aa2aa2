"""The fp64 yardstick of psd_to_psf (tests/psd_to_psf_ref.py) without a GPU: against the reference's values (g8)
and the oracle, against a long-double evaluation that shares no FFT call with it, and a check that the inputs
of tests/test_gpu_psd_to_psf_inputs.py tell a right answer from the wrong ones a kernel could give."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import psfr_oracle as O
import psd_to_psf_ref as R

TOL = 1e-10                 # the GPU tests' bound, of the peak (tests/test_gpu_psd_to_psf.py)
# The yardstick's own error, of the peak.  Five fp64 transforms of 128 or 256 points per axis: a few hundred eps at
# most, and 1e-13 leaves the GPU bound a factor 1000 above the yardstick.  On a PSD scaled to a large exponent
# ("rung": the largest (1/2)(2 pi / lambda_nm)^2 Dphi0 of the window) the operation itself is ill-conditioned: the
# exponent of every lag is c (dc - Re(...)), both terms of the size of the rung and each carrying a few eps of its
# transform, so the exponent is off by up to 8 eps rung in absolute terms -- which is the relative error of the
# system OTF, and so of the PSF against its peak, in any fp64 evaluation, the kernels' included.
YARDSTICK_TOL = 1e-13


def _yardstick_tol(rung):
    return max(YARDSTICK_TOL, 8 * np.finfo(np.float64).eps * rung)
D = 8.0
LB = 500e-9


def _rel(got, want, peak=None):
    peak = np.abs(want).max() if peak is None else peak
    return float(np.abs(got - want).max() / peak)


def test_plan_table_equals_the_header():
    """PLAN names the threads per line and the lines per workgroup the GPU tests place their pupil sizes round."""
    with open(os.path.join(ROOT, 'muse_psfr_amd', 'csrc', 'fft_lds.h')) as fh:
        text = fh.read()
    macros = dict(re.findall(r'#define (MPSFR_SLOTS\d+) (\d+)', text))
    for m, want in R.PLAN.items():
        body = re.search(r'struct Plan<%d> \{.*?TPR = (\d+), SLOTS = (\w+);' % m, text, re.S)
        assert body, m
        slots = body.group(2)
        assert (int(body.group(1)), int(macros.get(slots, slots))) == (want['TPR'], want['SLOTS']), m


def _fixture_psd(g, name):
    quad, centre = g[name + '_quad'], g[name + '_centre']
    h, c = quad.shape[0], centre.shape[0] // 2
    full = np.block([[quad, quad[:, ::-1]], [quad[::-1], quad[::-1, ::-1]]])
    full[h - c:h + c, h - c:h + c] = centre
    return full.astype(np.float64)


def _crop(p, c):
    n = p.shape[-1]
    return p[..., n // 2 - c:n // 2 + c, n // 2 - c:n // 2 + c]


def test_equals_the_reference_values(golden):
    """Cases a to d of g8 in the quantities of test_gpu_psd_to_psf.py::test_cases_equal_the_reference, at its
    bound: b is the static phase, c the dimnum < dim branch, d the apodised pupil with spiders."""
    g = golden('g8_psd_to_psf')
    lb = g['lbda']
    c = int(g['crop'])
    pup = g['pup_muse256'].astype(float)
    psd = _fixture_psd(g, 'psd256')
    a = R.psd_to_psf_ref(psd, pup, D, lb)
    worst = {'a': _rel(a[:, :129], g['psf_a_half'])}

    def crops(case, p):
        peak = g['peak_' + case].max()
        worst[case] = max(_rel(_crop(p, c), g['crop_' + case], peak), _rel(p.sum(axis=2), g['rows_' + case], peak),
                          _rel(p.sum(axis=1), g['cols_' + case], peak))
    b = R.psd_to_psf_ref(psd, pup, D, lb, phase_static=g['phase_b'].astype(float))
    crops('b', b)
    diff = np.abs(b - a).max()
    assert abs(diff - g['maxdiff_ab']) <= TOL * (a.max() + g['peak_b'].max())
    psd5 = _fixture_psd(g, 'psd512')
    for case, pup_ in (('c', g['pup_c'].astype(float)), ('d', g['pup_d_4096'] / 4096.0)):
        n = int(g['dimnum_' + case])
        p = R.psd_to_psf_ref(psd5, pup_, D, lb, dimnum=n)
        assert p.shape == (2, n, n)
        crops(case, p)
    assert int(g['dimnum_c']) == 256 and int(g['dimnum_d']) == 512
    print('yardstick against g8:', worst)
    assert max(worst.values()) <= TOL, worst


def test_equals_the_oracle_at_256():
    pup = R.rand_pupil(128)
    psd = R.scaled_psd(R.asym_psd(256), pup, O.DPUP, LB, 256, 10.0)
    err = _rel(R.psd_to_psf_ref(psd, pup, O.DPUP, LB), O.psd_to_psf_refshaped(psd, pup, LB))
    print('yardstick against the oracle:', err)
    assert err <= YARDSTICK_TOL


def _harsh_cases():
    """dimnum 128: the harshest inputs of the GPU tests.  name -> (psd, pup, phase, rung)."""
    pup = R.rand_pupil(37)
    pup61 = R.rand_pupil(61)
    asym256 = R.asym_psd(256)
    asym = R.asym_psd(128)
    ph30 = R.rand_phase(37, 30.0, LB)
    full = R.rand_pupil(128, seed=5)
    lpup = R.l_pupil_with_huge_phase(37, LB)
    return {
        'asym': (R.scaled_psd(asym, pup, D, LB, 128, 10.0), pup, None, 10.0),
        'asym_phase30': (R.scaled_psd(asym, pup, D, LB, 128, 10.0), pup, ph30, 10.0),
        'scale_700': (R.scaled_psd(asym, pup, D, LB, 128, 700.0), pup, None, 700.0),
        'scale_1e5_phase30': (R.scaled_psd(asym, pup, D, LB, 128, 1e5), pup, ph30, 1e5),     # the largest rung
        # the ladder of the GPU tests where it measured most: the window of 128 cut from 256
        'window_scale_50': (R.scaled_psd(asym256, pup61, D, LB, 128, 50.0), pup61, None, 50.0),
        'window_scale_700': (R.scaled_psd(asym256, pup61, D, LB, 128, 700.0), pup61, None, 700.0),
        'window_scale_800': (R.scaled_psd(asym256, pup61, D, LB, 128, 800.0), pup61, None, 800.0),
        'signed': (R.scaled_psd(R.signed_psd(128), pup, D, LB, 128, 20.0), pup, None, 20.0),
        'ridge': (R.scaled_psd(R.ridge_psd(128), pup, D, LB, 128, 10.0), pup, ph30, 10.0),
        'npup_is_dimnum': (R.scaled_psd(asym, full, D, LB, 128, 10.0), full, R.rand_phase(128, 30.0, LB), 10.0),
        'zero_psd_l_pupil': (np.zeros((128, 128)), lpup[0], lpup[1], 0.0),
        'negative_sum': (R.scaled_psd(asym, pup, D, LB, 128, 10.0), R.rand_pupil(37, lo=-1.0, hi=0.2), ph30, 10.0),
    }


def test_against_the_long_double_evaluation():
    """The yardstick's own error: worst max |diff| / peak against explicit long-double DFTs.  The figure is kept
    in profiles/psd_to_psf_margins.json ("yardstick_vs_long_double"); the GPU figures are read against it."""
    worst, over = {}, {}
    for name, (psd, pup, ph, rung) in _harsh_cases().items():
        want = R.psd_to_psf_longdouble(psd, pup, D, LB, ph, 128)
        assert np.isfinite(want).all(), name
        worst[name] = _rel(R.psd_to_psf_ref(psd, pup, D, LB, ph, 128), want.astype(np.float64))
        over[name] = worst[name] / _yardstick_tol(rung)
    print('yardstick against long double:', worst)
    assert max(over.values()) <= 1, (worst, over)


@pytest.mark.parametrize('dim,dimnum,npup', [(128, 128, 37), (256, 128, 61), (1280, 1024, 500), (1280, 1280, 333)])
def test_the_inputs_discriminate(dim, dimnum, npup):
    """A kernel that transposed or mirrored an input, read the window one sample off or took the phase in nm
    would be 1000 tolerances or more off the yardstick on the asymmetric inputs of the GPU tests.  (The sign of
    the phase and the place of the pupil inside the padded array cannot be seen: the modulus of the OTF removes
    both, in the reference as here.)"""
    pup = R.rand_pupil(npup)
    ph = R.rand_phase(npup, 2 * np.pi * 1e-7 / LB, LB)              # 1e-7 m
    psd = R.scaled_psd(R.asym_psd(dim), pup, D, LB, dimnum, 10.0)
    ridge = R.scaled_psd(R.ridge_psd(dim), pup, D, LB, dimnum, 10.0)

    def ref(psd_=psd, pup_=pup, ph_=ph, **kw):
        return R.psd_to_psf_ref(psd_, pup_, D, LB, ph_, dimnum, **kw)
    right = ref()
    wrong = {
        'psd_transposed': ref(psd_=psd.T),
        'psd_mirrored': ref(psd_=np.roll(psd[::-1], 1, axis=0)),    # about the DC row
        'psd_flipped': ref(psd_=psd[:, ::-1]),                      # about the middle of the array
        'pupil_transposed': ref(pup_=pup.T),
        'phase_transposed': ref(ph_=ph.T),
        'window_plus_one': ref(window_shift=1),
        'window_minus_one': ref(window_shift=-1),
        'phase_in_nm': ref(ph_=ph * 1e-9),
    }
    moved = {k: _rel(v, right) for k, v in wrong.items()}
    moved['ridge_transposed'] = _rel(ref(psd_=ridge.T), ref(psd_=ridge))
    print('moved by, of the peak:', moved)
    assert min(moved.values()) >= 1000 * TOL, moved
