"""GPU: the convolution stage bit for bit against the stamps recorded on gfx950 (tests/golden/conv_stamps_gfx950.npz,
written by scripts/record_conv_stamps.py from the build before the column phase of k_conv_fft went from two forward
transforms in wave 0 -- one for slot 0's packed DC / Nyquist column, one for slots 1-7 -- to one for all slots: the
instructions changed, and none of their operands or their order).  The set is tests/conv_bits_cases.py: two tasks whose
tip-tilt kernels differ six-fold in width, 465 and 930 nm, a Moffat-like class and a "hard" class with its energy in the
DC and Nyquist column and row, which is what slot 0 carries; Context.convolve_stamps in the mixed mode
(k_conv_fft<float, double>) and in the f64 mode.  Every element is compared with np.array_equal.  The flagship's
k_conv_fft<float, float> differs in the final cast only and is held by the reconstruct rows of tests/test_gpu_fit_bits.py.
Skipped on any other architecture: the record is gfx950's.
"""
import numpy as np
import pytest

import conv_bits_cases as C

pytestmark = pytest.mark.gpu


def _arch():
    import torch
    if not torch.cuda.is_available():
        return ''
    return torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]


@pytest.fixture(scope='module')
def recorded():
    return np.load(C.RECORD)


@pytest.fixture(scope='module')
def outputs():
    if _arch() != 'gfx950':
        pytest.skip('the record is of gfx950')
    import muse_psfr_amd
    return C.record(muse_psfr_amd)


def test_the_inputs_are_those_of_the_record(recorded):
    pre, par = C.inputs()
    assert pre.shape == (4, 2, C.NS, C.NS) and par.shape == (4, 3)
    assert str(recorded['inputs_sha256']) == C.digest(pre)
    assert str(recorded['arch']) == 'gfx950'
    assert int(recorded['dim']) == C.DIM and int(recorded['grid']) == C.GRID and int(recorded['seed']) == C.SEED
    assert np.array_equal(recorded['lbda'], C.LBDA) and np.array_equal(recorded['tasks'], C.TASKS)
    assert [str(c) for c in recorded['classes']] == list(C.CLASSES)
    assert tuple(recorded['shape']) == pre.shape
    for prec in C.MODES:
        assert C.values(recorded['out_%s' % prec], prec, pre.shape).dtype == C.DTYPE[prec]


@pytest.mark.parametrize('prec', C.MODES)
def test_final_stamps_equal_the_record_bit_for_bit(outputs, recorded, prec):
    got = outputs['out_%s' % prec]
    want = C.values(recorded['out_%s' % prec], prec, tuple(recorded['shape'])).astype(np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape
    diff = got != want
    bad = [(int(k), int(l), int(diff[k, l].sum())) for k, l in zip(*np.nonzero(diff.any(axis=(-1, -2))))]
    assert not bad, ('(task, wavelength, elements that differ)', bad)
    assert np.array_equal(got, want)
