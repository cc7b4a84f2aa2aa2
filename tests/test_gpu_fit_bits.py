"""GPU: k_fit bit for bit against the rows recorded on gfx950 (tests/golden/fit_rows_gfx950.npz, written by
scripts/record_fit_rows.py from the build before the wave-uniform overhead of the kernel was cut: reductions,
argmax, the pixel reads of the polish and the covariance changed their instructions, and none of their operands or
their order).  The set is tests/fit_bits_cases.py: the golden stamps a-d, a brightest pixel in each of the 64 lane
classes, equal maxima inside a quad, a row of lanes and across rows, a peak near an edge, NaN / negative / constant
stamps, peaks 2^-30 and 2^30, calls of 1, 2 and 65 stamps, both precision modes, and the rows of a reconstruct with
float and with double final stamps.  Every one of the 16 columns is compared with np.array_equal (NaN equal to NaN).
Skipped on any other architecture: the record is gfx950's.
"""
import numpy as np
import pytest

import fit_bits_cases as C

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
def rows():
    if _arch() != 'gfx950':
        pytest.skip('the record is of gfx950')
    import muse_psfr_amd
    cache = {}

    def get(prec):
        if prec not in cache:
            cache[prec] = C.record(muse_psfr_amd, (prec,))
        return cache[prec]
    return get


def test_the_stamps_are_those_of_the_record(recorded):
    st = C.stamps()
    assert [str(n) for n in recorded['names']] == [n for n, _ in C.cases()]
    assert len(st) > max(C.CALL_SIZES)
    assert str(recorded['stamps_sha256']) == C.digest(st)
    assert str(recorded['arch']) == 'gfx950'
    for k, v in (('call_lbda', C.CALL_LBDA), ('call_seeing', C.CALL_SEEING), ('call_gl', C.CALL_GL), ('call_l0', C.CALL_L0)):
        assert np.array_equal(recorded[k], v)


@pytest.mark.parametrize('prec', C.MODES)
def test_fit_rows_equal_the_record_bit_for_bit(rows, recorded, prec):
    got = rows(prec)
    names = [n for n, _ in C.cases()]
    assert sorted(got) == sorted(k for k in recorded.files if k.startswith(('rows_%s' % prec, 'call_%s' % prec)))
    bad = []
    for key in sorted(got):
        a, b = got[key], recorded[key]
        assert a.shape == b.shape and a.shape[1] == 16, key
        for j in range(len(a)):
            if not np.array_equal(a[j], b[j], equal_nan=True):
                cols = [c for c in range(16) if not np.array_equal(a[j, c], b[j, c], equal_nan=True)]
                bad.append((key, names[j] if key.startswith('rows') else j, cols))
    assert not bad, bad
    # the rows of a stamp do not depend on the call it is in
    full = got['rows_%s' % prec]
    for k in C.CALL_SIZES:
        assert np.array_equal(got['rows_%s_first%d' % (prec, k)], full[:k], equal_nan=True)
