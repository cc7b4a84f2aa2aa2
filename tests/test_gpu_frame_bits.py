"""GPU: the frame calls bit for bit against the outputs recorded on gfx950 (tests/golden/frame_calls_gfx950.npz, written by
scripts/record_frame_calls.py from the build before render.hip, frame_fit.hip, find.hip and group.hip went onto one
star list, one workspace layout and one model window -- csrc/frame_common.h: the code moved, and no operand of any sum
or its order).  The calls are those of tests/frame_bits_cases.py: mpsfr_render_stars on the scene whose pile overflows
the LDS sort, added, on zeros and subtracted, and on the 1 x 1, 1 x 200 and 200 x 1 frames; mpsfr_fit_frame_psf on its
scene for the four (var, background) combinations; mpsfr_find_stars with and without var at half 2 and 3;
mpsfr_group_stars on every scene of group_ref.  Every recorded array is compared with np.array_equal over its bytes
(NaN equals NaN, -0 differs from +0), a frame above 4096 values through the SHA-256 of its bytes as the record keeps
it, in the mixed and in the f64 mode, and one case of every call once more through device pointers.  Skipped on any
other architecture: the record is gfx950's.
"""
import numpy as np
import pytest

import frame_bits_cases as C

pytestmark = pytest.mark.gpu


def _arch():
    import torch
    if not torch.cuda.is_available():
        return ''
    return torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]


@pytest.fixture(scope='module')
def recorded():
    return np.load(C.RECORD)


_CTX = {}


@pytest.fixture
def ctx(prec):
    if _arch() != 'gfx950':
        pytest.skip('the record is of gfx950')
    if prec not in _CTX:
        import muse_psfr_amd
        _CTX[prec] = C.context(muse_psfr_amd, prec)
    return _CTX[prec]


def _names(recorded):
    return [k for k in recorded.files if k.split('.')[0] in C.CALLS]


def test_the_inputs_and_the_cases_are_those_of_the_record(recorded):
    assert str(recorded['inputs_sha256']) == C.digest(C.inputs())
    assert str(recorded['arch']) == 'gfx950' and int(recorded['hash_above']) == C.HASH_ABOVE
    cases = list(C.render_cases()) + list(C.fit_cases()) + list(C.find_cases()) + list(C.group_cases())
    assert len(cases) == 9 + 4 + 4 + 8
    outputs = {'render': ('frame', 'rows'), 'fit': ('rows', 'head', 'resid'), 'find': ('rows', 'origin', 'count', 'map'),
               'group': ('label', 'groups', 'origin', 'shift', 'counts')}
    want = sorted('%s.%s' % (c, o) for c in cases for o in outputs[c.split('.')[0]])
    assert sorted(_names(recorded)) == want             # no array was left out of the record
    # the whole frames are kept as digests, everything else in full
    small = tuple('render.%dx%d.' % s for s in C.DEGENERATE)
    for k in want:
        hashed = recorded[k].dtype == np.uint8 and recorded[k].shape == (32,)
        assert hashed == (k.rsplit('.', 1)[-1] in C.FRAMES and not k.startswith(small)), k
    assert all(k in want for k in (c + '.' + o for c in C.DEVICE_CASES for o in outputs[c.split('.')[0]]))


@pytest.mark.parametrize('prec', C.MODES)
def test_every_output_equals_the_record_bit_for_bit(ctx, recorded, prec):
    got = C.record(ctx)
    names = _names(recorded)
    assert sorted(got) == sorted(names)
    differ = [k for k in names if not C.same(k, got[k], recorded[k])]
    assert not differ, differ
    for k in names:
        assert np.array_equal(C.bits(C.stored(k, got[k])), C.bits(recorded[k])), k


@pytest.mark.parametrize('prec', C.MODES)
def test_device_pointers_give_the_bits_of_the_record(ctx, recorded, prec):
    got = C.record_device(ctx)
    assert sorted(got) == sorted(k for k in _names(recorded) if k.rsplit('.', 1)[0] in C.DEVICE_CASES)
    differ = [k for k in sorted(got) if not C.same(k, got[k], recorded[k])]
    assert not differ, differ
