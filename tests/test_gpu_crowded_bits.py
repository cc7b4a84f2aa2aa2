"""GPU: the four crowded-field fits bit for bit against the outputs recorded on gfx950
(tests/golden/crowded_calls_gfx950.npz, written by scripts/record_crowded_calls.py from the build before the step
kernels k_ff_step, k_fr_step and k_cf_step took their conjugate-gradient step, their star rows and their position update
from one place each: the code moved, and no operand of any sum or its order).  The cases are those of
tests/crowded_bits_cases.py: mpsfr_fit_frame_psf on the live lattice on both sides of 1024 unknowns;
mpsfr_fit_frame_psf_free on the displaced scene through every branch of its outer loop and on the lattice's 3268
unknowns; mpsfr_fit_cube_psf with and without the constant at two batch sizes; mpsfr_fit_cube_psf_free on the
three-layer cube, on a dead and on a faint layer and on 1025 layers.  Every recorded array is compared with
np.array_equal over its bytes (NaN equals NaN, -0 differs from +0), one above 4096 values through the SHA-256 of its
bytes as the record keeps it, in the mixed and in the f64 mode, and one case of every call once more through device
pointers.  Skipped on any other architecture: the record is gfx950's.
"""
import numpy as np
import pytest

import crowded_bits_cases as C

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
def contexts():
    """One context per precision mode, made when first asked for and closed at the end of the module."""
    made = {}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture
def ctx(contexts, prec):
    if _arch() != 'gfx950':
        pytest.skip('the record is of gfx950')
    if prec not in contexts:
        import muse_psfr_amd
        contexts[prec] = C.context(muse_psfr_amd, prec)
    return contexts[prec]


def _names(recorded):
    return [k for k in recorded.files if k.split('.')[0] in C.CALLS]


def _outputs(case):
    return ['%s.%s' % (case, o) for o in C.OUTPUTS[case.split('.')[0]]]


def test_the_inputs_and_the_cases_are_those_of_the_record(recorded):
    assert str(recorded['inputs_sha256']) == C.digest(C.inputs())
    assert str(recorded['arch']) == 'gfx950' and int(recorded['hash_above']) == C.HASH_ABOVE
    cases = list(C.cases())
    assert [sum(c.startswith(call + '.') for c in cases) for call in C.CALLS] == [3, 12, 4, 12]
    want = sorted(k for c in cases for k in _outputs(c))
    assert sorted(_names(recorded)) == want             # no array was left out of the record
    # the residual frames and cubes are kept as digests; of the 34-star cases everything else in full
    small = ('free.', 'cube.', 'cubefree.')
    big = ('free.lattice', 'cubefree.deep_')
    for k in want:
        hashed = recorded[k].dtype == np.uint8 and recorded[k].shape == (32,)
        if k.endswith('.resid'):
            assert hashed, k
        elif k.startswith(small) and not k.startswith(big):
            assert not hashed and recorded[k].dtype == np.float64, k
    assert all(c in cases for c in C.DEVICE_CASES) and {c.split('.')[0] for c in C.DEVICE_CASES} == set(C.CALLS)


@pytest.mark.parametrize('case', list(C.cases()))
@pytest.mark.parametrize('prec', C.MODES)
def test_every_output_equals_the_record_bit_for_bit(ctx, recorded, prec, case):
    got = C.run(ctx, case)
    assert sorted(got) == sorted(_outputs(case))
    differ = [k for k in sorted(got) if not C.equal(k, got[k], recorded[k])]
    assert not differ, differ


@pytest.mark.parametrize('case', C.DEVICE_CASES)
@pytest.mark.parametrize('prec', C.MODES)
def test_device_pointers_give_the_bits_of_the_record(ctx, recorded, prec, case):
    got = C.run_device(ctx, case)
    assert sorted(got) == sorted(_outputs(case))
    differ = [k for k in sorted(got) if not C.equal(k, got[k], recorded[k])]
    assert not differ, differ
