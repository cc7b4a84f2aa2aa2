"""GPU: the pipeline calls bit for bit against the outputs recorded on gfx950 (tests/golden/reconstruct_calls_gfx950.npz,
written by scripts/record_reconstruct_calls.py from the build before reconstruct_impl of mpsfr_api.cpp was cut into a
call preparation, context steps, chunk stages and three stage-level drivers: host code moved, and no kernel, grid,
stream, event or wait).  The cases are those of tests/reconstruct_bits_cases.py: the default paths, the options, the
entry points, the stage-level calls, the output forms and the call sequences.  Every recorded array is compared with
np.array_equal over its bytes (NaN equals NaN, -0 differs from +0), an array above 4096 values through the SHA-256 of
its bytes as the record keeps it.  A second run of every case under the `profile`
option gives the timed scopes per kernel id, held to the record too: the same kernels queued the same number of times,
which equal results alone do not say.  Every call of a sequence equals the same call on a fresh context.  Skipped on
any other architecture: the record is gfx950's.
"""
import numpy as np
import pytest

import reconstruct_bits_cases as C

pytestmark = pytest.mark.gpu
META = ('arch', 'inputs_sha256', 'hash_above')


def _arch():
    import torch
    if not torch.cuda.is_available():
        return ''
    return torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]


@pytest.fixture(scope='module')
def recorded():
    return np.load(C.RECORD)


@pytest.fixture(scope='module')
def api():
    if _arch() != 'gfx950':
        pytest.skip('the record is of gfx950')
    import muse_psfr_amd
    return muse_psfr_amd


def _keys(recorded, name):
    from_case = [k for k in recorded.files if k not in META and k.startswith(name + '.')]
    longer = [n for n in C.cases() if n != name and n.startswith(name + '.')]
    return [k for k in from_case if not any(k.startswith(n + '.') for n in longer)]


def test_the_inputs_and_the_cases_are_those_of_the_record(recorded):
    assert str(recorded['inputs_sha256']) == C.digest(C.inputs())
    assert str(recorded['arch']) == 'gfx950' and int(recorded['hash_above']) == C.HASH_ABOVE
    names = list(C.cases())
    assert len(names) == 17 + 15 + 12 + 6 + 5
    for name in names:
        keys = _keys(recorded, name)
        assert name + '.scopes' in keys, name
        # no psf and no fit array was left out: every case keeps an output, every reconstruct-like one its fit
        assert len(keys) >= 2, name
    seq = [n for n in names if n.startswith('seq.')]
    for name in seq:
        assert name + '.d0t_clears' in recorded.files
        for k in range(3):
            if (name, k) != ('seq.refused', 1) and (name, k) != ('seq.stage_between', 1):
                for o in C.OUT:
                    assert '%s.c%d.%s' % (name, k, o) in recorded.files and '%s.f%d.%s' % (name, k, o) in recorded.files
    assert int(recorded['seq.refused.c1.code'][0]) == C.E_GRID
    for k in recorded.files:
        if k not in META:
            hashed = recorded[k].dtype == np.uint8 and recorded[k].shape == (32,)
            assert not (hashed and k.rsplit('.', 1)[-1] in ('fit', 'scopes', 'd0t_clears', 'code')), k


@pytest.mark.parametrize('name', list(C.cases()))
def test_every_output_equals_the_record_bit_for_bit(api, recorded, name):
    got = C.record(api, name)
    keys = [k for k in _keys(recorded, name) if not k.endswith('.scopes')]
    assert sorted(got) == sorted(keys)
    differ = [k for k in keys if not C.same(k, got[k], recorded[k])]
    assert not differ, differ
    loose = [a for a, b in C.held_to_fresh(sorted(got)) if not np.array_equal(C.bits(got[a]), C.bits(got[b]))]
    assert not loose, loose


@pytest.mark.parametrize('name', list(C.cases()))
def test_the_same_kernels_are_queued_the_same_number_of_times(api, recorded, name):
    got = C.record(api, name, profile=True)
    k = name + '.scopes'
    assert np.array_equal(got[k], recorded[k]), (got[k].tolist(), recorded[k].tolist())
