"""GPU: k_fit_ell, k_fit_obs, k_fit_psf and k_fit_group bit for bit against the rows recorded on gfx950
(tests/golden/fit_rows_models_gfx950.npz, written by scripts/record_fit_rows.py --set models: the rows of the kernels
with their Levenberg-Marquardt loop, polish and error columns written out in each of them, which the shared forms of
fit_common.h must reproduce -- no operand or order of an operation may move).  The set is tests/fit_models_cases.py: fit_stamps_elliptical;
fit_stamps_observed in the four background x circular variants, each with and without a variance plane;
fit_stamps_psf with background x fixed_shift, with and without psf_index / shift and a variance plane; fit_groups_psf
for K = 2, 3, 4 in the modes free, common and fixed, with and without background -- over the golden stamps, off-centre
and near-edge peaks, stamps that run down the valley of eta through limited steps (n = 16, and narrower than two
pixels), stamps elongated to the |e| bound, NaN / negative / constant stamps, peaks 2^-30 and 2^30, masked pixels,
shifts that rest on their bound and a singular group; calls of 1, 2 and 65 stamps; both precision modes.  Every column
of every row is compared with np.array_equal (NaN equal to NaN).  Skipped on any other architecture: the record is
gfx950's.
"""
import numpy as np
import pytest

import fit_models_cases as M

gpu = pytest.mark.gpu


def _arch():
    import torch
    if not torch.cuda.is_available():
        return ''
    return torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]


@pytest.fixture(scope='module')
def recorded():
    return np.load(M.RECORD)


@pytest.fixture(scope='module')
def rows():
    if _arch() != 'gfx950':
        pytest.skip('the record is of gfx950')
    import muse_psfr_amd
    cache = {}

    def get(prec):
        if prec not in cache:
            cache[prec] = M.record(muse_psfr_amd, (prec,))
        return cache[prec]
    return get


def test_the_stamps_are_those_of_the_record(recorded):
    # (no GPU needed: the stamps are made on the host)
    for k, v in M.digests().items():
        assert str(recorded[k]) == v, k
    for k, v in M.names().items():
        assert [str(n) for n in recorded[k]] == list(v), k
    assert str(recorded['arch']) == 'gfx950'
    inp = M.inputs()
    assert all(len(inp[k][2 if k != 'moffat' else 1]) > max(M.CALL_SIZES) for k in ('moffat', 'psf', 'group2'))
    assert len(M.observed_variants()) == 8 and len(M.psf_variants()) == 16 and len(M.group_variants()) == 18


@gpu
@pytest.mark.parametrize('prec', M.MODES)
def test_fit_rows_equal_the_record_bit_for_bit(rows, recorded, prec):
    got = rows(prec)
    assert sorted(got) == sorted(k for k in recorded.files if k.split('_')[0] in ('ell', 'obs', 'psf', 'grp')
                                 and k.split('_')[1] == prec)
    bad = []
    for key in sorted(got):
        a, b = got[key], recorded[key]
        assert a.shape == b.shape, key
        for j in range(len(a)):
            if not np.array_equal(a[j], b[j], equal_nan=True):
                cols = [c for c in range(a.shape[1]) if not np.array_equal(a[j, c], b[j, c], equal_nan=True)]
                bad.append((key, M.row_name(key, j), cols))
    assert not bad, bad


@gpu
@pytest.mark.parametrize('prec', M.MODES)
def test_the_rows_of_a_stamp_do_not_depend_on_the_call(recorded, prec):
    if _arch() != 'gfx950':
        pytest.skip('the record is of gfx950')
    import muse_psfr_amd
    for key, k, part in M.subcalls(muse_psfr_amd, prec):
        assert np.array_equal(part, recorded[key][:k], equal_nan=True), (key, k)
