"""GPU: k_fit_spec bit for bit against the rows recorded on gfx950 (tests/golden/fit_rows_spec_gfx950.npz, written by
scripts/record_fit_rows.py --set spec from the kernel with its intake -- pixel rule, star and model scans, refusal
rules, normalisation, stamp loader -- written out in fit_spec.hip, which the shared intake of fit_common.h and
fit_psf_common.h must reproduce).  The set is tests/fit_spec_cases.py: fit_spectra_psf with 1, 2, 5 and 9 layers (a
wave of the four then owns none, one, two or three of them), background x drift, with and without a variance plane,
with and without psf_index / shift -- over stars with an all-NaN layer, masked pixels, an infinite pixel, every layer
left out, peaks 2^-30, 2^30 and 2^-50, a star 12 px from its model and seeded noisy stars; calls of the first 1 and 2
stars; both precision modes, which run the same fp64 kernel and must give the same rows.  Every column of every row is
compared with np.array_equal (NaN equal to NaN).  Skipped on any other architecture: the record is gfx950's.
"""
import numpy as np
import pytest

import fit_spec_cases as S

gpu = pytest.mark.gpu


def _arch():
    import torch
    if not torch.cuda.is_available():
        return ''
    return torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]


@pytest.fixture(scope='module')
def recorded():
    return np.load(S.RECORD)


@pytest.fixture(scope='module')
def rows():
    if _arch() != 'gfx950':
        pytest.skip('the record is of gfx950')
    import muse_psfr_amd
    cache = {}

    def get(prec):
        if prec not in cache:
            cache[prec] = S.record(muse_psfr_amd, prec)
        return cache[prec]
    return get


def test_the_cubes_are_those_of_the_record(recorded):
    # (no GPU needed: the cubes are made on the host)
    for k, v in S.digests().items():
        assert str(recorded[k]) == v, k
    for k, v in S.names().items():
        assert [str(n) for n in recorded[k]] == list(v), k
    assert str(recorded['arch']) == 'gfx950'
    vs = S.variants()
    assert sorted('spec_' + v[0] for v in vs) == sorted(k for k in recorded.files if k.startswith('spec_'))
    assert {v[1] for v in vs} == set(S.LAYERS) == {1, 2, 5, 9}
    # background x drift, each with and without a variance plane; one variant with psf_index and shift
    assert {(bool(b), bool(d), bool(w)) for _, _, b, d, w, _ in vs} == {(b, d, w) for b in (0, 1) for d in (0, 1) for w in (0, 1)}
    assert any(v[5] for v in vs)
    for v in vs:
        assert recorded['spec_' + v[0]].shape == (len(S.inputs()[v[1]][2]), S.NFIT_SPEC + S.NFIT_SPEC_LAYER * v[1])
    # the paths of the set are in the record: fitted rows, rows on the bound, refused rows, layers left out
    status = np.concatenate([recorded['spec_' + v[0]][:, 10] for v in vs])
    assert set(status.astype(int)) == {0, 1, 2}
    r = recorded['spec_l5b1d1v1g0']
    nm = list(S.names()['names_spec5'])
    layer_status = r[:, S.NFIT_SPEC:].reshape(len(r), 5, S.NFIT_SPEC_LAYER)[:, :, 8]
    assert r[nm.index('nan_layer'), 10] == 0 and list(layer_status[nm.index('nan_layer')]) == [0, 0, 2, 0, 0]
    assert r[nm.index('inf_pixel'), 10] == 0 and list(layer_status[nm.index('inf_pixel')]) == [0, 0, 0, 0, 2]
    assert r[nm.index('all_left_out'), 10] == 2 and r[nm.index('peak_2m50'), 10] == 2
    assert r[nm.index('far_12px'), 10] == 1
    assert r[nm.index('peak_2m30'), 10] == 0 and r[nm.index('peak_2p30'), 10] == 0 and r[nm.index('masked'), 10] == 0


@gpu
@pytest.mark.parametrize('prec', S.MODES)
def test_spec_rows_equal_the_record_bit_for_bit(rows, recorded, prec):
    got = rows(prec)
    assert sorted(got) == sorted(k for k in recorded.files if k.startswith('spec_'))
    bad = []
    for key in sorted(got):
        a, b = got[key], recorded[key]
        assert a.shape == b.shape, key
        for j in range(len(a)):
            if not np.array_equal(a[j], b[j], equal_nan=True):
                cols = [c for c in range(a.shape[1]) if not np.array_equal(a[j, c], b[j, c], equal_nan=True)]
                bad.append((key, S.row_name(key, j), cols))
    assert not bad, bad


@gpu
def test_the_two_precision_modes_give_the_same_rows(rows):
    a, b = rows('mixed'), rows('f64')
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


@gpu
@pytest.mark.parametrize('prec', S.MODES)
def test_the_rows_of_a_star_do_not_depend_on_the_call(recorded, prec):
    if _arch() != 'gfx950':
        pytest.skip('the record is of gfx950')
    import muse_psfr_amd
    for key, k, part in S.subcalls(muse_psfr_amd, prec):
        assert np.array_equal(part, recorded[key][:k], equal_nan=True), (key, k)
