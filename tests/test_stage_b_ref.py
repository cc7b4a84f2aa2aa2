"""CPU: the fp64 reference of the per-wavelength stage (tests/stage_b_ref.py) against the oracle, what the fp32
storage of D_phi0 costs, and the size of the matrix-core arithmetic by the oracle's split-fp16 model -- the scale of
the tolerances tests/test_gpu_stage_b.py asserts on the GPU."""
import numpy as np
import pytest

import psfr_oracle as O
import stage_b_ref as R
from muse_psfr_amd.synthetic import grid_pixscale

LB = np.array([480.0, 700.0, 930.0])


def _case(name):
    """(dim, pixscale, psd [ndir][dim][dim]) of the three input classes."""
    if name == '128x1':
        return 128, grid_pixscale(128), R.model_psd(128, 0.7, 0.8, 22.0)
    if name == '256x4':
        return 256, grid_pixscale(256), R.model_psd(256, 0.6, 0.7, 16.0, npl=2, three=True)
    if name == 'ridge256':
        return 256, grid_pixscale(256), R.ridge_psd(256)[None]
    if name == 'zero256':
        return 256, grid_pixscale(256), np.zeros((1, 256, 256))
    raise KeyError(name)


@pytest.fixture(scope='module')
def planes():
    cache = {}

    def get(name):
        if name not in cache:
            dim, ps, psd = _case(name)
            d0t = R.transposed_half_plane(np.array([O.structure_function0(p) for p in psd]), dim)
            d0t.setflags(write=False)
            cache[name] = (dim, ps, psd, d0t)
        return cache[name]
    return get


def test_half_plane_round_trip(planes):
    """full_plane undoes transposed_half_plane on a plane with D[-u][-v] = D[u][v] and no other symmetry."""
    dim, _, psd, d0t = planes('ridge256')
    d0 = O.structure_function0(psd[0])
    assert np.abs(d0 - d0.T).max() > 1e-3 * d0.max()                   # (the ridge: not symmetric in u <-> v)
    np.testing.assert_allclose(R.full_plane(d0t, dim)[0], d0, rtol=0, atol=1e-12 * d0.max())


@pytest.mark.parametrize('name', ['128x1', '256x4', 'ridge256'])
def test_reference_against_the_oracle(planes, name):
    """stamps_from_dphi0 fed with the oracle's structure function is the oracle's reference-shaped psf_muse."""
    dim, ps, psd, d0t = planes(name)
    err = R.stamp_errors(R.stamps_from_dphi0(d0t, dim, LB, ps), O.psf_stamps_refshaped(psd, LB, 40, ps))
    print('stage_b_ref vs oracle', name, err)
    assert err.max() < 1e-13


@pytest.mark.parametrize('name', ['128x1', '256x4', 'ridge256'])
def test_storage_rounding_of_dphi0(planes, name):
    """Mixed mode stores D_phi0 in fp32.  That rounding alone moves the stamps by less than 1e-7 of the peak (1.5e-8 at
    128^2, 3.6e-9 at 256^2 x 4, 1.8e-8 on the tilted ridge): the reason the GPU tests feed the reference with the STORED plane."""
    dim, ps, _, d0t = planes(name)
    err = R.stamp_errors(R.stamps_from_dphi0(d0t.astype(np.float32), dim, LB, ps), R.stamps_from_dphi0(d0t, dim, LB, ps))
    print('fp32 storage of dphi0', name, err)
    assert err.max() < 1e-7


@pytest.mark.parametrize('name', ['128x1', '256x4', 'zero256'])
def test_arithmetic_model_of_the_matrix_core_stage(planes, name):
    """The oracle's model of the matrix-core kernel (fp32 OTF elements, every operand in two fp16 halves, three
    products, fp32 accumulation, fp16 subnormals flushed) against the fp64 reference from the same fp32-rounded
    plane.  Recorded: 3.8e-7 (128^2), 6.4e-7 (256^2 x 4 directions), 2.5e-7 (zero PSD: OTF = telescope OTF) of the
    peak.  The mixed tolerances of tests/test_gpu_stage_b.py are of this size."""
    dim, ps, psd, d0t = planes(name)
    model = O.psf_stamps_contraction_fp16(psd, LB, 40, ps)
    err = R.stamp_errors(model, R.stamps_from_dphi0(d0t.astype(np.float32), dim, LB, ps))
    print('split-fp16 model vs fp64', name, err)
    assert err.max() < 1e-6


def test_size_of_a_lost_low_half_by_the_model():
    """What the sensitivity test of tests/test_gpu_stage_b.py switches on -- every block of the matrix-core kernel
    without the low fp16 half of the OTF -- by the model: 3.7e-5 ... 3.8e-4 of the peak on the zero PSD at the seven
    wavelengths that test uses, at least ten times the largest tolerance a matrix-core variant may get (2e-6)."""
    dim, ps = 256, grid_pixscale(256)
    lb = R.wavelength_set(dim, ps, 7)
    ref = R.stamps_from_dphi0(np.zeros((1, dim // 2 + 1, dim)), dim, lb, ps)
    err = R.stamp_errors(O.psf_stamps_contraction_fp16(np.zeros((1, dim, dim)), lb, 40, ps, otf_low=False), ref)
    print('model without the low OTF half, zero PSD', err)
    assert err.min() >= 10 * 2e-6


def test_wavelengths_for_grid():
    """The wavelengths the GPU tests pick per grid reach what they are meant to reach."""
    for dim in (128, 256, 512, 1024, 1280):
        ps = grid_pixscale(dim)
        npc = O.npix_crop(R.wavelengths_for_grid(dim, ps), 40, ps)
        assert npc[0] == dim and npc[1] % 40 == 0 and npc[2] == npc[1] + 2 and npc[3] < npc[1], (dim, npc)


def test_ladder_scales():
    dim = 256
    d0 = O.structure_function0(R.model_psd(dim, 0.8, 0.6, 15.0)[0])
    support = R.telescope_support(dim)
    targets = (-10, -17, -19, -28, -30, -40)
    for s, t in zip(R.ladder_scales(d0, 700.0, targets, support), targets):
        e = (-0.5 * (2 * np.pi / 700.0) ** 2 * np.log2(np.e) * s * d0)[support].min()
        assert abs(e - t) < 1e-9
