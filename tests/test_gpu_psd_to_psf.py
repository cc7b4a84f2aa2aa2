"""GPU: psd_to_psf (psfrec.py:689-807) against the reference's values (g8), the complex128 oracle at the native
grid, the validated psf_muse path, and its batching / device-output / concurrency guarantees."""
import numpy as np
import pytest

from conftest import H, record_margin
import psfr_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-10          # of the reference PSF's peak
D = 8.0


def _fov(dim, lb):
    return (lb * 1e9 / (2 * D)) * dim / (4.85 * 1e3)      # as psf_muse passes it (psfrec.py:662)


def _check(name, got, want, peak=None):
    peak = np.abs(want).max() if peak is None else peak
    err = float(np.abs(got - want).max() / peak)
    record_margin('psd_to_psf', **{name: err})
    assert err <= TOL, (name, err)


def _psd(g, name):
    """The PSD of the fixture: top-left quadrant mirrored along both axes, then the central block
    (tools/make_golden_psd_to_psf.py)."""
    quad, centre = g[name + '_quad'], g[name + '_centre']
    h, c = quad.shape[0], centre.shape[0] // 2
    full = np.block([[quad, quad[:, ::-1]], [quad[::-1], quad[::-1, ::-1]]])
    full[h - c:h + c, h - c:h + c] = centre
    return full.astype(np.float64)


def _crop(p, c):
    n = p.shape[-1]
    return p[..., n // 2 - c:n // 2 + c, n // 2 - c:n // 2 + c]


@pytest.mark.parametrize('precision', ['mixed', 'f64'])
def test_cases_equal_the_reference(golden, precision):
    from muse_psfr_amd import psd_to_psf
    g = golden('g8_psd_to_psf')
    lb = g['lbda']
    pup = g['pup_muse256'].astype(int)
    kw = dict(precision=precision)
    # a: MUSE pupil, FoV as psf_muse passes it, one wavelength per call; the fixture keeps rows 0 .. 128 of the
    # reference's planes (they are point symmetric), and the other rows are checked as the mirror of ours
    psd = _psd(g, 'psd256')
    psf_a = []
    for i, l in enumerate(lb):
        p = psd_to_psf(psd, pup, D, l, samp=2, FoV=_fov(256, l), **kw)
        assert p.shape == (256, 256)
        _check('a_' + precision, p[:129], g['psf_a_half'][i])
        assert np.abs(p - np.roll(p[::-1, ::-1], 1, axis=(0, 1))).max() <= 1e-14 * p.max()   # p[i][j] = p[-i][-j]
        assert abs(p.sum() - 1) < 1e-12
        psf_a.append(p)
    psf_a = np.array(psf_a)
    c = int(g['crop'])

    def check_crop(case, p):
        peak = g['peak_' + case].max()
        _check(case + '_' + precision, _crop(p, c), g['crop_' + case], peak)
        _check(case + '_rows_' + precision, p.sum(axis=2), g['rows_' + case], peak)
        _check(case + '_cols_' + precision, p.sum(axis=1), g['cols_' + case], peak)
        np.testing.assert_allclose(p.sum(axis=(1, 2)), 1, rtol=0, atol=1e-12)
    # b: + static phase (metres), all wavelengths in one call
    p = psd_to_psf(psd, pup, D, lb, phase_static=g['phase_b'].astype(float), samp=2, FoV=_fov(256, lb), **kw)
    assert p.shape == (2, 256, 256)
    check_crop('b', p)
    diff = np.abs(p - psf_a).max()                         # the phase matters: as much as in the reference
    assert abs(diff - g['maxdiff_ab']) <= TOL * (psf_a.max() + g['peak_b'].max()), (diff, g['maxdiff_ab'])
    assert diff > 1e-4 * psf_a.max()
    # c: samp < sampnum (dim 512, npup 128 -> dimnum 256); d: apodised pupil with spiders (dimnum 512)
    psd5 = _psd(g, 'psd512')
    for case, pup_ in (('c', g['pup_c'].astype(int)), ('d', g['pup_d_4096'] / 4096.0)):
        p = psd_to_psf(psd5, pup_, D, lb, samp=2, **kw)
        n = int(g['dimnum_' + case])
        assert p.shape == (2, n, n)
        check_crop(case, p)
    # e: return_all (the reference's planes are those of a)
    psf, sampout, fov = psd_to_psf(psd, pup, D, lb, samp=2, return_all=True, **kw)
    np.testing.assert_array_equal(sampout, g['sampout_e'][0])
    np.testing.assert_array_equal(fov, g['fov_e'])
    np.testing.assert_array_equal(psf, psf_a)
    for i, l in enumerate(lb):
        one = psd_to_psf(psd, pup, D, l, samp=2, return_all=True, **kw)
        assert one[1] == g['sampout_e'][i] and one[2] == g['fov_e'][i]


def test_native_1280_equals_the_oracle():
    from muse_psfr_amd import Context, pupil_mask
    ctx = Context(dim=1280, precision='f64')
    try:
        psd = ctx.simul_psd(1.0, 0.7, 25.0)[0]
        pup = pupil_mask(1280 / 4, 1280 / 2, oc=0.14)
        lb = np.array([490e-9, 700e-9, 930e-9])
        p = ctx.psd_to_psf(psd, pup, D, lb)[0]
        for i, l in enumerate(lb):
            want = O.psd_to_psf_refshaped(psd, pup, l)
            _check('native1280', p[i], want)
            assert abs(p[i].sum() - 1) < 1e-12
    finally:
        ctx.close()


@pytest.mark.parametrize('dim', [512, 1280])
def test_agrees_with_psf_muse(dim):
    """psf_muse's stamps (psfrec.py:677-685) rebuilt from the full-field PSF equal the validated stamp path
    (at the pixel scale that makes the grid runnable, grid_pixscale: 0.2 arcsec at 1280)."""
    from muse_psfr_amd import crop, grid_pixscale, interpolate, psd_to_psf, pupil_mask
    from muse_psfr_amd.psfrec import get_context
    ps = grid_pixscale(dim)
    ctx = get_context(dim, ps, 40, 'f64', 0)
    psd = ctx.simul_psd(1.2, 0.6, 20.0)[0]
    lbn = np.array([490.0, 650.0, 920.0])
    want = ctx.psf_from_psd(psd, lbn)
    pup = pupil_mask(dim / 4, dim / 2, oc=0.14)
    npixc = (np.round(((40 * ps * 2 * 8 * 4.85 * 1000) / lbn) / 2) * 2).astype(int)
    full = psd_to_psf(psd, pup, D, lbn * 1e-9, samp=2, FoV=_fov(dim, lbn * 1e-9), precision='f64')
    for i in range(lbn.size):
        p = crop(full[i], center=dim // 2, size=npixc[i] // 2).copy()
        p /= p.sum()
        np.maximum(p, 0, out=p)
        st = interpolate(p, np.mgrid[:40, :40] * npixc[i] / 40)
        st /= st.sum()
        _check('psf_muse_%d' % dim, st, want[i])


def test_batch_equals_single_and_device_equals_host():
    import torch
    from muse_psfr_amd import Context, pupil_mask
    ctx = Context(dim=256, precision='mixed')
    try:
        psd = np.stack([ctx.simul_psd(s, 0.7, 25.0)[0] for s in (0.6, 1.0, 1.5)])
        pup = pupil_mask(64, 128, oc=0.14) * (1.0 + 0.1 * np.linspace(-1, 1, 128))[None, :]
        ph = 20e-9 * np.outer(np.linspace(-1, 1, 128), np.ones(128))
        lb = np.array([480e-9, 600e-9, 750e-9, 930e-9])
        for phase in (None, ph):
            many = ctx.psd_to_psf(psd, pup, D, lb, phase_static=phase)
            assert many.shape == (3, 4, 256, 256)
            for p in range(3):
                for i in range(4):
                    one = ctx.psd_to_psf(psd[p], pup, D, lb[i], phase_static=phase)[0, 0]
                    np.testing.assert_array_equal(one, many[p, i])
            dev = torch.empty(many.shape, dtype=torch.float64, device='cuda:0')
            assert ctx.psd_to_psf(psd, pup, D, lb, phase_static=phase, out=dev.data_ptr()) is None
            np.testing.assert_array_equal(dev.cpu().numpy(), many)
        # more wavelengths than one chunk holds (the OTFs of a static phase are rebuilt per chunk)
        lb20 = np.linspace(470e-9, 930e-9, 20)
        many = ctx.psd_to_psf(psd[0], pup, D, lb20, phase_static=ph)[0]
        for i in (0, 9, 19):
            np.testing.assert_array_equal(ctx.psd_to_psf(psd[0], pup, D, lb20[i], phase_static=ph)[0, 0], many[i])
    finally:
        ctx.close()


def test_no_interference_with_asynchronous_reconstructions():
    from muse_psfr_amd import Context, grid_pixscale, pupil_mask
    ctx = Context(dim=512, pixscale=grid_pixscale(512), precision='mixed')
    try:
        lb = np.array([480.0, 700.0, 930.0])
        see, gl, l0 = np.array([1.0, 0.8, 1.4]), np.array([0.7, 0.5, 0.6]), np.array([25.0, 20.0, 15.0])
        three = np.array([0, 1, 0])
        psd = ctx.simul_psd(1.0, 0.7, 25.0)[0]
        pup = pupil_mask(128, 256, oc=0.14)
        want1 = ctx.reconstruct(lb, see, gl, l0, three, H)
        want2 = ctx.reconstruct(lb, see[::-1], gl[::-1], l0[::-1], three[::-1], H)
        alone = ctx.psd_to_psf(psd, pup, D, lb * 1e-9)
        r1 = ctx.reconstruct_async(lb, see, gl, l0, three, H)
        mid = ctx.psd_to_psf(psd, pup, D, lb * 1e-9)
        r2 = ctx.reconstruct_async(lb, see[::-1], gl[::-1], l0[::-1], three[::-1], H)
        got1, got2 = r1.wait(), r2.wait()
        np.testing.assert_array_equal(mid, alone)
        for got, want in ((got1, want1), (got2, want2)):
            for k in ('psf', 'fit'):
                np.testing.assert_array_equal(got[k], want[k])
    finally:
        ctx.close()
