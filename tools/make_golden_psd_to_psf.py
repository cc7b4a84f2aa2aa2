"""Capture of tests/golden/g8_psd_to_psf.npz: inputs and the reference's outputs of psd_to_psf
(psfrec.py:689-807) and of its helpers pupil_mask, crop, interpolate, seeing2r01.  Runs in the
reference's own environment (astropy, scipy):

    /opt/conda/bin/python3.9 -B tools/make_golden_psd_to_psf.py

The fixture is kept small; every input the reference saw is stored exactly (the reference is fed the
decoded values, and decoding is exact):
  * PSDs: float32.  Outside the corrected zone simul_psd_wfm's PSD is mirror symmetric about
    (dim - 1) / 2 along both axes, so only the top-left quadrant and the central (2 CENTRE)^2 block are
    stored (psd_decode; the capture asserts that the decoded PSD equals the generated one bit for bit).
  * the apodised pupil: multiples of 1/4096 (uint16 numerators); the static phase: float32 metres.
Cases (each at 500 and 800 nm):
  a  MUSE pupil pupil_mask(dim/4, dim/2, oc=0.14), simul_psd_wfm PSD, dim 256, samp=2, FoV as psf_muse passes it
  b  a + a static phase (defocus + astigmatism, tens of nm, in metres)
  c  samp < sampnum: dim 512, npup 128, samp 2 -> dimnum 256
  d  apodised pupil with spider vanes, dim 512, npup 256 -> dimnum 512
  e  return_all=True (the inputs of a; the reference's planes equal a's bit for bit, so only sampout and FoV)
Case a keeps the full plane as rows 0 .. dimnum/2: the PSF is point symmetric, PSF[i][j] = PSF[-i][-j] (indices
mod dimnum; the transform of a real even OTF), which the capture asserts for the reference's planes to 1e-14 of the
peak.  The other cases keep the central (2 CROP)^2 crop and the row and column sums.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))
from _refload import load_reference  # noqa: E402

OUT = os.path.join(HERE, '..', 'tests', 'golden', 'g8_psd_to_psf.npz')
LBDA = np.array([500e-9, 800e-9])
D = 8.0
CROP = 24
CENTRE = 48


def psd_decode(quad, centre):
    """The (dim, dim) float64 PSD from its top-left quadrant and its central block (see above)."""
    h, c = quad.shape[0], centre.shape[0] // 2
    full = np.empty((2 * h, 2 * h), dtype=np.float32)
    full[:h, :h] = quad
    full[:h, h:] = quad[:, ::-1]
    full[h:, :h] = quad[::-1]
    full[h:, h:] = quad[::-1, ::-1]
    full[h - c:h + c, h - c:h + c] = centre
    return full.astype(np.float64)


def ref_psd(ref, dim, out, name):
    """simul_psd_wfm's PSD rounded to float32, stored compactly in `out`; returns the decoded float64 PSD."""
    psd = ref.simul_psd_wfm([0.7, 0.3], (100, 10000), 1.0, 25.0, zenith=0., npsflin=1, dim=dim,
                            three_lgs_mode=False, verbose=False)[0].astype(np.float32)
    h = dim // 2
    out[name + '_quad'] = psd[:h, :h]
    out[name + '_centre'] = psd[h - CENTRE:h + CENTRE, h - CENTRE:h + CENTRE]
    dec = psd_decode(out[name + '_quad'], out[name + '_centre'])
    assert np.array_equal(dec, psd.astype(np.float64)), 'the PSD is not mirror symmetric outside the centre'
    return dec


def static_phase(npup):
    """30 nm rms-ish defocus and 20 nm astigmatism over the unit disc of the pupil, in metres."""
    c = (npup - 1) / 2
    y, x = (np.mgrid[:npup, :npup] - c) / (npup / 2)
    r2 = x * x + y * y
    return ((30e-9 * (2 * r2 - 1) + 20e-9 * (x * x - y * y)) * (r2 < 1)).astype(np.float32).astype(np.float64)


def spider_pupil(ref, npup):
    """Apodised (Gaussian taper), centrally obscured pupil with four spider vanes 3 px wide."""
    pup = ref.pupil_mask(npup / 2, npup, oc=0.14).astype(float)
    c = (npup - 1) / 2
    y, x = np.mgrid[:npup, :npup] - c
    pup *= np.round(4096 * np.exp(-0.5 * (x * x + y * y) / (0.45 * npup) ** 2)) / 4096
    pup[np.abs(x - y) < 1.5] = 0.0
    pup[np.abs(x + y) < 1.5] = 0.0
    return pup


def fov_psf_muse(dim, lbda_m):
    """FoV as psf_muse passes it (psfrec.py:662) for lambdamuse = lbda_m in nm."""
    return (lbda_m * 1e9 / (2 * D)) * dim / (4.85 * 1e3)


def _crop(p):
    n = p.shape[-1]
    return p[..., n // 2 - CROP:n // 2 + CROP, n // 2 - CROP:n // 2 + CROP]


def _keep_crop(out, name, planes):
    planes = np.asarray(planes)
    out['crop_' + name] = _crop(planes)
    out['rows_' + name] = planes.sum(axis=2)
    out['cols_' + name] = planes.sum(axis=1)
    out['peak_' + name] = planes.max(axis=(1, 2))


def main():
    ref = load_reference()
    out = {'lbda': LBDA, 'D': np.array(D), 'crop': np.array(CROP)}
    # a, b, e: dim 256, MUSE pupil
    dim = 256
    psd = ref_psd(ref, dim, out, 'psd256')
    pup = ref.pupil_mask(dim / 4, dim / 2, oc=0.14)
    ph = static_phase(pup.shape[0])
    out.update(pup_muse256=pup.astype(np.int8), phase_b=ph.astype(np.float32))
    psf_a = np.array([ref.psd_to_psf(psd, pup, D, lb, samp=2, FoV=fov_psf_muse(dim, lb)) for lb in LBDA])
    n = psf_a.shape[-1]
    mirror = np.roll(psf_a[:, ::-1, ::-1], 1, axis=(1, 2))          # PSF[-i][-j]
    assert np.abs(mirror - psf_a).max() < 1e-14 * psf_a.max()
    out['psf_a_half'] = psf_a[:, :n // 2 + 1]
    psf_b = [ref.psd_to_psf(psd, pup, D, lb, phase_static=ph, samp=2, FoV=fov_psf_muse(dim, lb)) for lb in LBDA]
    _keep_crop(out, 'b', psf_b)
    out['maxdiff_ab'] = np.array(np.abs(np.array(psf_b) - psf_a).max())
    e = [ref.psd_to_psf(psd, pup, D, lb, samp=2, return_all=True) for lb in LBDA]
    for r, want in zip(e, psf_a):         # the same arithmetic as case a: only sampout and FoV are kept
        assert np.array_equal(r[0], want)
    out['sampout_e'] = np.array([r[1] for r in e])
    out['fov_e'] = np.array([r[2] for r in e])
    # c, d: dim 512
    dim = 512
    psd = ref_psd(ref, dim, out, 'psd512')
    pup_c = ref.pupil_mask(64, 128, oc=0.14)
    pup_d = spider_pupil(ref, 256)
    out['pup_c'] = pup_c.astype(np.int8)
    num = np.round(pup_d * 4096)
    assert np.array_equal(num / 4096, pup_d)
    out['pup_d_4096'] = num.astype(np.uint16)
    for name, p in (('c', pup_c), ('d', pup_d)):
        planes = [ref.psd_to_psf(psd, p, D, lb, samp=2) for lb in LBDA]
        out['dimnum_' + name] = np.array(planes[0].shape[0])
        _keep_crop(out, name, planes)
    # helpers
    for i, args in enumerate([(10, 32, 0.2, False), (7.5, 20, 0, True), (64, 128, 0.14, False),
                              (256 / 4, 256 / 2, 0.14, False)]):
        out['pupil_mask_args%d' % i] = np.array(args[:3], dtype=float)
        out['pupil_mask_inv%d' % i] = np.array(args[3])
        out['pupil_mask%d' % i] = ref.pupil_mask(*args[:3], inverse=args[3]).astype(np.int8)
    rng = np.random.default_rng(8)
    arr = rng.uniform(0, 1, (24, 24))
    out['arr'] = arr
    out['crop_out'] = ref.crop(arr, 12, 5)
    pos = np.mgrid[:40, :40] * 23 / 40
    out['interp_pos'] = pos
    out['interp_out'] = ref.interpolate(arr, pos, method='linear')
    pts = rng.uniform(0, 23, (2, 7, 5))
    out['interp_pts'] = pts
    out['interp_pts_out'] = ref.interpolate(arr, pts, method='linear')
    see = np.array([0.6, 1.0, 1.7])
    out['s2r_seeing'] = see
    out['s2r_out'] = np.array([ref.seeing2r01(see, lb, z) for lb, z in ((0.5, 0.0), (0.7, 30.0), (0.93, 45.0))])
    out['s2r_args'] = np.array([(0.5, 0.0), (0.7, 30.0), (0.93, 45.0)])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))


if __name__ == '__main__':
    main()
