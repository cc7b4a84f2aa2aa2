"""fp64 reference of the per-wavelength stage alone (NumPy only).  TEST INFRASTRUCTURE.

The stage turns the stored structure function D_phi0 of a task -- the transposed half plane
[ndir][dim/2+1][dim] that `Context.debug_fetch('dphi0', ...)` hands out -- into the 40 x 40 stamps before the
convolutions (psf_muse, psfrec.py:644-686).  `stamps_from_dphi0` does the same from the same plane in
float64 / complex128: the plane completed by D[-u][-v] = D[u][v], the oracle's exact telescope OTF (not the
library's `log2 tel` table, whose error is thereby charged to the library), OTF = tel . sum_d exp(-1/2 (2 pi /
lambda)^2 D_d), stamp = Re(G OTF G^T) with the oracle's sampling matrix, clamped at 0 and divided by its sum
(psfrec.py:682-685).  Nothing here is pruned, tiered or split: what a kernel loses to any of these is its error
against this function.
"""
import functools

import numpy as np

import psfr_oracle as O
from conftest import H


@functools.lru_cache(maxsize=8)
def _tel(dim):
    t = O.telescope_otf(dim)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=64)
def _sample_matrix(dim, npixc, dimpsf):
    g = O.sample_matrix(dim, npixc, dimpsf)
    g.setflags(write=False)
    return g


def full_plane(d0t, dim):
    """[ndir][dim/2+1][dim] transposed half plane (d0t[d][v][u] = D_d[u][v], v <= dim/2) -> D [ndir][dim][dim] in
    the oracle's layout, the other half by D[u][v] = D[-u][-v]."""
    d0t = np.asarray(d0t, dtype=np.float64)
    if d0t.ndim == 2:
        d0t = d0t[None]
    nh = dim // 2 + 1
    if d0t.shape[1:] != (nh, dim):
        raise ValueError('dphi0 must be [ndir][%d][%d], got %s' % (nh, dim, d0t.shape))
    D = np.empty((d0t.shape[0], dim, dim))
    D[:, :, :nh] = np.swapaxes(d0t, 1, 2)
    mu = (-np.arange(dim)) % dim
    v = np.arange(nh, dim)
    D[:, :, nh:] = D[:, mu][:, :, dim - v]
    return D


def transposed_half_plane(d0, dim):
    """The inverse view: the oracle's D [ndir][dim][dim] (or [dim][dim]) as the library stores it."""
    d0 = np.asarray(d0, dtype=np.float64)
    if d0.ndim == 2:
        d0 = d0[None]
    return np.ascontiguousarray(np.swapaxes(d0, 1, 2)[:, :dim // 2 + 1, :])


def stamps_from_dphi0(d0t, dim, lbda_nm, pixscale, dimpsf=40):
    """(nl, dimpsf, dimpsf) float64 stamps of one task from its stored structure function (see the module text)."""
    lbda_nm = np.atleast_1d(np.asarray(lbda_nm, dtype=np.float64))
    D = full_plane(d0t, dim)
    tel = _tel(dim)
    npixc = O.npix_crop(lbda_nm, dimpsf, pixscale)
    if npixc.max() > dim:
        raise ValueError('grid too small: npixc=%d > dim=%d' % (npixc.max(), dim))
    out = np.empty((lbda_nm.size, dimpsf, dimpsf))
    for k, lb in enumerate(lbda_nm):
        s = (2.0 * np.pi / lb) ** 2
        otf = tel * np.exp(-0.5 * s * D).sum(axis=0)
        G = _sample_matrix(dim, int(npixc[k]), dimpsf)
        st = np.maximum((G @ otf.astype(np.complex128) @ G.T).real, 0.0)
        out[k] = st / st.sum()
    return out


def stamp_errors(got, want):
    """max |got - want| / peak of `want`, per stamp: arrays (..., dimpsf, dimpsf) -> (...)."""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want).max(axis=(-2, -1)) / want.max(axis=(-2, -1))


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _tables(three, npl):
    return O.ao_tables(H, bool(three), npl, exact_masks=True)


def model_psd(dim, seeing, gl, l0, npl=1, three=False):
    """(npl^2, dim, dim) PSD of the atmosphere model, centred as the oracle and `psf_from_psd` take it."""
    return O.residual_psd([gl, 1 - gl], H, seeing, l0, npl, dim, bool(three), tables=_tables(bool(three), npl))


def ridge_psd(dim=256):
    """The non-model PSD of test_psf_muse_takes_any_psd: a bump off the axes and a tilted ridge, no symmetry
    between the rows su and -1-su."""
    psd = model_psd(dim, 0.9, 0.6, 18.0)[0]
    yy, xx = np.mgrid[:dim, :dim] - dim // 2
    return psd * (1.0 + 0.3 * np.exp(-((xx - 7) ** 2 + (yy + 3) ** 2) / 50.0)
                  + 0.2 * (np.hypot(xx, yy) > 20) * (xx > 2 * yy))


def wavelengths_for_grid(dim, pixscale, dimpsf=40):
    """Four wavelengths [nm] that reach the edges of the sampling on this grid, chosen from O.npix_crop:
    (the shortest the grid admits: npix_crop = dim, the crop wraps round the whole grid;
     npix_crop a multiple of dimpsf: every bilinear weight a_i = 0;
     npix_crop = multiple of dimpsf + 2: npix_crop / dimpsf just above an integer, weights i / 20 mod 1;
     930 nm)."""
    k = dimpsf * pixscale * 2 * 8 * 4.85 * 1000        # npix_crop = 2 round(k / lbda / 2)

    def lam(npc):                                      # the middle of the wavelengths that give npix_crop = npc
        lb = k / npc
        assert O.npix_crop(np.array([lb]), dimpsf, pixscale)[0] == npc, (npc, lb)
        return lb
    shortest = lam(dim)
    lo = int(O.npix_crop(np.array([930.0]), dimpsf, pixscale)[0])
    mult = [n for n in range(lo + 2, dim - 2, 2) if n % dimpsf == 0]
    whole = mult[len(mult) // 2]
    out = np.array([shortest, lam(whole), lam(whole + 2), 930.0])
    npc = O.npix_crop(out, dimpsf, pixscale)
    assert npc[1] % dimpsf == 0 and npc[2] % dimpsf == 2 and npc.max() <= dim, npc
    return out


def wavelength_set(dim, pixscale, nl):
    """nl wavelengths for this grid, ascending: the shortest it admits alone (nl = 1), with npix_crop a multiple of 40
    and 930 nm (nl = 3), or the four of wavelengths_for_grid and an even fill between them (nl >= 4)."""
    sp = wavelengths_for_grid(dim, pixscale)
    if nl == 1:
        lb = sp[:1]
    elif nl == 3:
        lb = sp[[0, 1, 3]]
    else:
        lb = np.sort(np.concatenate([sp, np.linspace(sp[0] * 1.03, 921.0, nl - 4)]))
    assert lb.size == nl
    return lb


def telescope_support(dim):
    """[dim][dim] mask of the telescope OTF's support (outside it the exact OTF is rounding noise of 1e-17)."""
    return _tel(dim) > 1e-9


def ladder_scales(d0, lbda_nm, targets, support):
    """Factors s such that min over `support` of -1/2 (2 pi / lbda)^2 (s d0) log2 e equals each target (< 0)."""
    c2 = -0.5 * (2 * np.pi / lbda_nm) ** 2 * np.log2(np.e)
    dmax = float(np.asarray(d0)[..., support].max())
    return [t / (c2 * dmax) for t in targets]
