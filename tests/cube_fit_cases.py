"""The cube the CPU and GPU tests of mpsfr_fit_cube_psf share, and its per-layer yardsticks.

cube() builds on frame_fit_ref.scene(): its 97 x 150 frame, its 34 stars, their origins, shifts and model indices, in
NL = 5 layers (no multiple of the batch of 2 the GPU tests use):
  models       layer l takes render_ref.models() rotated by l -- psf[i, l] = models[(i - l) % 4] -- so every star has a
               different PSF in every layer; psf is (4, NL, 40, 40), the layout of the call.  The models of layer 4 are
               also 1.6 times as wide (models_of_layer says why)
  layer_shift  (0.11 l, -0.07 l) px: the shift of star k in layer l is shift[k] + layer_shift[l], one rounded addition
  data         every layer rendered afresh at those shifts with its own fluxes (layer l: uniform in 200 .. 5000 times
               FLUX_SCALE[l]) and its own noise seed; sky, variance, NaN pixels and the dark star as in the scene
  layer 3      all NaN: nothing fitted, head status 2, the residual a copy of the layer
  layer 1      the disc of chain star MASKED also NaN: that star is status 2 there and status 0 in every other layer
reference(l, with_var, background) is frame_fit_ref.solve on layer l with the summed shifts, computed once.
layer_call(c, l, ...) are the contiguous inputs mpsfr_fit_frame_psf takes for layer l: what the cube call must equal.
"""
import numpy as np

import frame_fit_ref as F
import render_ref as Y

NL = 5
NAN_LAYER = 3
MASK_LAYER = 1
MASKED = 2                                     # a star of the chain
FLUX_SCALE = (1.0, 0.05, 4.0, 1.0, 0.3)        # the layers differ in brightness ...
WIDTH = (1.0, 1.0, 1.0, 1.0, 1.6)              # ... and the last one in the width of its models: see models_of_layer
FITTED = [l for l in range(NL) if l != NAN_LAYER]
RADIUS = 8.0
_CUBE = {}
_REF = {}


def layer_shifts(nl=NL):
    l = np.arange(nl, dtype=np.float64)
    return np.stack([0.11 * l, -0.07 * l], axis=1)


def models_of_layer(l, nl=NL):
    """render_ref.models() rotated by l.  Brightness alone does not move the iteration counts of the yardstick (22 on
    every layer: they follow the overlaps, which the geometry fixes), so the models of the last layer of the shared
    cube are also 1.6 times as wide -- its stars overlap more and its solve takes more steps."""
    base = Y.models()
    width = WIDTH[l] if nl == NL else 1.0
    if width != 1.0:
        ps = np.array([Y.R.moffat(20.0, 20.0, 3.0 * width, 2.5), Y.R.moffat(19.5, 19.5, 4.5 * width, 3.0),
                       Y.R.moffat(20.0, 19.5, 2.2 * width, 2.0), Y.R.moffat(19.5, 20.0, 6.0 * width, 3.5)])
        base = ps / ps.sum(axis=(1, 2))[:, None, None]
    return np.roll(base, l, axis=0)


def cube():
    """dict(cube, var (NL, 97, 150), psf (4, NL, 40, 40), index, origin, shift, layer_shift (NL, 2), flux (NL, n), n)."""
    if _CUBE:
        return _CUBE
    s = F.scene()
    n, shape = s['n'], F.FRAME
    psf = np.stack([models_of_layer(l) for l in range(NL)], axis=1)
    assert psf.shape == (4, NL, F.NS, F.NS) and np.array_equal(psf[1, 2], Y.models()[3])
    ls = layer_shifts()
    lit = np.arange(n) != s['dark']
    data, var, flux = np.empty((NL,) + shape), np.empty((NL,) + shape), np.empty((NL, n))
    for l in range(NL):
        rng = np.random.default_rng(100 + l)
        flux[l] = rng.uniform(200, 5000, n) * FLUX_SCALE[l]
        sh = s['shift'] + ls[l]
        model, _, _ = Y.render(None, np.ascontiguousarray(psf[:, l]), s['index'][lit], s['origin'][lit], sh[lit],
                               flux[l][lit], shape=shape)
        var[l] = 4.0 + model / 2.0
        data[l] = model + F.SKY + rng.normal(size=shape) * np.sqrt(var[l])
        data[l][rng.uniform(size=shape) < 0.01] = np.nan
        cy, cx = int(round(s['pos'][s['dark']][0])), int(round(s['pos'][s['dark']][1]))
        data[l][max(cy - 10, 0):cy + 11, max(cx - 10, 0):cx + 11] = np.nan
        if l == MASK_LAYER:                    # the star's own disc in this layer, and no pixel more
            data[l][F.disc(shape, F.centre(s['origin'][MASKED], sh[MASKED]), RADIUS)] = np.nan
    data[NAN_LAYER] = np.nan
    _CUBE.update(cube=data, var=var, psf=psf, index=s['index'], origin=s['origin'], shift=s['shift'], layer_shift=ls,
                 flux=flux, n=n, off=s['off'], dark=s['dark'])
    return _CUBE


def layer_call(c, l, with_var=True, with_layer_shift=True, scale0=None):
    """(image, psf, origin, keywords) of Context.fit_frame_psf for layer l of the cube dict c."""
    shift = c['shift'] + c['layer_shift'][l] if with_layer_shift else c['shift']
    kw = dict(var=np.ascontiguousarray(c['var'][l]) if with_var else None, shift=shift, psf_index=c['index'],
              scale0=None if scale0 is None else np.ascontiguousarray(scale0[l]))
    return np.ascontiguousarray(c['cube'][l]), np.ascontiguousarray(c['psf'][:, l]), c['origin'], kw


def reference(l, with_var=True, background=True, radius=RADIUS):
    """frame_fit_ref.solve of layer l at the summed shifts, once per case."""
    key = (l, with_var, background, radius)
    if key not in _REF:
        c = cube()
        _REF[key] = F.solve(c['cube'][l], c['var'][l] if with_var else None, np.ascontiguousarray(c['psf'][:, l]),
                            c['index'], c['origin'], c['shift'] + c['layer_shift'][l], radius, background)
    return _REF[key]


def lattice(nl=2):
    """289 stars on a jittered 17 x 17 lattice of 3 px pitch in an 80 x 80 frame, dense enough that a tile's list
    passes the 256 entries the renderer sorts in LDS; nl layers of different fluxes, the models rotated by layer."""
    rng = np.random.default_rng(16)
    g = 16.0 + 3.0 * np.arange(17)
    pos = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2) + rng.uniform(-0.8, 0.8, (289, 2))
    origin = (np.rint(pos) - F.NS // 2).astype(np.int32)
    shift = pos - (origin + F.NS // 2)
    index = (np.arange(289) % 4).astype(np.int32)
    base = Y.models()
    psf = np.stack([np.roll(base, l, axis=0) for l in range(nl)], axis=1)
    shape = (80, 80)
    data, var = np.empty((nl,) + shape), np.empty((nl,) + shape)
    for l in range(nl):
        flux = rng.uniform(300.0, 3000.0, 289) * (1.0 + 3.0 * l)
        model, _, _ = Y.render(None, np.ascontiguousarray(psf[:, l]), index, origin, shift, flux, shape=shape)
        var[l] = 4.0 + model / 2.0
        data[l] = model + F.SKY + rng.normal(size=shape) * np.sqrt(var[l])
    return dict(cube=data, var=var, psf=psf, index=index, origin=origin, shift=shift, layer_shift=None, n=289)


def longest_tile_list(origin, shape, tile=32):
    """The length of the longest per-tile star list of the renderer, from the geometry: a star is on every tile its
    footprint (the stamp and APRON pixels around it, cut to the frame) meets."""
    ny, nx = shape
    count = np.zeros(((ny + tile - 1) // tile, (nx + tile - 1) // tile), dtype=int)
    for o in origin:
        y0, y1, x0, x1 = Y.footprint(shape, o)
        if y0 < y1 and x0 < x1:
            count[y0 // tile:(y1 - 1) // tile + 1, x0 // tile:(x1 - 1) // tile + 1] += 1
    return int(count.max())
