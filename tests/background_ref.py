"""NumPy restatement of mpsfr_frame_background (include/mpsfr.h), written literally: the sort-based med, the pass loop of
a cell, filter and fill, the linear continuation of the mesh and the Keys taps; the a-priori bound of the interpolated
maps; the scenes the host and the GPU tests share.  mesh and head have no rounding freedom and are compared bit for bit.
fill_plan states a second time, from ring membership alone, which valid cells a cell's level and rms come from: the
certificates of tests/background_cases.py are read from it.
"""
import functools

import numpy as np

EPS = 2.0 ** -53
NBACK, NHEAD = 8, 4
FILLED, CLIP_CAP, FLAT = 1, 2, 4
MAD_TO_SIGMA = 1.4826
FRAME = (97, 150)
DEFAULTS = dict(box=32, filter=3, kappa=3.0, max_clip=5, min_frac=0.25)


def med(v):
    """v[(n-1)/2] of the ascending values for odd n, 0.5 v[n/2-1] + 0.5 v[n/2] for even n."""
    s = np.sort(np.asarray(v, dtype=np.float64))
    n = len(s)
    if n % 2:
        return s[(n - 1) // 2]
    return np.float64(0.5) * s[n // 2 - 1] + np.float64(0.5) * s[n // 2]


def valid_pixels(image, var=None):
    ok = np.isfinite(image)
    if var is not None:
        with np.errstate(invalid='ignore'):
            ok &= np.isfinite(var) & (var > 0)
    return ok


def cell_estimate(x, npix, kc, max_clip, min_frac):
    """The row columns 2 .. 7 of one cell from its valid pixels x (any order) and its number of pixels on the frame."""
    x = np.asarray(x, dtype=np.float64) + 0.0
    n_valid = len(x)
    if not (n_valid >= 1 and float(n_valid) >= np.float64(min_frac) * np.float64(npix)):
        return [np.nan, np.nan, 0.0, float(n_valid), 0.0, float(FILLED)]
    p, flags = 0, 0
    with np.errstate(over='ignore', invalid='ignore'):
        while True:
            m = med(x)
            d = np.abs(x - m)
            mad = med(d)
            if p == max_clip:
                flags |= CLIP_CAP
            if mad == 0.0:
                flags |= FLAT
            if flags:
                break
            t = np.float64(kc) * mad
            keep = d <= t
            if keep.all():
                break
            x = x[keep]
            p += 1
        return [m, np.float64(MAD_TO_SIGMA) * mad, float(len(x)), float(n_valid), float(p), float(flags)]


def mesh_shape(ny, nx, box):
    return -(-ny // box), -(-nx // box)


def layer_mesh(image, var, box, filter, kappa, max_clip, min_frac):
    """(mesh (my, mx, 8), head (4,)) of one layer."""
    ny, nx = image.shape
    my, mx = mesh_shape(ny, nx, box)
    ok = valid_pixels(image, var)
    kc = np.float64(kappa) * np.float64(MAD_TO_SIGMA)
    mesh = np.zeros((my, mx, NBACK))
    for i in range(my):
        for j in range(mx):
            sl = (slice(i * box, min((i + 1) * box, ny)), slice(j * box, min((j + 1) * box, nx)))
            mesh[i, j, 2:] = cell_estimate(image[sl][ok[sl]], ok[sl].size, kc, max_clip, min_frac)
    good = (mesh[:, :, 7].astype(int) & FILLED) == 0
    h = (filter - 1) // 2
    for i in range(my):
        for j in range(mx):
            r = h
            while True:
                sl = (slice(max(i - r, 0), i + r + 1), slice(max(j - r, 0), j + r + 1))
                w = good[sl]
                if w.any() or not r < max(my, mx):
                    break
                r += 1
            if w.any():
                mesh[i, j, 0] = med(mesh[:, :, 2][sl][w])
                mesh[i, j, 1] = med(mesh[:, :, 3][sl][w])
            else:
                mesh[i, j, :2] = np.nan
    nvalid = int(good.sum())
    head = np.array([0.0 if nvalid == my * mx else 1.0 if nvalid else 2.0, nvalid, my * mx - nvalid, 0.0])
    return mesh, head


def fill_plan(good, filter):
    """Where every cell of a layer's mesh takes its level and rms from, written from ring membership alone (not from
    layer_mesh's slices): plan[i][j] = (radius used, [(i', j') of the valid cells found at that radius]).  `good` (my, mx)
    marks the valid cells.  Radius h = (filter - 1) / 2 stands for the filter window, the whole square
    max(|di|, |dj|) <= h; a cell whose window holds no valid cell takes the ring max(|di|, |dj|) == r of the first
    r = h + 1 .. max(my, mx) that holds one.  (None, []) in a layer without a valid cell."""
    good = np.asarray(good, dtype=bool)
    my, mx = good.shape
    h = (filter - 1) // 2
    live = [(int(a), int(b)) for a, b in zip(*np.nonzero(good))]
    plan = [[(None, []) for _ in range(mx)] for _ in range(my)]
    for i in range(my):
        for j in range(mx):
            dist = [max(abs(a - i), abs(b - j)) for a, b in live]
            window = [c for c, d in zip(live, dist) if d <= h]
            if window:
                plan[i][j] = (h, window)
                continue
            for r in range(h + 1, max(my, mx) + 1):
                ring = [c for c, d in zip(live, dist) if d == r]
                if ring:
                    plan[i][j] = (r, ring)
                    break
    return plan


def keys_weights(t):
    """The four Keys weights c(t+1), c(t), c(t-1), c(t-2) as the library evaluates them, and the sums of the absolute
    values of their monomials (for the bound)."""
    t2 = t * t
    t3 = t2 * t
    w = np.stack([0.5 * (-t3 + 2.0 * t2 - t), 0.5 * (3.0 * t3 - 5.0 * t2 + 2.0), 0.5 * (-3.0 * t3 + 4.0 * t2 + t),
                  0.5 * (t3 - t2)], axis=-1)
    a = np.stack([0.5 * (t3 + 2.0 * t2 + t), 0.5 * (3.0 * t3 + 5.0 * t2 + 2.0), 0.5 * (3.0 * t3 + 4.0 * t2 + t),
                  0.5 * (t3 + t2)], axis=-1)
    return w, a


def axis_taps(n, box):
    """For the n pixels of an axis: i0 (n,), the weights (n, 4) and their monomial sums (n, 4)."""
    u = (np.arange(n, dtype=np.float64) + 0.5) / np.float64(box) - 0.5
    i0 = np.floor(u)
    w, a = keys_weights(u - i0)
    return i0.astype(int), w, a


def extend(M, absolute=False):
    """The plane M (my, mx) continued linearly by two nodes each way, columns first, then rows: (my + 4, mx + 4), node
    (i, j) at [i + 2, j + 2].  absolute: the same expressions over absolute values, an upper bound of every term."""
    def along(P):                                                        # continues the last axis
        m = P.shape[-1]
        if m == 1:
            return np.repeat(P, 5, axis=-1)
        lo, lo1, hi, hi1 = P[..., 0], P[..., 1], P[..., m - 1], P[..., m - 2]
        step_lo = (np.abs(lo) + np.abs(lo1)) if absolute else (lo - lo1)
        step_hi = (np.abs(hi) + np.abs(hi1)) if absolute else (hi - hi1)
        left = [lo + np.float64(j) * step_lo for j in (2, 1)]
        right = [hi + np.float64(j) * step_hi for j in (1, 2)]
        return np.concatenate([np.stack(left, -1), P, np.stack(right, -1)], axis=-1)
    with np.errstate(invalid='ignore', over='ignore'):
        P = np.abs(M) if absolute else M
        return along(along(P).T).T


def interpolate(M, ny, nx, box):
    """(map (ny, nx), bound (ny, nx)) of the plane M on the mesh nodes: rows outer, columns inner, both ascending.
    bound, a priori: (16 + 2) eps sum |w_y w_x E| for the products and the sums; the weights' own rounding to first
    order -- a weight is a cubic whose monomials see at most 6 roundings (t^2, t^3, the coefficient, three sums; the
    factor 0.5 is exact), so |dw| <= 6 eps A with A the sum of its absolute monomials --; and 6 eps of the continued
    nodes' absolute terms (three roundings per continuation, two continuations at a corner)."""
    iy, wy, ay = axis_taps(ny, box)
    ix, wx, ax = axis_taps(nx, box)
    E, Eabs = extend(M), extend(M, absolute=True)
    my, mx = M.shape
    out = np.zeros((ny, nx))
    terms = np.zeros((ny, nx))
    wterm = np.zeros((ny, nx))
    eterm = np.zeros((ny, nx))
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(4):
            r = iy - 1 + a + 2
            inner = np.zeros((ny, nx))
            outside_r = ((r < 2) | (r >= my + 2))[:, None]
            for b in range(4):
                c = ix - 1 + b + 2
                e = E[r][:, c]
                inner = inner + wx[None, :, b] * e
                ea = np.abs(e)
                terms += np.abs(wy[:, None, a] * wx[None, :, b]) * ea
                wterm += (ay[:, None, a] * np.abs(wx[None, :, b]) + np.abs(wy[:, None, a]) * ax[None, :, b]) * ea
                outside = outside_r | ((c < 2) | (c >= mx + 2))[None, :]
                eterm += np.where(outside, np.abs(wy[:, None, a] * wx[None, :, b]) * Eabs[r][:, c], 0.0)
            out = out + wy[:, None, a] * inner
    bound = 18 * EPS * terms + 6 * EPS * wterm + 6 * EPS * eterm
    return out, bound


def background(image, var=None, *, box=32, filter=3, kappa=3.0, max_clip=5, min_frac=0.25, apply_to=None):
    """The whole call on a frame (ny, nx) or a cube (nl, ny, nx).  Returns a dict: mesh (nl, my, mx, 8), head (nl, 4),
    map, rms, applied (or None) of the input's shape and the bounds map_bound, rms_bound."""
    image = np.asarray(image, dtype=np.float64)
    cube = image.reshape((-1,) + image.shape[-2:])
    vcube = None if var is None else np.asarray(var, dtype=np.float64).reshape(cube.shape)
    nl, ny, nx = cube.shape
    res = dict(mesh=[], head=[], map=[], rms=[], map_bound=[], rms_bound=[])
    for layer in range(nl):
        mesh, head = layer_mesh(cube[layer], None if vcube is None else vcube[layer], box, filter, kappa, max_clip, min_frac)
        level, lb = interpolate(mesh[:, :, 0], ny, nx, box)
        rms, rb = interpolate(mesh[:, :, 1], ny, nx, box)
        with np.errstate(invalid='ignore'):
            rms = np.where(rms < 0.0, 0.0, rms)
        for k, v in zip(('mesh', 'head', 'map', 'rms', 'map_bound', 'rms_bound'), (mesh, head, level, rms, lb, rb)):
            res[k].append(v)
    out = {k: np.stack(v) for k, v in res.items()}
    for k in ('map', 'rms', 'map_bound', 'rms_bound'):
        out[k] = out[k].reshape(image.shape)
    out['applied'] = None
    if apply_to is not None:
        with np.errstate(invalid='ignore'):
            out['applied'] = np.asarray(apply_to, dtype=np.float64).reshape(image.shape) - out['map']
    return out


# ---- the shared scenes
@functools.lru_cache(maxsize=None)
def scene():
    """The 97 x 150 frame of the parity tests: a gradient, unit noise, a few dozen compact sources above it, a NaN
    block that kills two cells at box 16, +-inf and NaN pixels, zeros of both signs, and a variance plane that masks a
    tile and a scatter of pixels.  Returns a dict: image, var, apply."""
    rng = np.random.default_rng(2028)
    ny, nx = FRAME
    Y, X = np.mgrid[:ny, :nx]
    image = 10.0 + 0.05 * Y - 0.03 * X + rng.normal(size=FRAME)
    for _ in range(40):
        y, x, f = rng.uniform(0, ny), rng.uniform(0, nx), rng.uniform(20, 400)
        image += f * np.exp(-0.5 * ((Y - y) ** 2 + (X - x) ** 2) / 1.5 ** 2)
    image[30:66, 40:75] = np.nan
    image[3, 5], image[80, 140], image[50, 10] = np.inf, -np.inf, np.nan
    image[90, 20:24] = [0.0, -0.0, 0.0, -0.0]
    var = rng.uniform(0.5, 1.5, FRAME)
    var[64:80, 96:112] = 0.0
    var[rng.uniform(size=FRAME) < 0.02] = -1.0
    var[10, 10], var[11, 11] = np.nan, np.inf
    apply = rng.normal(size=FRAME) * 5.0
    apply[7, 7] = np.nan
    for a in (image, var, apply):
        a.setflags(write=False)
    return dict(image=image, var=var, apply=apply)


@functools.lru_cache(maxsize=None)
def scene_reference(usevar, box, filter, max_clip):
    s = scene()
    return background(s['image'], s['var'] if usevar else None, box=box, filter=filter, max_clip=max_clip,
                      apply_to=s['apply'])


def permute_cells(image, box, rng):
    """The frame with the pixels of every cell permuted inside the cell."""
    out = image.copy()
    ny, nx = image.shape[-2:]
    for i in range(0, ny, box):
        for j in range(0, nx, box):
            block = out[..., i:i + box, j:j + box]
            shape = block.shape
            flat = block.reshape(shape[:-2] + (-1,))
            out[..., i:i + box, j:j + box] = flat[..., rng.permutation(flat.shape[-1])].reshape(shape)
    return out


SKY_FRAME = (128, 160)
SKY_RADIUS = 6.0
SKY_LEVEL = 20.0
SKY_PAR = dict(box=16, filter=1, passes=2)


@functools.lru_cache(maxsize=None)
def sky_scene():
    """The scene of the sky loop: 42 stars on a jittered 20-pixel grid of the 128 x 160 frame (fluxes 300 .. 3000, the
    first model of render_ref), unit Gaussian noise, and two backgrounds under the same stars and noise: the constant
    SKY_LEVEL (`flat`) and SKY_LEVEL + 0.25 Y - 0.15 X + 0.0005 (X - 80)^2 (`image`: 50 counts across the frame, fifty
    times the noise).  Returns a dict: image, flat, sky, psf (1, 40, 40), index, origin, shift, pos, flux, n."""
    import render_ref as Y
    rng = np.random.default_rng(77)
    ny, nx = SKY_FRAME
    gy, gx = np.meshgrid(np.arange(12, ny - 8, 20.0), np.arange(12, nx - 8, 20.0), indexing='ij')
    pos = np.stack([gy.ravel(), gx.ravel()], 1) + rng.uniform(-4, 4, (gy.size, 2))
    n = len(pos)
    flux = rng.uniform(300, 3000, n)
    origin = (np.rint(pos) - Y.NS // 2).astype(np.int32)
    shift = pos - (origin + Y.NS // 2)
    psf = Y.models()[:1]
    index = np.zeros(n, dtype=np.int32)
    model, _, _ = Y.render(None, psf, index, origin, shift, flux, shape=SKY_FRAME)
    noise = rng.normal(size=SKY_FRAME)
    Yp, Xp = np.mgrid[:ny, :nx]
    sky = SKY_LEVEL + 0.25 * Yp - 0.15 * Xp + 0.0005 * (Xp - 80.0) ** 2
    return dict(image=model + noise + sky, flat=model + noise + SKY_LEVEL, sky=sky, psf=psf, index=index, origin=origin,
                shift=shift, pos=pos, flux=flux, n=n)


def sky_loop(image, fit, passes, **par):
    """The loop of fit_crowded_stars(sky=...) over a fit(frame) -> (F, residual): map_0 = 0; for p = 1 .. passes, fit
    image - map_(p-1) and add the background of its residual.  Returns (map, image - map)."""
    sky = np.zeros(image.shape)
    frame = image
    for _ in range(passes):
        sky = sky + background(fit(frame)[1], **par)['map']
        frame = image - sky
    return sky, frame
