"""NumPy yardstick of the frame calls (mpsfr_cut_stamps, mpsfr_render_stars, include/mpsfr.h) and the scenes the CPU and
GPU tests share.

render: the stars in index order; star k adds (or subtracts) scale_k keys(t_y) @ P_k @ keys(t_x).T on its footprint, the
60 x 60 window around its stamp (rows origin_p - 10 .. origin_p + 49), clipped to the frame; keys is psf_fit_ref.keys,
t_y[p, j] = p - dp - j over the window rows p = -10 .. 49 and the 40 model rows j.  cut: plain slicing.
"""
import numpy as np

import psf_fit_ref as R

NS = R.NS
APRON = 10
SIDE = NS + 2 * APRON
TILE = 32                      # the renderer's frame tile; only used to place stars on borders


def window(psf, dp, dq):
    """P~(p - dp, q - dq) on the window p, q = -10 .. 49."""
    p = np.arange(-APRON, NS + APRON)[:, None]
    j = np.arange(NS)[None, :]
    return R.keys(p - dp - j) @ psf @ R.keys(p - dq - j).T


def footprint(shape, origin):
    """(y0, y1, x0, x1): the frame pixels inside the footprint of a star at `origin`; empty if y0 >= y1 or x0 >= x1."""
    ny, nx = shape
    op, oq = int(origin[0]), int(origin[1])
    return max(op - APRON, 0), min(op + NS + APRON, ny), max(oq - APRON, 0), min(oq + NS + APRON, nx)


def render(image_in, psf, psf_index, origin, shift, scale, subtract=False, shape=None):
    """(frame, npix, S): the rendered frame, the number of frame pixels in every star's footprint, and the magnitude
    S = |image_in| + sum over the stars reaching a pixel of |scale_k| max|P_k| of the parity tolerance."""
    out = np.zeros(shape) if image_in is None else np.array(image_in, dtype=float)
    S = np.abs(out)
    n = len(origin)
    npix = np.zeros(n, dtype=int)
    for k in range(n):
        P = psf[k if psf_index is None else psf_index[k]]
        dp, dq = (0.0, 0.0) if shift is None else shift[k]
        y0, y1, x0, x1 = footprint(out.shape, origin[k])
        if y0 >= y1 or x0 >= x1:
            continue
        npix[k] = (y1 - y0) * (x1 - x0)
        w = window(P, dp, dq)
        wy, wx = y0 - (int(origin[k][0]) - APRON), x0 - (int(origin[k][1]) - APRON)
        t = scale[k] * w[wy:wy + y1 - y0, wx:wx + x1 - x0]
        if subtract:
            out[y0:y1, x0:x1] -= t
        else:
            out[y0:y1, x0:x1] += t
        S[y0:y1, x0:x1] += abs(scale[k]) * np.abs(P).max()
    return out, npix, S


def cut(image, var, origin, ns=NS):
    """(stamps, var_stamps or None) by slicing: NaN (0) off the frame."""
    ny, nx = image.shape
    n = len(origin)
    st = np.full((n, ns, ns), np.nan)
    vs = None if var is None else np.zeros((n, ns, ns))
    for k in range(n):
        op, oq = int(origin[k][0]), int(origin[k][1])
        y0, y1, x0, x1 = max(op, 0), min(op + ns, ny), max(oq, 0), min(oq + ns, nx)
        if y0 >= y1 or x0 >= x1:
            continue
        st[k, y0 - op:y1 - op, x0 - oq:x1 - oq] = image[y0:y1, x0:x1]
        if var is not None:
            vs[k, y0 - op:y1 - op, x0 - oq:x1 - oq] = var[y0:y1, x0:x1]
    return st, vs


def models():
    """Four distinct Moffat model stamps, sum 1."""
    ps = np.array([R.moffat(20.0, 20.0, 3.0, 2.5), R.moffat(19.5, 19.5, 4.5, 3.0), R.moffat(20.0, 19.5, 2.2, 2.0),
                   R.moffat(19.5, 20.0, 6.0, 3.5)])
    return ps / ps.sum(axis=(1, 2))[:, None, None]


PILE = 300                     # stars of the pile: more than the renderer sorts in LDS (RENDER_SORT_CHUNK)
FRAME = (97, 150)
_SCENE = {}


def scene(offset=(0, 0), shape=FRAME):
    """The parity scene on a 97 x 150 frame (no multiple of the tile, several tiles each way): 64 stars on four models
    -- 54 at random with their footprints on the frame (a 60-pixel footprint straddles at least one tile border each
    way, and the 54 straddle every border of the frame's tile grid: asserted here), one on each of the four edges, two
    on corners, one whose footprint touches the frame with a single row, three wholly off the frame -- then a pile of
    300 stars within +-4 px of one point.  Shifts uniform in +-8, scales in +-1000.  image_in: Gaussian noise with 1 %
    NaN pixels.  `offset` moves every origin (in a frame of `shape`).  Returns a dict."""
    key = (tuple(offset), tuple(shape))
    if key in _SCENE:
        return _SCENE[key]
    rng = np.random.default_rng(2024)
    ny, nx = FRAME
    org = [(int(rng.integers(-30, 81)), int(rng.integers(-30, 131))) for _ in range(54)]
    org += [(-30, 50), (80, 50), (30, -30), (30, 130), (-30, -30), (80, 130), (-49, 30)]
    off_frame = [(-50, 20), (ny + APRON, 20), (20, nx + APRON + 1000)]
    org += off_frame
    assert len(org) == 64
    org = [org[i] for i in rng.permutation(64)]
    org += [(30 + int(a), 60 + int(b)) for a, b in rng.integers(-4, 5, (PILE, 2))]
    origin = np.array(org, dtype=np.int32)
    for axis, n in ((0, ny), (1, nx)):                       # every tile border has a footprint across it
        for border in range(TILE, n, TILE):
            lo = origin[:64, axis] - APRON
            assert np.any((lo < border) & (lo + SIDE > border)), (axis, border)
    n = len(origin)
    shift, scale = rng.uniform(-8, 8, (n, 2)), rng.uniform(-1000, 1000, n)
    image = rng.normal(size=FRAME)
    image[rng.uniform(size=FRAME) < 0.01] = np.nan
    if tuple(shape) != FRAME:
        big = rng.normal(size=shape)
        big[offset[0]:offset[0] + ny, offset[1]:offset[1] + nx] = image
        image = big
    s = dict(image=image, psf=models(), index=(np.arange(n) % 4).astype(np.int32),
             origin=origin + np.array(offset, dtype=np.int32), shift=shift, scale=scale,
             off_frame=[org.index(o) for o in off_frame], n=n)
    _SCENE[key] = s
    return s


_REF = {}


def scene_reference(subtract):
    """render() of the parity scene, computed once per mode."""
    if subtract not in _REF:
        s = scene()
        _REF[subtract] = render(s['image'], s['psf'], s['index'], s['origin'], s['shift'], s['scale'], subtract)
    return _REF[subtract]


def longest_tile_list(s, shape=FRAME):
    """The largest number of stars whose footprint reaches one 32 x 32 tile of the frame."""
    nty, ntx = -(-shape[0] // TILE), -(-shape[1] // TILE)
    count = np.zeros((nty, ntx), dtype=int)
    for o in s['origin']:
        y0, y1, x0, x1 = footprint(shape, o)
        if y0 < y1 and x0 < x1:
            count[y0 // TILE:(y1 - 1) // TILE + 1, x0 // TILE:(x1 - 1) // TILE + 1] += 1
    return int(count.max())
