"""The scenes that make the frame and cube calls walk past one workgroup's span of work, shared by the CPU and GPU tests,
and for every scene the facts that make it cross its constant, computed from the geometry alone.

The constants (named here by value; test_frame_span_host.py reads them out of the sources):
  STEP      1024  threads of k_ff_step / k_fr_step / k_cf_step, which loop i += 1024 over the unknowns and the layers,
                  and the summands step_sum takes per trip over the partials of k_ff_reduce
  CHUNK     4096  frame pixels per partial of k_ff_reduce
  SCAN      1024  threads of k_scan_counts: per = ceil(tiles / 1024) counts per thread
  SEGS      1024  row segments (one frame row of one 32-pixel tile column) per chunk of k_find_count / k_find_list
  ROWBLOCKS 8192  blocks of k_find_rows, which stride over the peaks
pad()             any star list inside a list of 2101 rows (three trips of 1024; a multiple of neither 64, 256 nor 1024),
                  the live stars in their order at seeded places that include both sides of every trip border
live_lattice()    33 x 33 = 1089 stars on 220 x 223: nu = 1024 and 1025 from its first 1023 and 1024 stars, 1090 from all
long_frame()      257 x 16384 = 4 210 688 px: 1028 partials of k_ff_reduce (four in the second trip), 4608 tiles (per = 5)
tile_frames()     1024 x 1024 (1024 tiles, per = 1) and 1312 x 800 (1025 tiles, per = 2)
finder_frames()   256 x 128 (1024 segments: one full chunk) and 257 x 128 (1028: four segments in chunk 1)
noise_frame()     300 x 300 of pure noise: more than 8192 peaks at sep = 1
deep_cube()       1025 layers of 12 x 12
No GPU code here.
"""
import numpy as np

import find_ref as FR
import frame_fit_ref as F
import render_ref as Y

NS = F.NS
STEP, CHUNK, SCAN, SEGS, ROWBLOCKS = 1024, 4096, 1024, 1024, 8192
TILE = Y.TILE
TOTAL = 2101
PLACES = (0, 63, 64, 255, 256, 1023, 1024, 1025, 2047, 2048, 2100)


# ---- a. padded lists
def pad(stars, shape, npsf, total=TOTAL, seed=0):
    """`stars` is a dict of per-star arrays (first axis the star; 'origin' (n, 2) int32 among them, None entries stay
    None).  Returns (padded dict of `total` rows, the places of the live rows, increasing): the live stars keep their
    order and sit at PLACES and at places default_rng(seed) spreads; every other row is a star wholly off the frame
    `shape` (status 1) -- origins on all four sides up to 1000 px away, 'index' valid in 0 .. npsf - 1, every other
    array uniform in +-0.5 (a legal shift, scale and start)."""
    n = len(stars['origin'])
    assert len(PLACES) <= n <= total and max(PLACES) < total
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(total), PLACES)
    places = np.sort(np.concatenate([np.array(PLACES), rng.choice(rest, n - len(PLACES), replace=False)]))
    ny, nx = shape
    side = rng.integers(0, 4, total)
    far = rng.integers(0, 1000, total)
    along_y, along_x = rng.integers(-100, ny + 100, total), rng.integers(-100, nx + 100, total)
    # the footprint is origin - APRON .. origin + NS + APRON: off the frame above / below / left / right
    oy = np.where(side == 0, -(NS + Y.APRON) - far, np.where(side == 1, ny + Y.APRON + far, along_y))
    ox = np.where(side == 2, -(NS + Y.APRON) - far, np.where(side == 3, nx + Y.APRON + far, along_x))
    out = {}
    for name, a in stars.items():
        if a is None:
            out[name] = None
            continue
        a = np.asarray(a)
        assert len(a) == n, name
        if name == 'origin':
            full = np.stack([oy, ox], axis=1).astype(a.dtype)
        elif name == 'index':
            full = rng.integers(0, npsf, total).astype(a.dtype)
        else:
            full = rng.uniform(-0.5, 0.5, (total,) + a.shape[1:]).astype(a.dtype)
        full[places] = a
        out[name] = full
    return out, places


def off_frame(shape, origin):
    """Which rows have a footprint that misses the frame."""
    fp = np.array([Y.footprint(shape, o) for o in origin])
    return (fp[:, 0] >= fp[:, 1]) | (fp[:, 2] >= fp[:, 3])


def pad_scene(s, names, seed):
    """A scene dict (image, psf, ...) with the per-star arrays `names` padded: (padded dict with n = TOTAL, places)."""
    p, places = pad({k: s[k] for k in names}, s['image'].shape, len(s['psf']), TOTAL, seed)
    return dict(s, n=TOTAL, **p), places


# ---- b. the live lattice
LATTICE_FRAME = (220, 223)
LATTICE_SIDE = 33
LATTICE_RADIUS = 3.0
_LATTICE = {}


def live_lattice():
    """33 x 33 = 1089 stars at a pitch of 6 px, jittered by +-1 px, on 220 x 223; the models of render_ref by k % 4,
    fluxes 300 .. 3000, sky 7, var = 4 + model / 2, Gaussian noise of that variance; default_rng(6)."""
    if not _LATTICE:
        rng = np.random.default_rng(6)
        n = LATTICE_SIDE ** 2
        g = 14.0 + 6.0 * np.arange(LATTICE_SIDE)
        pos = np.stack(np.meshgrid(g, g + 1.0, indexing='ij'), axis=-1).reshape(-1, 2) + rng.uniform(-1.0, 1.0, (n, 2))
        flux = rng.uniform(300.0, 3000.0, n)
        origin = (np.rint(pos) - NS // 2).astype(np.int32)
        shift = pos - (origin + NS // 2)
        index = (np.arange(n) % 4).astype(np.int32)
        psf = Y.models()
        model, _, _ = Y.render(None, psf, index, origin, shift, flux, shape=LATTICE_FRAME)
        var = 4.0 + model / 2.0
        image = model + F.SKY + rng.normal(size=LATTICE_FRAME) * np.sqrt(var)
        _LATTICE.update(image=image, var=var, psf=psf, index=index, origin=origin, shift=shift, flux=flux, n=n)
    return _LATTICE


def head_of(s, m):
    """The scene with its first m stars only (the frame still holds the light of all)."""
    return dict(s, index=s['index'][:m], origin=s['origin'][:m], shift=s['shift'][:m], flux=s['flux'][:m], n=m)


LATTICE_CASES = {'1023_back': (1023, True), '1024_back': (1024, True), '1089_back': (1089, True),
                 '1089_noback': (1089, False)}
_LATTICE_REF = {}


def lattice_reference(case):
    """(scene, solve_sparse of it) of a case of LATTICE_CASES, once."""
    if case not in _LATTICE_REF:
        m, back = LATTICE_CASES[case]
        s = head_of(live_lattice(), m)
        _LATTICE_REF[case] = (s, F.solve_sparse(s['image'], s['var'], s['psf'], s['index'], s['origin'], s['shift'],
                                                LATTICE_RADIUS, back))
    return _LATTICE_REF[case]


# ---- c. the long frame
LONG_FRAME = (257, 16384)
LONG_RADIUS = 8.0
LONG_FIND = dict(half=2, sep=2, threshold=15.0)
_LONG = {}


def nchunk(shape):
    return -(-(shape[0] * shape[1]) // CHUNK)


def ntiles(shape):
    return -(-shape[0] // TILE) * -(-shape[1] // TILE)


def scan_per(nt):
    return -(-nt // SCAN)


def long_frame():
    """257 x 16384: 16 stars of find_ref's model -- in the four corners (columns near 0 and 16383 on the rows 0 and
    256), three more along row 256, four whose discs lie across a multiple of 4096 in linear pixel index (x = 4096,
    8192, 12288 on any row) and five at random --, fluxes 2000 .. 5000, sky 7, var = 4 + model / 2, Gaussian noise, 1 %
    NaN pixels (none within a pixel of a star's centre); default_rng(31).  'scale' are signed scales for the renderer."""
    if not _LONG:
        rng = np.random.default_rng(31)
        ny, nx = LONG_FRAME
        pos = [(0.3, 2.4), (0.4, 16381.2), (255.8, 1.1), (255.7, 16382.3), (255.9, 8000.7), (256.0, 5000.2),
               (255.6, 12000.4), (128.5, 4096.2), (130.1, 8191.6), (64.7, 12288.4), (200.3, 4095.1)]
        pos += [(float(a), float(b)) for a, b in zip(rng.uniform(10, ny - 10, 5), rng.uniform(100, nx - 100, 5))]
        pos = np.array(pos)
        n = len(pos)
        flux = rng.uniform(2000.0, 5000.0, n)
        origin = (np.rint(pos) - NS // 2).astype(np.int32)
        shift = pos - (origin + NS // 2)
        index = np.zeros(n, dtype=np.int32)
        psf = FR.model()[None]
        model, _, _ = Y.render(None, psf, index, origin, shift, flux, shape=LONG_FRAME)
        var = 4.0 + model / 2.0
        image = model + F.SKY + rng.normal(size=LONG_FRAME) * np.sqrt(var)
        nan = rng.uniform(size=LONG_FRAME) < 0.01
        for cy, cx in pos:
            y, x = int(np.rint(cy)), int(np.rint(cx))
            nan[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = False
        image[nan] = np.nan
        _LONG.update(image=image, var=var, psf=psf, index=index, origin=origin, shift=shift, flux=flux, pos=pos, n=n,
                     scale=rng.uniform(-1000.0, 1000.0, n))
    return _LONG


_REFS = {}


def fit_reference(name, s, radius):
    """solve_sparse of a scene dict with var and the background, once per name."""
    if name not in _REFS:
        _REFS[name] = F.solve_sparse(s['image'], s['var'], s['psf'], s['index'], s['origin'], s['shift'], radius, True)
    return _REFS[name]


def render_reference(name, s, subtract):
    """render_ref.render of a scene's 'scale' on its image, once per name and mode."""
    key = (name, 'render', subtract)
    if key not in _REFS:
        _REFS[key] = Y.render(s['image'], s['psf'], s['index'], s['origin'], s['shift'], s['scale'], subtract)
    return _REFS[key]


def find_reference(name, s, var=True, **kw):
    """find_ref.find of a scene dict (its psf's first model), once per name."""
    key = (name, 'find')
    if key not in _REFS:
        psf = s['psf'] if s['psf'].ndim == 2 else s['psf'][0]
        _REFS[key] = FR.find(s['image'], s['var'] if var else None, psf, **kw)
    return _REFS[key]


def footprints(shape, origin):
    """The boolean frame of the pixels inside any star's footprint."""
    inside = np.zeros(shape, dtype=bool)
    for o in origin:
        y0, y1, x0, x1 = Y.footprint(shape, o)
        if y0 < y1 and x0 < x1:
            inside[y0:y1, x0:x1] = True
    return inside


# ---- d. tile-count frames
TILE_FRAMES = {'1024x1024': (1024, 1024), '1312x800': (1312, 800)}
TILE_TARGETS = {'1024x1024': (0, 511, 512, 513, 1023), '1312x800': (0, 511, 512, 513, 1023, 1024)}
TILE_RADIUS = 8.0
_TILES = {}


def tiles_of(shape, origin):
    """The set of tile indices (ty ntx + tx, the renderer's order) a star's footprint meets."""
    ntx = -(-shape[1] // TILE)
    y0, y1, x0, x1 = Y.footprint(shape, origin)
    if y0 >= y1 or x0 >= x1:
        return set()
    return {ty * ntx + tx for ty in range(y0 // TILE, (y1 - 1) // TILE + 1) for tx in range(x0 // TILE, (x1 - 1) // TILE + 1)}


def tile_frame(name):
    """About 40 stars on a frame of TILE_FRAMES: one centred in every tile of TILE_TARGETS (tile 0, the last tile, and
    the tiles around the borders of the scan's shares), the rest at random; the models of render_ref by k % 4, fluxes
    300 .. 3000, sky 7, var = 4 + model / 2, Gaussian noise, 1 % NaN; 'scale' and 'noise' (an image_in) for the
    renderer; default_rng(41)."""
    if name not in _TILES:
        shape = TILE_FRAMES[name]
        ny, nx = shape
        ntx = -(-nx // TILE)
        rng = np.random.default_rng(41)
        pos = [((t // ntx) * TILE + 15.7, (t % ntx) * TILE + 16.2) for t in TILE_TARGETS[name]]
        m = 40 - len(pos)
        pos += [(float(a), float(b)) for a, b in zip(rng.uniform(5, ny - 5, m), rng.uniform(5, nx - 5, m))]
        pos = np.array(pos)
        n = len(pos)
        flux = rng.uniform(300.0, 3000.0, n)
        origin = (np.rint(pos) - NS // 2).astype(np.int32)
        shift = pos - (origin + NS // 2)
        index = (np.arange(n) % 4).astype(np.int32)
        psf = Y.models()
        model, _, _ = Y.render(None, psf, index, origin, shift, flux, shape=shape)
        var = 4.0 + model / 2.0
        image = model + F.SKY + rng.normal(size=shape) * np.sqrt(var)
        image[rng.uniform(size=shape) < 0.01] = np.nan
        _TILES[name] = dict(image=image, var=var, psf=psf, index=index, origin=origin, shift=shift, flux=flux, pos=pos, n=n,
                            scale=rng.uniform(-1000.0, 1000.0, n), render_shift=rng.uniform(-8.0, 8.0, (n, 2)))
    return _TILES[name]


def tile_render_scene(name):
    """The renderer's view of tile_frame(name): the same image (noise, stars, NaN) and origins, shifts in +-8."""
    s = tile_frame(name)
    return dict(s, shift=s['render_shift'])


# ---- e. finder frames
FINDER_FRAMES = {'256x128': (256, 128), '257x128': (257, 128)}
FINDER = dict(half=3, sep=3, threshold=6.0)
# peaks on the rows 254, 255 and (where it exists) 256: in the last segment of chunk 0 (row 255, columns 96 .. 127) and,
# of 257 rows, two in chunk 1 (row 256), the first of them in its first segment
PLANTED = {'256x128': ((254.2, 60.3), (255.9, 110.4), (255.7, 12.3)),
           '257x128': ((254.2, 60.3), (255.1, 110.4), (256.6, 12.3), (256.3, 80.2))}
NOISE_FRAME = (300, 300)
NOISE_FIND = dict(half=1, sep=1, threshold=-1e300)
_FINDER = {}


def nseg(shape):
    return shape[0] * -(-shape[1] // TILE)


def segment(shape, pixel):
    """The row segment (row-major over (frame row, tile column): pixel order) of a flat pixel index."""
    Yp, Xp = divmod(int(pixel), shape[1])
    return Yp * -(-shape[1] // TILE) + Xp // TILE


def finder_frame(name):
    """Background 10, a variance plane in 0.5 .. 1.5 with matching Gaussian noise, Moffat stars of find_ref's model and
    flux 300 .. 3000 on a 16-px grid jittered by +-2.5 px down to row 237, and the PLANTED stars of the frame;
    default_rng(51)."""
    if name not in _FINDER:
        shape = FINDER_FRAMES[name]
        rng = np.random.default_rng(51)
        pos = [(10 + 16 * i + rng.uniform(-2.5, 2.5), 10 + 16 * j + rng.uniform(-2.5, 2.5))
               for i in range(15) for j in range(8)]
        pos = np.array(pos + list(PLANTED[name]))
        flux = rng.uniform(300.0, 3000.0, 124)[:len(pos)]
        var = rng.uniform(0.5, 1.5, (257, 128))
        image = FR.BACK + rng.normal(size=(257, 128)) * np.sqrt(var)
        for (cy, cx), f in zip(pos, flux):
            image += f * FR.moffat(cy, cx, (257, 128)) / FR.moffat(NS // 2, NS // 2).sum()
        ny = shape[0]
        _FINDER[name] = dict(image=np.ascontiguousarray(image[:ny]), var=np.ascontiguousarray(var[:ny]), psf=FR.model(),
                             pos=pos, flux=flux)
    return _FINDER[name]


def narrow_core():
    """A Gaussian of sigma 0.6 px as a model stamp: a 3 x 3 core that hardly smooths, so that white noise keeps about one
    local maximum in nine pixels."""
    y, x = np.mgrid[:NS, :NS]
    return np.exp(-((y - 20.0) ** 2 + (x - 20.0) ** 2) / (2 * 0.6 ** 2))


def noise_frame():
    """300 x 300 of unit-variance Gaussian noise (default_rng(61)), var = 1, searched with narrow_core()."""
    if 'noise' not in _FINDER:
        image = np.random.default_rng(61).normal(size=NOISE_FRAME)
        _FINDER['noise'] = dict(image=image, var=np.ones(NOISE_FRAME), psf=narrow_core())
    return _FINDER['noise']


# ---- f. the deep cube
DEEP_NL = 1025
DEEP_FRAME = (12, 12)
DEEP_NAN_LAYER = 1024
DEEP_RADIUS = 4.0
_DEEP = {}


def deep_cube():
    """1025 layers of 12 x 12 with two stars: psf[i, l] = models[(i - l) % 4] as in cube_fit_cases.lattice, layer_shift
    (0.4 sin(0.1 l), 0.3 cos(0.07 l)) px, fluxes 500 .. 3000 per layer, sky 7, var = 4 + model / 2, Gaussian noise
    (default_rng(71)); layer 1024 all NaN."""
    if not _DEEP:
        rng = np.random.default_rng(71)
        nl = DEEP_NL
        pos = np.array([[3.8, 4.3], [7.6, 8.1]])
        origin = (np.rint(pos) - NS // 2).astype(np.int32)
        shift = pos - (origin + NS // 2)
        index = np.array([0, 1], dtype=np.int32)
        base = Y.models()
        psf = np.stack([np.roll(base, l, axis=0)[:2] for l in range(nl)], axis=1)
        l = np.arange(nl, dtype=np.float64)
        ls = np.stack([0.4 * np.sin(0.1 * l), 0.3 * np.cos(0.07 * l)], axis=1)
        data, var = np.empty((nl,) + DEEP_FRAME), np.empty((nl,) + DEEP_FRAME)
        flux = rng.uniform(500.0, 3000.0, (nl, 2))
        for i in range(nl):
            model, _, _ = Y.render(None, np.ascontiguousarray(psf[:, i]), index, origin, shift + ls[i], flux[i],
                                   shape=DEEP_FRAME)
            var[i] = 4.0 + model / 2.0
            data[i] = model + F.SKY + rng.normal(size=DEEP_FRAME) * np.sqrt(var[i])
        data[DEEP_NAN_LAYER] = np.nan
        _DEEP.update(cube=data, var=var, psf=psf, index=index, origin=origin, shift=shift, layer_shift=ls, flux=flux, n=2)
    return _DEEP


def deep_joint_reference():
    """The deep cube with the positions held as ONE least-squares problem, which is what fit_cube_psf_free's opening
    solve iterates on: the live layers' systems of frame_fit_ref.solve_sparse side by side (block diagonal; the
    unknowns of layer l are its two fluxes, then its constant).  Returns the dict frame_fit_ref.bounds reads -- of it
    only 'y', 'kappa' and 'terms' are meaningful, the per-star bounds assume one constant in the last place -- with
    'layers' (the per-layer results) and 'live'.  Its 'ref_err': every layer's own a-posteriori term holds for that
    layer's part of y, so the 2-norm over the layers holds for the whole."""
    if 'joint' not in _DEEP:
        import scipy.sparse as sp
        c = deep_cube()
        live = [l for l in range(DEEP_NL) if l != DEEP_NAN_LAYER]
        refs = [F.solve_sparse(c['cube'][l], c['var'][l], np.ascontiguousarray(c['psf'][:, l]), c['index'], c['origin'],
                               c['shift'] + c['layer_shift'][l], DEEP_RADIUS, True) for l in live]
        nu = sum(len(r['x']) for r in refs)
        N, Nabs = np.zeros((nu, nu)), np.zeros((nu, nu))
        o = 0
        for r in refs:
            m = len(r['x'])
            N[o:o + m, o:o + m], Nabs[o:o + m, o:o + m] = r['N'], r['Nabs']
            o += m
        cat = {k: np.concatenate([r[k] for r in refs]) for k in ('w', 'd', 'x', 'dg', 'res')}
        _DEEP['joint'] = dict(cat, A=sp.block_diag([r['A'] for r in refs], format='csr'), N=N, Nabs=Nabs, nacc=nu,
                              chi2=float(sum(r['chi2'] for r in refs)), background=True, sparse=True,
                              L=max(r['L'] for r in refs),
                              ref_err=float(np.sqrt(sum(r['ref_err'] ** 2 for r in refs))), layers=refs, live=live)
    return _DEEP['joint']
