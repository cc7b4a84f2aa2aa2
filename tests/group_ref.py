"""The contract of mpsfr_group_stars (include/mpsfr.h) restated in NumPy -- the yardstick of test_group_host.py and
test_gpu_group.py -- and the scenes they share.

Every output of the call is an integer or a single rounding, so the reference is exact: the tests compare with
assert_array_equal, there is no tolerance.  NumPy evaluates dy * dy, dx * dx and their sum as three rounded operations,
which is the link rule.  Candidate pairs come either from all pairs (small scenes) or from a 32-pixel grid (the large
field): a grid of its own, so that nothing of the library's binning is restated here.
"""
import functools

import numpy as np

NS = 40
MAX_GROUP = 4
NGROUP = 8
OVERSIZE, WIDE = 1, 2
MAX_SHIFT = 8.0
FILLER_ORIGIN = -(1 << 30)
_GRID = 32.0                     # > 16 + rounding: linked stars lie in the same or in adjacent cells of this grid


def star_kinds(pos, shape):
    """0 a star, -1 a filler (NaN in either coordinate), -2 out of range."""
    ny, nx = shape
    y, x = pos[:, 0], pos[:, 1]
    nan = np.isnan(y) | np.isnan(x)
    with np.errstate(invalid='ignore'):
        inside = (y >= -1.0) & (y <= ny) & (x >= -1.0) & (x <= nx)
    return np.where(nan, -1, np.where(inside, 0, -2))


def linked(pos, a, b, crit):
    """The link rule on the index arrays a, b."""
    dy = pos[a, 0] - pos[b, 0]
    dx = pos[a, 1] - pos[b, 1]
    d2 = dy * dy + dx * dx
    return d2 <= crit * crit


def _all_pairs(idx):
    a, b = np.triu_indices(idx.size, 1)
    return idx[a], idx[b]


def _grid_pairs(pos, idx):
    cy = np.floor(pos[idx, 0] / _GRID).astype(np.int64) + 2
    cx = np.floor(pos[idx, 1] / _GRID).astype(np.int64) + 2
    ncx = int(cx.max()) + 3
    key = cy * ncx + cx
    order = np.argsort(key, kind='stable')
    skey, sidx = key[order], idx[order]
    out_a, out_b = [], []
    for dy, dx in ((0, 0), (0, 1), (1, -1), (1, 0), (1, 1)):
        other = skey + dy * ncx + dx
        lo, hi = np.searchsorted(skey, other, 'left'), np.searchsorted(skey, other, 'right')
        cnt = hi - lo
        a = np.repeat(np.arange(skey.size), cnt)
        b = np.repeat(lo, cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        if (dy, dx) == (0, 0):
            keep = a < b
            a, b = a[keep], b[keep]
        out_a.append(sidx[a])
        out_b.append(sidx[b])
    return np.concatenate(out_a), np.concatenate(out_b)


def links(pos, crit, kind, pairs='auto'):
    """(a, b): every linked pair of stars, once."""
    idx = np.flatnonzero(kind == 0)
    if idx.size < 2:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if pairs == 'auto':
        pairs = 'all' if idx.size <= 3000 else 'grid'
    a, b = _all_pairs(idx) if pairs == 'all' else _grid_pairs(pos, idx)
    keep = linked(pos, a, b, crit)
    return a[keep], b[keep]


def components(n, a, b):
    """Union-find on the host: for each of n nodes the smallest index of its component."""
    parent = list(range(n))

    def find(i):
        root = i
        while parent[root] != root:
            root = parent[root]
        while parent[i] != root:
            parent[i], i = root, parent[i]
        return root
    for i, j in zip(a.tolist(), b.tolist()):
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


def group(pos, crit, shape, device=False, pairs='auto'):
    """The tables of the call for all groups (max_groups = their number): dict with label (nstar,), groups (G, 8),
    origin (G, 2), shift (G, 4, 2) one group per row, counts (6,).  On host pointers (device=False) a position out of
    range is a ValueError, as the call refuses it; with device=True it gets the label -2."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    crit = float(crit)
    kind = star_kinds(pos, shape)
    if not device and np.any(kind == -2):
        raise ValueError('a position outside the frame')
    n = pos.shape[0]
    a, b = links(pos, crit, kind, pairs)
    root = components(n, a, b)
    label = np.where(kind == 0, root, kind).astype(np.int32)
    stars = np.flatnonzero(kind == 0)
    order = stars[np.argsort(root[stars], kind='stable')]          # by label, ascending index inside a group
    labels, first, size = np.unique(root[order], return_index=True, return_counts=True)
    klass = np.minimum(size, MAX_GROUP + 1)
    rank = np.lexsort((labels, klass))
    G = labels.size
    groups = np.zeros((G, NGROUP), dtype=np.int32)
    groups[:, 4:] = -1
    origin = np.full((G, 2), FILLER_ORIGIN, dtype=np.int32)
    shift = np.zeros((G, MAX_GROUP, 2))
    for row, g in enumerate(rank):
        members = order[first[g]:first[g] + size[g]]
        assert members[0] == labels[g] and np.all(np.diff(members) > 0)
        nmem = int(size[g])
        groups[row, 0] = nmem
        groups[row, 2] = labels[g]
        groups[row, 4:4 + min(nmem, MAX_GROUP)] = members[:MAX_GROUP]
        if nmem > MAX_GROUP:
            groups[row, 1] = OVERSIZE
            continue
        p = pos[members, :2]
        c = 0.5 * (p.min(axis=0) + p.max(axis=0))
        o = np.floor(c + 0.5).astype(np.int64) - NS // 2
        origin[row] = o
        shift[row, :nmem] = p - (o + NS // 2).astype(np.float64)
        if np.any(np.abs(shift[row]) > MAX_SHIFT):
            groups[row, 1] |= WIDE
    counts = np.array([G] + [int(np.sum(klass == k)) for k in range(1, MAX_GROUP + 2)], dtype=np.int32)
    return dict(label=label, groups=groups, origin=origin, shift=shift, counts=counts)


def buffers(ref, max_groups):
    """What the call writes at `max_groups`: group_out (max_groups, 8), origin_out (max_groups, 2) and shift_out
    (max_groups * 8,) with the shifts of every class at the pitch of the class, filler rows behind the groups."""
    G = int(ref['counts'][0])
    n = min(G, max_groups)
    groups = np.zeros((max_groups, NGROUP), dtype=np.int32)
    groups[:, 4:] = -1
    origin = np.full((max_groups, 2), FILLER_ORIGIN, dtype=np.int32)
    groups[:n], origin[:n] = ref['groups'][:n], ref['origin'][:n]
    shift = np.zeros(max_groups * 2 * MAX_GROUP)
    off = np.concatenate([[0], np.cumsum(ref['counts'][1:])])
    for k in range(1, MAX_GROUP + 1):
        lo = int(min(off[k - 1], max_groups))
        m = int(min(off[k], max_groups)) - lo
        if m > 0:
            shift[8 * lo:8 * lo + 2 * k * m] = ref['shift'][lo:lo + m, :k].ravel()
    return groups, origin, shift


# ---- the shared scenes: name -> (pos, crit, shape) -------------------------------------------------------------------

FIELD_SEED = 3
FIELD = (200, 200)


def random_field(seed=FIELD_SEED, n=1500, shape=FIELD):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (n, 2)) * np.array(shape, dtype=float)


def check_field_classes(ref):
    """The conditions that make scene (a) a test of every class: asserted on the reference alone."""
    c = ref['counts']
    assert all(c[k] >= 20 for k in range(1, 5)) and c[5] >= 5, c


def chain(n, start, step):
    return np.asarray(start, dtype=float) + np.arange(n)[:, None] * np.asarray(step, dtype=float)


def chains_scene():
    """(c) three chains at 0.999 crit: 400 stars along a diagonal across many cells, 200 along row 16 and 200 along
    column 32, shuffled.  Each is one oversize group."""
    crit = 2.5
    s = 0.999 * crit
    pos = np.concatenate([chain(400, (5.0, 5.0), (s / np.sqrt(2.0), s / np.sqrt(2.0))),
                          chain(200, (16.0, 100.0), (0.0, s)),
                          chain(200, (100.0, 32.0), (s, 0.0))])
    rng = np.random.default_rng(11)
    return pos[rng.permutation(pos.shape[0])], crit, (720, 720)


BELOW16 = float(np.nextafter(16.0, 0.0))
BELOW17 = float(np.nextafter(17.0, 0.0))

# (d) pairs across the borders and corners of 16- and 17-pixel grids, 40 pixels apart from each other; crit = 2
BORDER_PAIRS = [((15.5, 50.0), (16.5, 50.0)),            # a row border of a 16-pixel grid
                ((BELOW16, 90.0), (16.0, 90.0)),         # 15.999... and 16.0
                ((60.0, 31.5), (60.0, 32.5)),            # a column border
                ((15.6, 127.6), (16.4, 128.4)),          # across the corner (16, 128)
                ((47.7, 47.7), (48.3, 48.3)),            # the corner (48, 48)
                ((48.4, 95.6), (47.6, 96.4)),            # the corner (48, 96), the other diagonal
                ((16.7, 170.0), (17.2, 170.0)),          # a row border of a 17-pixel grid
                ((100.0, BELOW17), (100.0, 17.0)),
                ((33.7, 33.7 + 170.0), (34.3, 34.3 + 170.0)),   # the corner (34, 204) of a 17-pixel grid
                ((101.9, 67.9), (102.1, 68.1)),          # the corner (102, 68) of a 17-pixel grid
                ((140.0, 140.0), (140.0, 142.5))]        # not linked: 2.5 > crit


def borders_scene():
    pos = np.array([p for pair in BORDER_PAIRS for p in pair])
    return pos, 2.0, (160, 240)


def far_scene():
    """crit = 16: the rounded difference of 32 and the double below 16 is 16.0 -- linked across a whole 16-pixel cell;
    33 minus the double below 17 is the double above 16 -- not linked."""
    pos = np.array([(BELOW16, 200.0), (32.0, 200.0), (BELOW17, 300.0), (33.0, 300.0)])
    return pos, 16.0, (64, 400)


def exact_scene(crit):
    """(b) a 3-4-5 pair and two stars at one position."""
    pos = np.array([(10.0, 10.0), (13.0, 14.0), (40.0, 40.0), (40.0, 40.0)])
    return pos, crit, (64, 64)


def wide_scene():
    """(e) a chain of four at crit = 6 whose ends are 17.7 pixels apart."""
    pos = np.array([(50.0, 50.0), (50.0, 55.9), (50.0, 61.8), (50.0, 67.7)])
    return pos, 6.0, (100, 120)


def edges_scene():
    """(f) stars at -1 and at (ny, nx), with neighbours."""
    ny, nx = 70, 90
    pos = np.array([(-1.0, -1.0), (0.5, 0.0), (float(ny), float(nx)), (ny - 1.5, nx - 1.0), (-1.0, float(nx)),
                    (float(ny), -1.0), (float(ny), 1.0), (35.0, 45.0)])
    return pos, 2.5, (ny, nx)


BLEND_FRAME = (160, 160)
BLEND_CRIT = 5.0
BLEND_FIND = dict(half=2, sep=2, threshold=5.0)      # a 5 x 5 core resolves stars 4 pixels apart at FWHM 3.5


def blend_field():
    """40 stars on 160 x 160: 10 isolated, 9 pairs 4 pixels apart, 4 triples (an L with 4-pixel arms), one to a cell of
    a 30-pixel grid.  Returns (positions (40, 2), fluxes (40,), the size of every star's blend (40,))."""
    rng = np.random.default_rng(7)
    cells = [(20 + 30 * i, 20 + 30 * j) for i in range(5) for j in range(5)]
    pos, size = [], []
    for n, count in ((1, 10), (2, 9), (3, 4)):
        for _ in range(count):
            c = np.array(cells[len(size)], dtype=float) + rng.uniform(-2, 2, 2)
            if n == 1:
                pts = [c]
            elif n == 2:
                pts = [c + (0, -2), c + (rng.uniform(-.4, .4), 2)]
            else:
                pts = [c + (-2, -2), c + (-2 + rng.uniform(-.3, .3), 2), c + (2, -2 + rng.uniform(-.3, .3))]
            pos += pts
            size.append(n)
    blend = np.repeat(size, size)
    return np.array(pos), rng.uniform(1500, 3000, len(pos)), blend


def blend_background():
    """Background 5 with unit-variance noise: the frame the stars of blend_field are rendered into."""
    return 5.0 + np.random.default_rng(1).normal(size=BLEND_FRAME)


def scenes():
    return {'field': (random_field(), 2.5, FIELD),
            'exact5': exact_scene(5.0),
            'exact5-': exact_scene(float(np.nextafter(5.0, 0.0))),
            'chains': chains_scene(),
            'borders': borders_scene(),
            'far': far_scene(),
            'wide': wide_scene(),
            'edges': edges_scene()}


@functools.lru_cache(maxsize=None)
def scene_reference(name):
    """(pos, crit, shape, ref) of a scene; computed once, to be left unchanged."""
    pos, crit, shape = scenes()[name]
    ref = group(pos, crit, shape)
    if name == 'field':
        check_field_classes(ref)
    return pos, crit, shape, ref


@functools.lru_cache(maxsize=None)
def large_field():
    """65 536 uniform stars on 2048 x 2048 at crit = 3, grouped through the grid."""
    rng = np.random.default_rng(5)
    pos = rng.uniform(0.0, 2048.0, (65536, 2))
    return pos, 3.0, (2048, 2048), group(pos, 3.0, (2048, 2048), pairs='grid')
