"""Seeded cases of the PSF energy metrics on hard inputs, shared by tests/test_metrics_cases_host.py (CPU: the cases hit
what they claim, the NumPy model of the kernel passes them, its edited forms fail) and tests/test_gpu_metrics_edges.py
(the kernel against the mpmath yardstick tests/metrics_mp_ref.py).

A case is a dict: name, cls (the class 'a' .. 'g'), stamps (n, 40, 40), centers ((n, 2), or None for the centroid),
radii, boxes, fracs (lists, pixels / pixels / fractions) -- one call of mpsfr_stamp_metrics.
"""
import numpy as np

import moffat_ell_ref as M

NS = 40
SQH = float(np.sqrt(0.5))                    # (its square rounds up, to 0.5000000000000001: the unit pixel is whole)
FRACS_HARD = [1e-6, 0.1, 0.5, 0.95, 1.0 - 1e-6]
CENTER_MAX = 100.0                           # kCenterMax of metrics.hip (and the check of _lib.metric_centers)
ROOT_PROMISE = 1e-12                         # include/mpsfr.h: |EE(R_k) - f_k| <= 1e-12 with status 0
TOL = 1e-10                                  # the project's tolerance on energies and centroid (test_gpu_metrics.py)

# Worst |kernel - yardstick| per class measured on an MI355X (both precision contexts give the same figures: the
# arithmetic is fp64 in both), in units of sum|I| / |flux| of the stamp: flux (relative), centroid (px), EE and SQE.
# A zero is a quantity the class determines exactly: the echo of a given centre, the flux of one pixel, no boxes.
# These figures govern the bounds.  They are the full-precision figures of the run, which profiles/metrics_margins.json
# records beside the bounds, rounded up to two digits.
MEASURED = {
    'a': dict(flux=8.1e-17, centroid=0.0, ee=1.7e-15, sqe=0.0),
    'b': dict(flux=0.0, centroid=0.0, ee=5.7e-14, sqe=0.0),
    'c': dict(flux=1.9e-16, centroid=4.4e-15, ee=4.4e-16, sqe=2.4e-16),
    'd': dict(flux=1.9e-16, centroid=5.7e-15, ee=5.4e-19, sqe=0.0),
    'f': dict(flux=5.6e-17, centroid=4.7e-15, ee=2.6e-12, sqe=3.2e-12),
    'g': dict(flux=7.7e-17, centroid=0.0, ee=8.8e-17, sqe=1.1e-17),
}


def bound(measured):
    """The smaller of TOL and four times the measured value, rounded up to one digit."""
    x = 4.0 * measured
    if x <= 0.0:
        return 0.0
    e = int(np.floor(np.log10(x)))
    return min(TOL, float('%de%d' % (int(np.ceil(x / 10.0 ** e - 1e-9)), e)))


BOUNDS = {cls: {k: bound(v) for k, v in m.items()} for cls, m in MEASURED.items()}

def case(name, cls, stamps, centers, radii=(), boxes=(), fracs=()):
    st = np.ascontiguousarray(np.asarray(stamps, dtype=float).reshape(-1, NS, NS))
    ce = None if centers is None else np.broadcast_to(np.asarray(centers, dtype=float), (st.shape[0], 2)).copy()
    return dict(name=name, cls=cls, stamps=st, centers=ce, radii=[float(r) for r in radii],
                boxes=[float(b) for b in boxes], fracs=[float(f) for f in fracs])


# ---- (a) cut counts: the queue pass at 64, 128 and beyond 128 entries
CUT_COUNTS = [((19.3, 20.1), 8.0, 64), ((19.3, 20.1), 16.0, 128), ((19.5, 19.5), 16.0, 124), ((19.5, 19.5), 16.3, 132),
              ((19.5, 19.5), 19.0, 148), ((19.5, 19.5), 19.9, 156), ((19.5, 19.5), 20.4, 124),
              ((19.6027, 19.3256), 19.3314, 156)]


def cut_mask(cp, cq, r):
    """The pixels the kernel's two compares queue, evaluated in fp64 as the kernel evaluates them."""
    p, q = np.mgrid[0:NS, 0:NS].astype(float)
    ay, ax = np.abs(p - cp), np.abs(q - cq)
    fx, fy = ax + 0.5, ay + 0.5
    nx, ny = np.maximum(ax - 0.5, 0.0), np.maximum(ay - 0.5, 0.0)
    r2 = r * r
    return ~(fx * fx + fy * fy <= r2) & (nx * nx + ny * ny < r2)


def stamps_a():
    rng = np.random.default_rng(1601)
    p, q = np.mgrid[0:NS, 0:NS]
    moffat = M.stamp(1.3, 19.4, 20.2, 9.0, 0.8, 30.0, 2.0)              # wide: light on every circle of the class
    noise = rng.standard_normal((NS, NS))
    assert noise.sum() > 0.0
    checker = np.where((p + q) % 2 == 0, 1.0, -1.0) + 2.0
    ring = cut_mask(19.5, 19.5, 19.9).astype(float)
    return np.array([moffat, noise, checker, ring])


def cases_a():
    st = stamps_a()
    out = []
    for k, c in enumerate(sorted({c for c, _, _ in CUT_COUNTS})):
        out.append(case('a%d' % k, 'a', st, c, radii=[r for cc, r, _ in CUT_COUNTS if cc == c]))
    return out


# ---- (b) impulses
def impulse_positions():
    rng = np.random.default_rng(1602)
    edge = [0, 7, 8, 39]
    pos = {(i, j) for i in edge for j in range(NS)} | {(i, j) for i in range(NS) for j in edge}
    pos = sorted(pos)
    extra = [(int(i), int(j)) for i, j in rng.integers(0, NS, (100, 2))]
    return pos + extra


B_NEAR_OFFSET = (0.3, -0.2)
B_NEAR_RADII = [0.15, 0.4, 0.75, 1.1]             # (none tangent to a grid line from the offset centre)
B_MID_RADII = [0.5, 1.0, 2.0, 4.0, 7.3, 10.0, 13.0, 16.0, 19.0, 20.4, 22.0, 25.0, 27.5, 28.3]
B_OWN_RADII = [0.25, 0.5, SQH, 1.0, 80.0]
B_OWN_BOXES = [0.25, 0.5, 1.0, 80.0]
B_OWN_FRACS = [0.1, 0.5]


def cases_b():
    pos = impulse_positions()
    st = np.zeros((len(pos), NS, NS))
    for k, (i, j) in enumerate(pos):
        st[k, i, j] = 1.0
    near = np.array(pos, dtype=float) + np.array(B_NEAR_OFFSET)
    return [case('b_near', 'b', st, near, radii=B_NEAR_RADII),
            case('b_mid', 'b', st, (19.5, 19.5), radii=B_MID_RADII),
            case('b_own', 'b', st, None, radii=B_OWN_RADII, boxes=B_OWN_BOXES, fracs=B_OWN_FRACS)]


# ---- (c) exact geometry
C_CENTERS = [(19.5, 19.5), (19.5, 20.0), (20.0, 20.0)]              # a pixel corner, an edge, a pixel
C_RADII_1 = [0.3, 0.5, SQH, 1.0, 5.0, 13.0, 2.0, 3.0, 4.0, 6.0]
C_RADII_2 = [7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 14.0, 15.0, 16.0, 17.0, 18.0, 19.0, 20.0]
C_BOXES = [1.0, 2.0, 3.0, 4.0, 7.0, 8.0, 39.0, 40.0]                # edges on pixel edges and on pixel centres


def stamps_c():
    rng = np.random.default_rng(1603)
    return np.array([np.full((NS, NS), 0.37), rng.standard_normal((NS, NS)) + 0.25])


def cases_c():
    st = stamps_c()
    stamps = np.array([s for _ in C_CENTERS for s in st])
    centers = np.array([c for c in C_CENTERS for _ in st])
    return [case('c1', 'c', stamps, centers, radii=C_RADII_1, boxes=C_BOXES),
            case('c2', 'c', stamps, centers, radii=C_RADII_2)]


def case_full():
    """16 + 16 + 16 parameters at once (class c: near centres, a non-negative stamp and a pedestal of noise)."""
    rng = np.random.default_rng(1604)
    st = np.array([M.stamp(0.9, 20.3, 18.8, 6.0, 0.7, 50.0, 2.5), np.abs(rng.standard_normal((NS, NS))) + 0.1])
    radii = [0.3, 0.8, 1.5, 2.5, 4.0, 5.5, 7.3, 9.0, 11.0, 13.0, 16.0, 19.0, 22.0, 31.0, 45.0, 80.0]
    boxes = [0.3, 1.0, 2.0, 3.7, 5.0, 8.0, 11.0, 13.5, 17.0, 21.0, 26.0, 33.0, 40.0, 55.0, 70.0, 80.0]
    fracs = [0.01, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.85, 0.9, 0.95, 0.98, 0.99, 0.999]
    return case('c_full', 'c', st, None, radii=radii, boxes=boxes, fracs=fracs)


# ---- (d) peak ties
D_TIES = [((3, 5), (11, 5)),        # one lane, two slots
          ((0, 39), (1, 0)),
          ((7, 8), (8, 0)),         # the row-major first is in the higher lane
          ((0, 8), (1, 0))]         # the row-major first is in the later slot of its lane


def cases_d():
    """Returns (case, expected) -- expected[k] = (peak, peak_p, peak_q, status)."""
    rng = np.random.default_rng(1605)
    st, want = [], []
    for a, b in D_TIES:
        s = 0.5 * rng.random((NS, NS)) + 0.1
        s[a] = s[b] = 3.0
        st.append(s)
        want.append((3.0, a[0], a[1], 0))
    st.append(np.full((NS, NS), 0.37))
    want.append((0.37, 0, 0, 0))
    neg = -(rng.random((NS, NS)) + 1.0)
    neg[17, 23] = neg[30, 2] = -0.5
    st.append(neg)
    want.append((-0.5, 17, 23, 2))
    inf = 0.5 * rng.random((NS, NS)) + 0.1
    inf[9, 9] = 7.0
    inf[12, 33] = inf[33, 12] = np.inf
    st.append(inf)
    want.append((np.inf, 12, 33, 2))
    return case('d', 'd', np.array(st), None, radii=[1.0]), want


# ---- (e) amplitudes
E_POWERS = [30, -30, 200, -200, 600, -600]
E_RADII = [8.0, 16.3, 19.9]
E_BOXES = [3.7, 17.0]
E_FRACS = [0.1, 0.5, 0.95]


def cases_e():
    """[(k, case)] with k = 0 first: the stamps of (a) times 2^k, at the centroid and at a given centre."""
    st = stamps_a()
    out = []
    for k in [0] + E_POWERS:
        s = st * 2.0 ** k
        assert np.all(np.isfinite(s)) and np.all((s == 0.0) | (np.abs(s) > 1e-290))
        out.append((k, case('e_centroid_%d' % k, 'e', s, None, radii=E_RADII, boxes=E_BOXES, fracs=E_FRACS)))
        out.append((k, case('e_given_%d' % k, 'e', s, (19.3, 20.1), radii=E_RADII, boxes=E_BOXES, fracs=E_FRACS)))
    return out


# ---- (f) mixed signs
LADDER = [1.0, 1e2, 1e4, 1e6, 1e8]


def ladder_stamps(rungs=LADDER):
    """One Moffat plus a noise pattern without flux or first moments, scaled so that sum|I| / flux is the rung."""
    rng = np.random.default_rng(1606)
    base = M.stamp(1.0, 19.7, 19.2, 6.0, 0.85, 20.0, 2.5)
    p, q = np.mgrid[0:NS, 0:NS].astype(float)
    z = rng.standard_normal((NS, NS))
    A = np.stack([np.ones(NS * NS), p.ravel(), q.ravel()], axis=1)
    z = z - (A @ np.linalg.lstsq(A, z.ravel(), rcond=None)[0]).reshape(NS, NS)
    out = []
    for g in rungs:
        t = 0.0 if g <= 1.0 else g * base.sum() / np.abs(z).sum()
        out.append(base + t * z)
    return np.array(out)


def cases_f():
    rng = np.random.default_rng(1607)
    ring = M.stamp(1.0, 19.8, 19.4, 3.0, 1.0, 0.0, 2.5) - 0.04 * M.stamp(1.0, 19.8, 19.4, 12.0, 1.0, 0.0, 4.0)
    noise = rng.standard_normal((NS, NS)) + 0.3
    two = np.zeros((NS, NS))
    two[15, 12] = two[15, 22] = 1.0
    assert ring.sum() > 0.0 and ring.min() < 0.0 and noise.sum() > 0.0
    return [case('f_signs', 'f', np.array([ring, noise]), None, radii=[2.0, 7.3, 19.9], boxes=[3.7, 17.0],
                 fracs=FRACS_HARD),
            case('f_two', 'f', two, (15.0, 12.0), radii=[SQH, 5.0, 9.0, 11.0], fracs=FRACS_HARD),
            case('f_ladder', 'f', ladder_stamps(), None, radii=[2.0, 7.3, 19.9], boxes=[3.7, 17.0], fracs=FRACS_HARD)]


# ---- (g) far centres
G_DIST = [0.0, 30.0, 100.0, 300.0, 1e3, 3e3, 1e4]


def far_centers():
    """[(distance, kind, (cp, cq))]: the ladder of distances along a row (to the left of the stamp) and along the
    diagonal, and centres beyond the limit that an earlier limit of 1e4 px let through ('other': off the axes, where an
    unflagged radius was off by 2e-12 to 4e-12 in the model of the kernel).  With CENTER_MAX = 100 the rung 100 of the
    row is the limit itself; the rungs from 300 on and every 'other' are refused."""
    out = []
    for d in G_DIST:
        out.append((d, 'row', (19.5, -d if d > 0.0 else -0.5)))
        s = float(np.round(d / np.sqrt(2.0)))
        out.append((d, 'diag', (-0.5 - s, -0.5 - s) if d < 1e4 else (-7000.0, -7000.0)))
    out += [(424.0, 'other', (300.0, 300.0)), (1414.0, 'other', (1000.0, 1000.0)), (2882.0, 'other', (-2202.0, -1859.0)),
            (5162.0, 'other', (-4209.0, -2988.0)), (2155.0, 'other', (-1551.0, -1497.0)),
            (1654.0, 'other', (-1124.0, -1214.0)), (100.0, 'other', (19.5, np.nextafter(-100.0, -np.inf)))]
    return out


def in_range(centers):
    """Mask of the centres mpsfr_stamp_metrics accepts."""
    return np.max(np.abs(np.asarray(centers, dtype=float)), axis=-1) <= CENTER_MAX


def g_stamp():
    st = M.stamp(1.0, 19.6, 20.3, 7.0, 0.9, 10.0, 2.2)
    assert st.min() >= 0.0
    return st


def cases_g():
    """The ladder, every fraction in one call: (accepted centres, refused centres) -- the second has no yardstick, the
    call refuses it (ValueError in the Python layer, status 2 from the kernel)."""
    st, fc = g_stamp(), far_centers()
    ce = np.array([c for _, _, c in fc])
    ok = in_range(ce)
    kw = dict(radii=[80.0], boxes=[80.0], fracs=FRACS_HARD)
    return (case('g', 'g', np.array([st] * int(ok.sum())), ce[ok], **kw),
            case('g_refused', 'g', np.array([st] * int((~ok).sum())), ce[~ok], **kw))


G_SINGLE_FRACS = FRACS_HARD + [0.332, 0.56, 0.812]


def limit_centers():
    """The four corners of the accepted range, the two limits on a row and a column of the stamp, and 18 seeded centres
    off the axes with |cp|, |cq| between 30 and CENTER_MAX."""
    rng = np.random.default_rng(1608)
    L = CENTER_MAX
    out = [(sa * L, sb * L) for sa in (1, -1) for sb in (1, -1)] + [(L, 7.25), (12.0, -L)]
    out += [tuple(rng.choice([-1.0, 1.0], 2) * rng.uniform(30.0, L, 2)) for _ in range(18)]
    return np.array(out)


def cases_g_single():
    """One fraction per call, so that a row's status is the status of that one radius: a row of several fractions is
    flagged as soon as any of them is, which would hide an unflagged radius that misses the promise."""
    ce = limit_centers()
    st = np.array([g_stamp()] * len(ce))
    return [case('g_single_%d' % k, 'g', st, ce, fracs=[f]) for k, f in enumerate(G_SINGLE_FRACS)]


def all_cases():
    return (cases_a() + cases_b() + cases_c() + [case_full(), cases_d()[0]] + [c for _, c in cases_e()] + cases_f()
            + [cases_g()[0]] + cases_g_single())


# ---- the comparison with the yardstick
HEAD = 8


def split(c, row):
    """(ee, sqe, r_ee) of an output row of case c."""
    nr, nb = len(c['radii']), len(c['boxes'])
    return row[HEAD:HEAD + nr], row[HEAD + nr:HEAD + nr + nb], row[HEAD + nr + nb:]


def measure(c, rows, stamps=None):
    """Errors of the rows of one call against tests/metrics_mp_ref.py, per stamp: dict of arrays
    flux (relative), centroid (px), ee (n, nrad), sqe (n, nbox) -- each divided by sum|I| / |flux| of the stamp, the
    factor by which a stamp of mixed signs magnifies a rounding error of the sums -- root (n, nfrac): the yardstick's
    |EE(R_k) - f_k|, not divided; rmax (n,) and ratio (n,).  Rows with status 2 give NaN.  The yardstick takes the
    centre the row reports: the centroid has its own column."""
    import metrics_mp_ref as Y
    st = c['stamps'] if stamps is None else stamps
    n, nr, nb, nf = len(st), len(c['radii']), len(c['boxes']), len(c['fracs'])
    out = dict(flux=np.full(n, np.nan), centroid=np.full(n, np.nan), ee=np.full((n, nr), np.nan),
               sqe=np.full((n, nb), np.nan), root=np.full((n, nf), np.nan), rmax=np.full(n, np.nan),
               ratio=np.full(n, np.nan))
    for k, (s, row) in enumerate(zip(st, rows)):
        if row[6] == 2.0:
            continue
        ratio = Y.abs_ratio(s)
        flux = Y.flux(s)
        ce = (float(row[4]), float(row[5]))
        ee, sqe, ree = split(c, row)
        out['ratio'][k] = ratio
        out['rmax'][k] = float(Y.r_max(ce))
        out['flux'][k] = float(abs(Y.mp.mpf(float(row[0])) - flux) / abs(flux)) / ratio
        if c['centers'] is None:
            cy = Y.centroid(s)
            out['centroid'][k] = float(max(abs(Y.mp.mpf(ce[0]) - cy[0]), abs(Y.mp.mpf(ce[1]) - cy[1]))) / ratio
        else:
            out['centroid'][k] = 0.0 if (ce[0] == c['centers'][k][0] and ce[1] == c['centers'][k][1]) else np.inf
        for j, r in enumerate(c['radii']):
            out['ee'][k, j] = float(abs(Y.EE(s, ce, r) - Y.mp.mpf(float(ee[j])))) / ratio
        for j, b in enumerate(c['boxes']):
            out['sqe'][k, j] = float(abs(Y.SQE(s, ce, b) - Y.mp.mpf(float(sqe[j])))) / ratio
        for j, f in enumerate(c['fracs']):
            if np.isfinite(ree[j]) and ree[j] > 0.0:
                out['root'][k, j] = float(abs(Y.EE(s, ce, ree[j]) - Y.mp.mpf(f)))
            else:
                out['root'][k, j] = np.inf if not np.isfinite(ree[j]) or ree[j] < 0.0 else f
    return out


def expected_peak(stamp):
    """(peak, peak_p, peak_q): the brightest pixel, the first in row-major order (np.argmax's rule)."""
    k = int(np.argmax(stamp))
    return float(stamp.flat[k]), k // NS, k % NS


def check_own_impulses(c, rows):
    """Case b_own (one pixel of value 1, centroid): known values, from no yardstick.  The centre is the pixel; EE(r) =
    pi r^2 for r <= 1/2 and 1 from sqrt(1/2) on; SQE(s) = s^2 for s <= 1; the radius of a fraction f <= pi / 4 is
    sqrt(f / pi)."""
    pos = impulse_positions()
    assert len(rows) == len(pos)
    for (i, j), row in zip(pos, rows):
        assert tuple(row[:8]) == (1.0, 1.0, i, j, i, j, 0.0, 0.0), (i, j, row[:8])
        ee, sqe, ree = split(c, row)
        assert abs(ee[0] - np.pi / 16) <= 1e-15 and abs(ee[1] - np.pi / 4) <= 1e-15, (i, j, ee)
        assert ee[2] == 1.0 and ee[3] == 1.0 and ee[4] == 1.0, (i, j, ee)
        assert np.array_equal(sqe, [0.0625, 0.25, 1.0, 1.0]), (i, j, sqe)
        for f, r in zip(c['fracs'], ree):
            assert abs(np.pi * r * r - f) <= ROOT_PROMISE, (i, j, f, r)


def check_peaks(rows, want):
    """Case d: peak, its position and the status exactly; with status 2 every energy is NaN."""
    for k, (row, (pk, pp, pq, status)) in enumerate(zip(rows, want)):
        assert (row[1], row[2], row[3], row[6], row[7]) == (pk, pp, pq, status, 0.0), (k, row[:8])
        assert np.all(np.isnan(row[HEAD:])) if status == 2 else np.all(np.isfinite(row)), (k, row)
