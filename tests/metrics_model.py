"""fp64 NumPy model of k_stamp_metrics (muse_psfr_amd/csrc/metrics.hip): the arithmetic of the kernel in the kernel's
own structure -- the 8 x 8 lane map with 25 slots per lane, the sweep with its two compares, the queue of cut pixels
written at ballot-prefix positions and taken 64 entries at a time, the corner sum of the overlap, the first-maximum
ladder, the bracketed Newton iteration.  It has no fused multiply-adds and sums the wave with np.sum, so it agrees with
the kernel to rounding, not bit for bit.

`edits` names deliberate mistakes (tests/test_metrics_cases_host.py shows that the cases of tests/metrics_cases.py
catch each of them):
  'queue128'   the queue pass stops after 128 entries
  'pos64'      an entry whose queue position is a positive multiple of 64 is written one slot early
  'sx0'        sx / sy taken as -1 (instead of +1) where x0 / y0 < 0: the sign of the near-corner terms of a pixel that
               holds the centre's row or column
  'sx_at_zero' sx / sy taken as +1 (instead of -1) where x0 / y0 == 0: no mistake at all, that term is zero
  'in_lt'      the whole-pixel compare with < instead of <=
  'tie_lane'   the maximum ladder prefers the lower lane on a tie, not the lower pixel offset
  'slot_swap'  slot m of a lane taken as pixel (8 mi + lr, 8 mo + lc)
"""
import numpy as np

NS, NPXL, MQ = 40, 25, 256
K_ROOT_GOAL, K_ROOT_TOL, K_ROOT_MAXIT = 2.0e-14, 5.0e-13, 100
K_CENTER_MAX = 100.0
LANE = np.arange(64)
LR, LC = LANE >> 3, LANE & 7


def to_lds(stamp, edits=()):
    """[25][64]: slot m of lane (lr, lc) is pixel (8 mo + lr, 8 mi + lc), m = 5 mo + mi."""
    st = np.asarray(stamp, dtype=float)
    sp = np.empty((NPXL, 64))
    for m in range(NPXL):
        mo, mi = divmod(m, 5)
        if 'slot_swap' in edits:
            mo, mi = mi, mo
        sp[m] = st[8 * mo + LR, 8 * mi + LC]
    return sp


def _quadrant_area(x, y, xa, yb, r2):
    inside = x * x + y * y <= r2
    ang = np.where(inside, 0.0, np.arctan2(x * y - yb * xa, x * xa + yb * y))
    area = np.where(inside, x * y, 0.5 * (xa * y + x * yb) + 0.5 * r2 * ang)
    return area, ang


def pixel_overlap(ax, ay, r, edits=()):
    """(area, arc) of the unit pixels centred (ax, ay) >= 0 away from the centre of the circle (arrays)."""
    r2 = r * r
    x0, y0 = ax - 0.5, ay - 0.5
    X0, X1 = np.minimum(np.abs(x0), r), np.minimum(ax + 0.5, r)
    Y0, Y1 = np.minimum(np.abs(y0), r), np.minimum(ay + 0.5, r)
    yb0, yb1 = np.sqrt(np.maximum(r2 - X0 * X0, 0.0)), np.sqrt(np.maximum(r2 - X1 * X1, 0.0))
    xa0, xa1 = np.sqrt(np.maximum(r2 - Y0 * Y0, 0.0)), np.sqrt(np.maximum(r2 - Y1 * Y1, 0.0))
    pos = -1.0 if 'sx0' in edits else 1.0
    if 'sx_at_zero' in edits:
        sx, sy = np.where(x0 <= 0.0, pos, -1.0), np.where(y0 <= 0.0, pos, -1.0)
    else:
        sx, sy = np.where(x0 < 0.0, pos, -1.0), np.where(y0 < 0.0, pos, -1.0)
    area, arc = np.zeros_like(ax), np.zeros_like(ax)
    for c in range(4):
        hx, hy = bool(c & 1), bool(c & 2)
        sg = (1.0 if hx else sx) * (1.0 if hy else sy)
        s, ang = _quadrant_area(X1 if hx else X0, Y1 if hy else Y0, xa1 if hy else xa0, yb1 if hx else yb0, r2)
        area = area + sg * s
        arc = arc + sg * ang
    return area, arc


def circle_sum(sp, cp, cq, r, edits=(), qo=None):
    """(sum_pq A I, d/dr of it, number of queued pixels) as the kernel's circle_sum.  `qo`: the queue in LDS (int[MQ]);
    what an earlier call left in it stays unless this call overwrites it, as on the device."""
    if qo is None:
        qo = np.zeros(MQ, dtype=int)
    r2 = r * r
    m = np.arange(NPXL)[:, None]
    mo, mi = m // 5, m % 5
    # the sweep, all 25 slots at once: [slot][lane]
    ay, ax = np.abs(8.0 * mo + (LR - cp)[None, :]), np.abs(8.0 * mi + (LC - cq)[None, :])
    fx, fy = ax + 0.5, ay + 0.5
    nx, ny = np.maximum(ax - 0.5, 0.0), np.maximum(ay - 0.5, 0.0)
    far2 = fx * fx + fy * fy
    inn = far2 < r2 if 'in_lt' in edits else far2 <= r2
    cut = ~inn & (nx * nx + ny * ny < r2)
    acc = np.where(inn, sp, 0.0).sum(axis=0)
    dacc = np.zeros(64)
    # the queue: entries in the order (slot, lane), the position of an entry is the ballot prefix (count of the
    # slots before + mbcnt of the lanes below)
    entries = np.nonzero(cut.ravel())[0]
    count = entries.size
    pos = np.arange(count)
    if 'pos64' in edits:
        pos = pos - ((pos > 0) & (pos % 64 == 0))
    w = pos < MQ
    qo[pos[w]] = entries[w]
    assert count <= MQ                                              # (the fallback is not modelled: unreachable)
    top = min(count, 128) if 'queue128' in edits else count
    for k0 in range(0, top, 64):
        k = k0 + LANE
        live = k < top
        o = qo[np.where(live, k, 0)]
        m, ln = o >> 6, o & 63
        mo, mi = m // 5, m - 5 * (m // 5)
        ay, ax = np.abs((8 * mo + (ln >> 3)) - cp), np.abs((8 * mi + (ln & 7)) - cq)
        a, arc = pixel_overlap(ax, ay, r, edits)
        v = sp.ravel()[o]
        acc = acc + np.where(live, a * v, 0.0)
        dacc = dacc + np.where(live, arc * v, 0.0)
    return float(acc.sum()), float(r * dacc.sum()), count


def peak(stamp, edits=()):
    """(best, offset) as the lane scan and the xor ladder of wave_first_max give them."""
    sp = to_lds(stamp, edits)
    best, besto = np.full(64, -np.inf), np.full(64, NS * NS)
    for m in range(NPXL):
        mo, mi = divmod(m, 5)
        off = (8 * mo + LR) * NS + 8 * mi + LC
        up = sp[m] > best
        best, besto = np.where(up, sp[m], best), np.where(up, off, besto)
    key = LANE if 'tie_lane' in edits else besto
    o = 32
    while o:
        ob, oo, ok = best[LANE ^ o], besto[LANE ^ o], key[LANE ^ o]
        up = (ob > best) | ((ob == best) & (ok < key))
        best, besto, key = np.where(up, ob, best), np.where(up, oo, besto), np.where(up, ok, key)
        o >>= 1
    bo = int(besto[0])
    return float(best[0]), (0 if bo >= NS * NS else bo)


def metrics(stamp, center, radii, boxes, fracs, edits=(), center_max=K_CENTER_MAX):
    """The kernel's output row of one stamp (center: (cp, cq) or None) and the queue counts of its EE sweeps."""
    st = np.asarray(stamp, dtype=float)
    sp = to_lds(st, edits)
    nout = 8 + len(radii) + len(boxes) + len(fracs)
    row = np.full(nout, np.nan)
    best, besto = peak(st, edits)
    with np.errstate(all='ignore'):
        flux = float(sp.sum())
        finite = bool(np.all(np.abs(sp) < np.inf))
        ok = finite and flux > 0.0 and flux < np.inf
        if center is not None:
            cp, cq = float(center[0]), float(center[1])
        else:
            pp = np.array([[8 * (m // 5) + lr for lr in LR] for m in range(NPXL)], dtype=float)
            qq = np.array([[8 * (m % 5) + lc for lc in LC] for m in range(NPXL)], dtype=float)
            cp, cq = ((pp * sp).sum() / flux, (qq * sp).sum() / flux) if ok else (np.nan, np.nan)
    ok = ok and abs(cp) <= center_max and abs(cq) <= center_max
    row[:8] = [flux, best, besto // NS, besto % NS, cp, cq, 0.0, 0.0]
    counts = []
    if not ok:
        row[6] = 2.0
        return row, counts
    iflux = 1.0 / flux
    qo = np.zeros(MQ, dtype=int)
    for k, r in enumerate(radii):
        s, _, n = circle_sum(sp, cp, cq, float(r), edits, qo)
        counts.append(n)
        row[8 + k] = s * iflux
    pidx = np.array([[8 * (m // 5) + lr for lr in LR] for m in range(NPXL)], dtype=float)
    qidx = np.array([[8 * (m % 5) + lc for lc in LC] for m in range(NPXL)], dtype=float)
    for k, s in enumerate(boxes):
        hs = 0.5 * float(s)
        wp = np.maximum(np.minimum(pidx + 0.5, cp + hs) - np.maximum(pidx - 0.5, cp - hs), 0.0)
        wq = np.maximum(np.minimum(qidx + 0.5, cq + hs) - np.maximum(qidx - 0.5, cq - hs), 0.0)
        row[8 + len(radii) + k] = float((wp * wq * sp).sum()) * iflux
    rmax = float(np.hypot(max(cp + 0.5, NS - 0.5 - cp), max(cq + 0.5, NS - 0.5 - cq)))
    status = 0
    for k, f in enumerate(fracs):
        lo, hi = 0.0, rmax
        r = float(np.sqrt(f * flux / (np.pi * max(best, flux / (NS * NS)))))
        if not (lo < r < hi):
            r = 0.5 * (lo + hi)
        g = 0.0
        for it in range(K_ROOT_MAXIT):
            s, d, _ = circle_sum(sp, cp, cq, r, edits, qo)
            g = s * iflux - f
            if abs(g) <= K_ROOT_GOAL:
                break
            if g < 0.0:
                lo = r
            else:
                hi = r
            with np.errstate(all='ignore'):
                rn = r - g / (d * iflux) if d != 0.0 else np.nan
            if not (d > 0.0) or not (lo < rn < hi):
                rn = 0.5 * (lo + hi)
            if rn == r or not (hi > lo) or it == K_ROOT_MAXIT - 1:
                break
            r = rn
        if not (abs(g) <= K_ROOT_TOL):
            status = 1
        row[8 + len(radii) + len(boxes) + k] = r
    row[6] = float(status)
    return row, counts
