"""NumPy yardstick of the PSF energy metrics (mpsfr_stamp_metrics, include/mpsfr.h), fp64.

Pixel (p, q) of a stamp is the unit square [p - 1/2, p + 1/2] x [q - 1/2, q + 1/2] (rows p, columns q: the coordinates
of the Moffat fits).  Written independently of the kernel: the area of a pixel inside a circle is not summed over pixel
corners but integrated along q,

    A = int_{q0}^{q1} [clamp(p1, -h, h) - clamp(p0, -h, h)] dx,   h(x) = sqrt(r^2 - x^2) on |x| <= r,

with the antiderivative H(t) = (t sqrt(r^2 - t^2) + r^2 arcsin(t / r)) / 2 of h: the level y cuts the circle at
|x| = c(y) = sqrt(r^2 - y^2); clamp(y, -h, h) is y inside |x| <= c and sgn(y) h outside.
"""
import numpy as np

NS = 40


def _H(t, r):
    t = np.clip(t, -r, r)
    return 0.5 * (t * np.sqrt(np.maximum(r * r - t * t, 0.0)) + r * r * np.arcsin(t / r))


def _level_integral(y, a, b, r):
    """int_a^b clamp(y, -h(x), h(x)) dx for -r <= a <= b <= r (arrays), level(s) y."""
    yc = np.clip(y, -r, r)
    c = np.sqrt(np.maximum(r * r - yc * yc, 0.0))
    ia, ib = np.clip(a, -c, c), np.clip(b, -c, c)                # the part of [a, b] inside |x| <= c
    whole = _H(b, r) - _H(a, r)
    inner = _H(ib, r) - _H(ia, r)
    return yc * (ib - ia) + np.sign(yc) * (whole - inner)


def circle_overlap(cp, cq, r, ns=NS):
    """(ns, ns) areas of the pixels inside the circle of radius r about (cp, cq), exact."""
    r = float(r)
    p, q = np.mgrid[0:ns, 0:ns].astype(float)
    y0, y1 = p - 0.5 - cp, p + 0.5 - cp
    a, b = np.clip(q - 0.5 - cq, -r, r), np.clip(q + 0.5 - cq, -r, r)
    area = _level_integral(y1, a, b, r) - _level_integral(y0, a, b, r)
    return np.clip(area, 0.0, 1.0)


def box_overlap(cp, cq, s, ns=NS):
    """(ns, ns) areas of the pixels inside the axis-aligned box of side s centred on (cp, cq)."""
    ax = np.arange(ns, dtype=float)

    def length(c):
        return np.clip(np.minimum(ax + 0.5, c + 0.5 * s) - np.maximum(ax - 0.5, c - 0.5 * s), 0.0, None)
    return length(cp)[:, None] * length(cq)[None, :]


def centroid(stamp):
    st = np.asarray(stamp, dtype=float)
    p, q = np.mgrid[0:st.shape[0], 0:st.shape[1]].astype(float)
    f = st.sum()
    return (p * st).sum() / f, (q * st).sum() / f


def EE(stamp, center, r):
    """Encircled energy: the flux inside the circle (what of it is on the stamp) over the flux of the stamp."""
    st = np.asarray(stamp, dtype=float)
    return float((circle_overlap(center[0], center[1], r, st.shape[0]) * st).sum() / st.sum())


def SQE(stamp, center, s):
    """Ensquared energy in the box of side s."""
    st = np.asarray(stamp, dtype=float)
    return float((box_overlap(center[0], center[1], s, st.shape[0]) * st).sum() / st.sum())


def r_max(center, ns=NS):
    """Distance from the centre to the farthest pixel corner of the stamp."""
    return float(np.hypot(max(center[0] + 0.5, ns - 0.5 - center[0]), max(center[1] + 0.5, ns - 0.5 - center[1])))


def ee_radius(stamp, center, f, tol=1e-13):
    """An r with |EE(r) - f| <= tol, by bisection on [0, r_max] (unique on a non-negative stamp)."""
    lo, hi = 0.0, r_max(center, np.asarray(stamp).shape[0])
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        g = EE(stamp, center, mid) - f
        if abs(g) <= tol or mid in (lo, hi):
            return mid
        if g < 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def metrics(stamp, radii=(), boxes=(), fractions=(), center=None):
    """dict(flux, peak, peak_p, peak_q, center, ee, sqe, r_ee) of one stamp (all lengths in pixels)."""
    st = np.asarray(stamp, dtype=float)
    c = centroid(st) if center is None else (float(center[0]), float(center[1]))
    k = int(np.argmax(st))
    return dict(flux=float(st.sum()), peak=float(st.flat[k]), peak_p=k // st.shape[1], peak_q=k % st.shape[1], center=c,
                ee=np.array([EE(st, c, r) for r in radii]), sqe=np.array([SQE(st, c, s) for s in boxes]),
                r_ee=np.array([ee_radius(st, c, f) for f in fractions]))
