"""mpmath yardstick of the PSF energy metrics (mpsfr_stamp_metrics), at 60 digits: the referee where the fp64 NumPy
reference (tests/metrics_ref.py) is itself the larger error -- circles of large radius about far centres, stamps of
mixed signs, pixels the circle barely touches.

The area of a pixel inside the circle is the integral of metrics_ref.py (along q, with the antiderivative
H(t) = (t sqrt(r^2 - t^2) + r^2 asin(t / r)) / 2 of sqrt(r^2 - t^2)), not the kernel's sum over pixel corners, so that
it stays independent of the kernel.  Only the pixels the circle cuts are evaluated in mpmath: whether a pixel is whole
(farthest corner inside or on the circle) or empty (nearest point outside or on it) is decided in rational arithmetic,
exactly.  Stamp values, centres and radii are float64, binary rationals: at the working precision (200 bits) every
sum of stamp values here is exact for stamps whose values span less than 2^100.

Areas are cached by (centre, radius), cut pixels are evaluated on demand (an impulse stamp costs one pixel).
"""
from fractions import Fraction

import mpmath
import numpy as np

NS = 40
mp = mpmath.mp.clone()          # (a context of its own: the precision of mpmath.mp, which sympy uses, is left alone)
mp.dps = 60
_HALF = Fraction(1, 2)


def _f(x):
    return mp.mpf(float(x))


class _Circle:
    """The circle of radius r about (cp, cq) on the ns x ns pixel grid: `whole` (bool mask), `cut` (bool mask) and the
    mpmath area of a cut pixel on demand."""

    def __init__(self, cp, cq, r, ns=NS):
        self.cp, self.cq, self.r, self.ns = float(cp), float(cq), float(r), ns
        k = np.arange(ns, dtype=float)
        ay, ax = np.abs(k - self.cp)[:, None], np.abs(k - self.cq)[None, :]
        far2 = (ax + 0.5) ** 2 + (ay + 0.5) ** 2
        near2 = np.maximum(ax - 0.5, 0.0) ** 2 + np.maximum(ay - 0.5, 0.0) ** 2
        r2 = self.r * self.r
        # float64 decides what is clear by 1e-9 relative (the fp64 error of these sums is ~1e-15); the rest exactly
        whole = far2 < r2 * (1.0 - 1e-9)
        empty = near2 > r2 * (1.0 + 1e-9)
        fcp, fcq, fr2 = Fraction(self.cp), Fraction(self.cq), Fraction(self.r) ** 2
        for i, j in zip(*np.nonzero(~whole & ~empty)):
            fy, fx = abs(Fraction(int(i)) - fcp), abs(Fraction(int(j)) - fcq)
            if (fx + _HALF) ** 2 + (fy + _HALF) ** 2 <= fr2:
                whole[i, j] = True
            elif max(fx - _HALF, 0) ** 2 + max(fy - _HALF, 0) ** 2 >= fr2:
                empty[i, j] = True
        self.whole, self.cut = whole, ~whole & ~empty
        self._area, self._Hc = {}, {}

    def _H(self, t):
        """H(t) for |t| <= r."""
        r = _f(self.r)
        return (t * mp.sqrt(r * r - t * t) + r * r * mp.asin(t / r)) / 2

    def _Hedge(self, t):
        if t not in self._Hc:
            self._Hc[t] = self._H(t)
        return self._Hc[t]

    def _level(self, y, a, b):
        """int_a^b clamp(y, -h(x), h(x)) dx for -r <= a <= b <= r."""
        r = _f(self.r)
        yc = min(max(y, -r), r)
        c = mp.sqrt(r * r - yc * yc)
        ia, ib = min(max(a, -c), c), min(max(b, -c), c)
        whole = self._Hedge(b) - self._Hedge(a)
        inner = self._H(ib) - self._H(ia)
        return yc * (ib - ia) + mp.sign(yc) * (whole - inner)

    def area(self, i, j):
        """Area of pixel (i, j) inside the circle (mpf)."""
        if self.whole[i, j]:
            return mp.mpf(1)
        if not self.cut[i, j]:
            return mp.mpf(0)
        key = (int(i), int(j))
        if key not in self._area:
            r, half = _f(self.r), mp.mpf(1) / 2
            y0, y1 = _f(i) - half - _f(self.cp), _f(i) + half - _f(self.cp)
            a = min(max(_f(j) - half - _f(self.cq), -r), r)
            b = min(max(_f(j) + half - _f(self.cq), -r), r)
            self._area[key] = self._level(y1, a, b) - self._level(y0, a, b)
        return self._area[key]

    def areas(self):
        """(ns, ns) object array of every pixel's area."""
        out = np.empty((self.ns, self.ns), dtype=object)
        for i in range(self.ns):
            for j in range(self.ns):
                out[i, j] = self.area(i, j)
        return out


_CIRCLES = {}


def circle(cp, cq, r, ns=NS):
    key = (float(cp), float(cq), float(r), ns)
    if key not in _CIRCLES:
        _CIRCLES[key] = _Circle(*key)
    return _CIRCLES[key]


def overlap(cp, cq, r, ns=NS):
    """(ns, ns) exact areas (mpf) of the pixels inside the circle of radius r about (cp, cq)."""
    return circle(cp, cq, r, ns).areas()


def cut_count(cp, cq, r, ns=NS):
    """Number of pixels the circle cuts, decided exactly."""
    return int(circle(cp, cq, r, ns).cut.sum())


def _msum(values):
    v = np.asarray(values, dtype=float).ravel()
    return mp.fsum(mp.mpf(float(x)) for x in v[v != 0.0])


_FLUX = {}


def _sums(stamp):
    """(flux, sum |I|) of a stamp (mpf), cached by the stamp's bytes."""
    st = np.ascontiguousarray(stamp, dtype=float)
    key = st.tobytes()
    if key not in _FLUX:
        _FLUX[key] = (_msum(st), _msum(np.abs(st)))
    return _FLUX[key]


def flux(stamp):
    return _sums(stamp)[0]


def abs_ratio(stamp):
    """sum |I| / |flux| (float): the factor by which a mixed-sign stamp magnifies a summation error."""
    f, a = _sums(stamp)
    return float(a / abs(f))


def centroid(stamp):
    st = np.asarray(stamp, dtype=float)
    f = flux(st)
    sp = mp.fsum(_f(i) * _msum(st[i]) for i in range(st.shape[0]))
    sq = mp.fsum(_f(j) * _msum(st[:, j]) for j in range(st.shape[1]))
    return sp / f, sq / f


def EE(stamp, center, r):
    """Encircled energy (mpf): the flux inside the circle (what of it is on the stamp) over the flux of the stamp.
    `center` is a pair of float64 (the yardstick takes the centre the kernel was given, or reports)."""
    st = np.asarray(stamp, dtype=float)
    c = circle(center[0], center[1], r, st.shape[0])
    tot = _msum(st[c.whole])
    tot += mp.fsum(c.area(i, j) * _f(st[i, j]) for i, j in zip(*np.nonzero(c.cut & (st != 0.0))))
    return tot / flux(st)


def SQE(stamp, center, s):
    """Ensquared energy in the axis-aligned box of side s (mpf)."""
    st = np.asarray(stamp, dtype=float)
    half, hs = mp.mpf(1) / 2, _f(s) / 2

    def length(c, n):
        c = _f(c)
        return [max(min(_f(k) + half, c + hs) - max(_f(k) - half, c - hs), mp.mpf(0)) for k in range(n)]
    wp, wq = length(center[0], st.shape[0]), length(center[1], st.shape[1])
    tot = mp.fsum(wp[i] * wq[j] * _f(st[i, j]) for i, j in zip(*np.nonzero(st)) if wp[i] != 0 and wq[j] != 0)
    return tot / flux(st)


def r_max(center, ns=NS):
    """Distance from the centre to the farthest pixel corner of the stamp (mpf)."""
    half = mp.mpf(1) / 2
    cp, cq = _f(center[0]), _f(center[1])
    return mp.hypot(max(cp + half, ns - half - cp), max(cq + half, ns - half - cq))
