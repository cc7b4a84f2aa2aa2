"""The stamps of the bit-identity record of k_fit (tests/golden/fit_rows_gfx950.npz), shared by
scripts/record_fit_rows.py, which writes the record, and tests/test_gpu_fit_bits.py, which holds a build to it.

Only generation parameters are kept, not pixels (a stamp is 12.8 KB), so the stamps must come out the same on every
machine: the exact Moffats use exponents n in {1.5, 2, 2.5, 3}, for which (1 + u / a^2)^-n is a handful of
multiplications, one square root and one division -- operations IEEE 754 rounds exactly -- and no pow, exp or log, whose
last bit depends on the library.  The record holds the SHA-256 of the stamps it was made from; the test compares that
first, so a stamp that differs is told apart from a kernel that does.
"""
import hashlib
import os

import numpy as np

NS = 40
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
RECORD = os.path.join(GOLDEN, 'fit_rows_gfx950.npz')
MODES = ('mixed', 'f64')
CALL_SIZES = (1, 2, 65)


def lane_of(p, q):
    """lane of pixel (p, q) in the pixel map of the model passes: cell (p mod 8, q mod 8) of an 8 x 8 block"""
    return (p & 7) * 8 + (q & 7)


def exact_moffat(peak, p0, q0, a2, n):
    """peak (1 + ((p - p0)^2 + (q - q0)^2) / a2)^-n for n in {1.5, 2, 2.5, 3}, in exactly rounded operations"""
    p, q = np.mgrid[:NS, :NS].astype(np.float64)
    g = 1.0 + ((p - p0) * (p - p0) + (q - q0) * (q - q0)) / a2
    den = {1.5: g * np.sqrt(g), 2.0: g * g, 2.5: g * g * np.sqrt(g), 3.0: g * g * g}[n]
    return peak / den


def golden_stamps():
    g = np.load(os.path.join(GOLDEN, 'g9_profile.npz'))
    d = np.load(os.path.join(GOLDEN, 'g9_profile_field.npz'))
    return np.concatenate([g['a_fin'], g['b_fin'], g['c_fin'], d['d_fin'].reshape(-1, NS, NS)])


def cases():
    """[(name, stamp (40, 40) float64)]: the golden stamps a-d; 64 exact Moffats, one with its brightest pixel in every
    lane class (centres 16..23 x 16..23, a sub-pixel offset of 0 or +-1/4 that keeps the brightest pixel); two equal
    maxima in one quad of lanes, in one row of 16 lanes, in different rows, and four equal maxima; a peak 4 px from an
    edge (the fallback start with the half-maximum count); a NaN pixel, an all-negative and a constant stamp; peaks
    2^-30 and 2^30."""
    out = [('golden_%02d' % k, s) for k, s in enumerate(golden_stamps())]
    assert len(out) == 38
    rng = np.random.default_rng(2025)
    seen = set()
    for p in range(16, 24):
        for q in range(16, 24):
            k = (p - 16) * 8 + (q - 16)
            dp, dq = 0.25 * (k % 3 - 1), 0.25 * ((k // 3) % 3 - 1)
            s = exact_moffat(rng.uniform(0.5, 2.0), p + dp, q + dq, rng.uniform(2.0, 40.0), (1.5, 2.0, 2.5, 3.0)[k % 4])
            assert np.argmax(s) == p * NS + q
            seen.add(lane_of(p, q))
            out.append(('lane_%02d' % lane_of(p, q), s))
    assert len(seen) == 64
    s = exact_moffat(1.0, 20.0, 20.5, 6.0, 2.5)             # lanes 36, 37: one quad
    assert s[20, 20] == s[20, 21] == s.max() and lane_of(20, 20) // 4 == lane_of(20, 21) // 4
    out.append(('tie_quad', s))
    s = exact_moffat(1.0, 20.5, 20.0, 6.0, 2.5)             # lanes 36, 44: one row of 16, two quads
    assert s[20, 20] == s[21, 20] == s.max()
    assert lane_of(20, 20) // 16 == lane_of(21, 20) // 16 and lane_of(20, 20) // 4 != lane_of(21, 20) // 4
    out.append(('tie_row', s))
    s = exact_moffat(1.0, 10.0, 10.0, 3.0, 2.5) + exact_moffat(1.0, 29.0, 29.0, 3.0, 2.5)      # lanes 18, 45
    assert s[10, 10] == s[29, 29] == s.max() and np.argmax(s) == 10 * NS + 10
    assert lane_of(10, 10) // 16 != lane_of(29, 29) // 16
    out.append(('tie_rows', s))
    s = exact_moffat(1.0, 19.5, 23.5, 6.0, 2.0)             # (19, 23) (19, 24) (20, 23) (20, 24): lanes 31, 24, 39, 32
    assert s[19, 23] == s[19, 24] == s[20, 23] == s[20, 24] == s.max()
    out.append(('tie_four', s))
    s = exact_moffat(1.0, 4.25, 20.25, 8.0, 2.5)
    a, b = np.unravel_index(np.argmax(s), s.shape)
    assert min(a, NS - 1 - a, b, NS - 1 - b) == 4
    out.append(('edge_4px', s))
    base = exact_moffat(1.0, 19.75, 20.25, 5.0, 2.5)
    s = base.copy()
    s[7, 11] = np.nan
    out.append(('nan_pixel', s))
    out.append(('negative', -base - 0.125))
    out.append(('constant', np.ones((NS, NS))))
    out.append(('peak_2m30', base * 2.0 ** -30))
    out.append(('peak_2p30', base * 2.0 ** 30))
    return out


def stamps():
    return np.ascontiguousarray(np.array([s for _, s in cases()], dtype=np.float64))


def digest(st):
    return hashlib.sha256(np.ascontiguousarray(st, dtype='<f8').tobytes()).hexdigest()


# The float-stamp instantiation k_fit<float, float> is reached only inside a reconstruct that keeps its final stamps on
# the device as floats (no stamps asked for): the rows of such a call, and of the same call with stamps, are part of the
# record.  Its inputs are these numbers.
CALL_DIM = 512
CALL_LBDA = np.array([465.0, 600.0, 700.0, 930.0])
CALL_SEEING = np.array([0.55, 0.7, 0.85, 1.0, 1.2, 1.45])
CALL_GL = np.array([0.45, 0.6, 0.7, 0.5, 0.8, 0.65])
CALL_L0 = np.array([12.0, 18.0, 25.0, 30.0, 16.0, 22.0])


def record(api, precisions=MODES):
    """The rows of the record from the library `api` loads: {key: (n, 16) float64}.  Keys: rows_<mode>: every case in
    one call; rows_<mode>_first<k>: the first k cases in a call of their own; call_<mode>_stamps / call_<mode>_nostamps:
    the fit rows of the reconstruct above with and without stamps asked for."""
    st = stamps()
    out = {}
    for prec in precisions:
        ctx = api.Context(dim=128, pixscale=0.2, precision=prec)
        out['rows_%s' % prec] = ctx.fit_stamps(st)
        for k in CALL_SIZES:
            out['rows_%s_first%d' % (prec, k)] = ctx.fit_stamps(st[:k])
        ctx.close()
        ctx = api.Context(dim=CALL_DIM, pixscale=api.grid_pixscale(CALL_DIM), precision=prec)
        a = ctx.reconstruct(CALL_LBDA, CALL_SEEING, CALL_GL, CALL_L0)
        b = ctx.reconstruct(CALL_LBDA, CALL_SEEING, CALL_GL, CALL_L0, want_psf=False)
        ctx.close()
        out['call_%s_stamps' % prec] = np.asarray(a['fit'], dtype=np.float64).reshape(-1, 16)
        out['call_%s_nostamps' % prec] = np.asarray(b['fit'], dtype=np.float64).reshape(-1, 16)
    return out
