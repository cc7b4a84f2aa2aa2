"""The stamps of the bit-identity record of the model fits (tests/golden/fit_rows_models_gfx950.npz): k_fit_ell
(fit_stamps_elliptical), k_fit_obs (fit_stamps_observed), k_fit_psf (fit_stamps_psf) and k_fit_group (fit_groups_psf).
Shared by scripts/record_fit_rows.py --set models, which writes the record, and tests/test_gpu_fit_models_bits.py,
which holds a build to it.  The record of k_fit and its cases (fit_bits_cases.py) are separate and unchanged.

As there, only generation parameters are kept and every stamp comes from exactly rounded operations: additions,
multiplications, divisions and square roots (exact_moffat, here up to n = 8 and 16 by repeated squaring, on coordinates
changed linearly with dyadic coefficients for elliptical isophotes), Generator.uniform scaled by powers of two for noise
and variances, and whole-pixel moves and two-term means of the golden stamps g9_profile*.npz for the PSF fits.  The
record holds the SHA-256 of every generated array; the test compares those first.

Every entry point has one variant that is run on its whole set (and in calls of the first 1, 2 and 65 of it); the other
variants run on all the `probe` stamps at the head of the set -- the named cases, which take the rare paths of the
iteration -- and on a share of the seeded rest (every 12th, 16th or 8th stamp), so that the record stays small; the
groups of three and four are eight per variant, the five probes and three seeded ones.
"""
import hashlib
import os

import numpy as np

from fit_bits_cases import GOLDEN, MODES, CALL_SIZES, NS, exact_moffat, golden_stamps     # noqa: F401

RECORD = os.path.join(GOLDEN, 'fit_rows_models_gfx950.npz')
GROUP_MODES = ('free', 'common', 'fixed')


def moffat(peak, p0, q0, a2, n, lin=(1.0, 0.0, 0.0, 1.0)):
    """peak (1 + (x'^2 + y'^2) / a2)^-n with (x', y') = lin (x, y), x = q - q0, y = p - p0, for n in
    {1.5, 2, 2.5, 3, 8, 16}: exactly rounded operations only (lin dyadic: its products are exact)"""
    if lin == (1.0, 0.0, 0.0, 1.0) and n in (1.5, 2.0, 2.5, 3.0):
        return exact_moffat(peak, p0, q0, a2, n)
    p, q = np.mgrid[:NS, :NS].astype(np.float64)
    x, y = q - q0, p - p0
    xs, ys = lin[0] * x + lin[1] * y, lin[2] * x + lin[3] * y
    g = 1.0 + (xs * xs + ys * ys) / a2
    g2 = g * g
    g4 = g2 * g2
    g8 = g4 * g4
    den = {1.5: g * np.sqrt(g), 2.0: g2, 2.5: g2 * np.sqrt(g), 3.0: g2 * g, 8.0: g8, 16.0: g8 * g8}[n]
    return peak / den


def spike(p, q, peak=1.0):
    """narrower than two pixels: a bright pixel with four neighbours at a quarter of it"""
    s = np.zeros((NS, NS))
    s[p, q] = peak
    for a, b in ((p - 1, q), (p + 1, q), (p, q - 1), (p, q + 1)):
        s[a, b] = 0.25 * peak
    return s


N_PROBE = 26          # the stamps at the head of moffat_cases() that take the rare paths: every variant runs them all


def moffat_cases():
    """[(name, stamp, var or None)] for fit_stamps_elliptical (the stamps alone) and fit_stamps_observed.  The first
    N_PROBE: the valley of eta (exact Moffats with n = 16 and 8, which the start eta = 0.4 of the observed fit and of a
    peak near an edge reaches through limited steps, and spikes narrower than two pixels, where eta runs down to the
    Gaussian stop), stamps elongated beyond the |e| bound, a peak 4 px from an edge, NaN / negative / constant stamps,
    peaks 2^-30 and 2^30, pixels masked through NaN and through non-positive or non-finite variance.  Then the golden
    stamps and seeded elliptical Moffats with off-centre peaks, with and without noise."""
    rng = np.random.default_rng(20251)
    noise = lambda k: (rng.uniform(-1.0, 1.0, (NS, NS))) * 2.0 ** -k       # noqa: E731
    variance = lambda: rng.uniform(0.5, 1.5, (NS, NS)) * 2.0 ** -12        # noqa: E731
    out = []
    for k, (n, p0, q0, a2) in enumerate(((16.0, 20.0, 20.0, 64.0), (16.0, 19.25, 21.5, 96.0), (16.0, 5.0, 21.0, 48.0),
                                          (8.0, 20.5, 19.75, 24.0), (16.0, 22.0, 17.25, 160.0), (8.0, 34.0, 20.0, 40.0))):
        s = moffat(1.0 + 0.125 * k, p0, q0, a2, n)
        if k % 2:
            s = s + noise(10)
        out.append(('valley_n%d_%d' % (n, k), s, variance()))
    for k, (p, q) in enumerate(((20, 20), (17, 23), (12, 28), (5, 20), (24, 9), (21, 21))):
        s = spike(p, q, 1.0 + 0.25 * k)
        if k >= 2:
            s = s + moffat(0.0625, p + 0.25, q - 0.25, 12.0, 2.5)
        if k >= 4:
            s = s + noise(9)
        out.append(('spike_%d' % k, s, variance()))
    for k, lin in enumerate(((4.0, 0.0, 0.0, 0.5), (0.5, 0.0, 0.0, 4.0), (2.0, 2.0, -0.25, 0.25), (4.0, 1.0, 0.0, 0.25))):
        out.append(('elongated_%d' % k, moffat(1.0, 20.25, 19.75, 8.0, 2.5, lin) + (noise(11) if k % 2 else 0.0), variance()))
    s = moffat(1.0, 4.25, 20.25, 8.0, 2.5, (1.0, 0.25, 0.0, 1.0))
    a, b = np.unravel_index(np.argmax(s), s.shape)
    assert min(a, NS - 1 - a, b, NS - 1 - b) == 4
    out.append(('edge_4px', s, variance()))
    base = moffat(1.0, 19.75, 20.25, 5.0, 2.5, (1.0, 0.25, -0.125, 0.75))
    s = base.copy()
    s[7, 11] = np.nan
    out.append(('nan_pixel', s, variance()))
    out.append(('negative', -base - 0.125, variance()))
    out.append(('constant', np.ones((NS, NS)), variance()))
    out.append(('peak_2m30', (base + noise(10)) * 2.0 ** -30, variance() * 2.0 ** -60))
    out.append(('peak_2p30', (base + noise(10)) * 2.0 ** 30, variance() * 2.0 ** 60))
    s, v = base + noise(9), variance()
    s[18:23, 25] = np.nan                      # masked through NaN: a column beside the core, and the brightest pixel
    s[20, 20] = np.nan
    out.append(('masked_nan', s, v))
    s, v = base + noise(9), variance()
    v[3:9, 4:30] = 0.0                         # masked through the variance: zero, negative, NaN, infinite
    v[19, 21] = -1.0
    v[21, 19] = np.nan
    v[30, 5:12] = np.inf
    out.append(('masked_var', s, v))
    s, v = moffat(1.5, 20.0, 20.5, 64.0, 16.0) + noise(10), variance()
    s[0:4, :] = np.nan
    v[:, 36:] = 0.0
    out.append(('masked_valley', s, v))
    s, v = spike(19, 22) + noise(10), variance()
    v[10:14, 10:14] = -0.5
    out.append(('masked_spike', s, v))
    assert len(out) == N_PROBE, len(out)
    for k, s in enumerate(golden_stamps()):
        out.append(('golden_%02d' % k, s, variance() * 2.0 ** -8))
    lins = ((1.0, 0.0, 0.0, 1.0), (1.0, 0.25, 0.0, 1.0), (1.0, 0.0, 0.5, 0.75), (0.75, -0.25, 0.25, 1.0), (1.25, 0.5, -0.5, 1.0),
            (1.0, 0.0, 0.0, 0.5), (1.5, 0.0, 0.0, 1.0), (1.0, 0.5, 0.5, 1.0))
    ns = (1.5, 2.0, 2.5, 3.0, 8.0, 16.0)
    for k in range(48):
        p0 = 20.0 + 0.25 * int(rng.integers(-24, 25))
        q0 = 20.0 + 0.25 * int(rng.integers(-24, 25))
        n = ns[k % 6]
        a2 = float(rng.integers(3, 40)) * (4.0 if n >= 8.0 else 1.0)
        s = moffat(rng.uniform(0.5, 2.0), p0, q0, a2, n, lins[(k // 6) % 8])
        if k % 3:
            s = s + noise(8 + k % 5)
        out.append(('moffat_%02d' % k, s, variance()))
    return out


def moved(m, sy, sx):
    """m moved by whole pixels: out[p, q] = m[p - sy, q - sx], zero outside"""
    out = np.zeros_like(m)
    out[max(sy, 0):NS + min(sy, 0), max(sx, 0):NS + min(sx, 0)] = m[max(-sy, 0):NS + min(-sy, 0), max(-sx, 0):NS + min(-sx, 0)]
    return out


def resampled(m, sy, sx, fy, fx):
    """m at the shift (sy + fy/4, sx + fx/4), fy, fx in 0..3: means of whole-pixel moves with dyadic weights"""
    wy, wx = 0.25 * fy, 0.25 * fx
    a = (1.0 - wx) * moved(m, sy, sx) + wx * moved(m, sy, sx + 1)
    b = (1.0 - wx) * moved(m, sy + 1, sx) + wx * moved(m, sy + 1, sx + 1)
    return (1.0 - wy) * a + wy * b


N_PSF_PROBE = 14


def psf_cases():
    """(models (38, 40, 40), [(name, star, var, model index, start shift (2,))]) for fit_stamps_psf.  The first
    N_PSF_PROBE: stars whose shift rests on the +-8 px bound, a NaN pixel, negative and constant stars, scales 2^-30 and
    2^30, pixels masked through NaN and through the variance; then seeded stars of every model stamp."""
    rng = np.random.default_rng(20252)
    models = golden_stamps()
    noise = lambda k: (rng.uniform(-1.0, 1.0, (NS, NS))) * 2.0 ** -k       # noqa: E731
    variance = lambda: rng.uniform(0.5, 1.5, (NS, NS)) * 2.0 ** -30        # noqa: E731
    out = []

    def star(name, j, sy, sx, fy, fx, F, b, nk, start=None):
        s = F * resampled(models[j], sy, sx, fy, fx) + b
        if nk:
            s = s + noise(nk) * F
        st = np.clip(np.array([sy + 0.25 * fy, sx + 0.25 * fx]) if start is None else np.array(start, dtype=float), -8.0, 8.0)
        out.append([name, s, variance(), j, st])

    star('bound_p', 0, 10, 1, 0, 2, 4.0, 2.0 ** -12, 14)
    star('bound_m', 7, -9, -11, 2, 0, 2.0, 0.0, 15)
    star('bound_q', 12, 2, 9, 1, 1, 1.0, 2.0 ** -11, 0, start=(2.0, 8.0))
    star('bound_far', 20, -12, 12, 0, 0, 8.0, 2.0 ** -13, 14, start=(-8.0, 8.0))
    star('nan_pixel', 3, 1, -2, 1, 3, 2.0, 2.0 ** -12, 14)
    out[-1][1][7, 11] = np.nan
    star('negative', 4, 0, 0, 0, 0, -2.0, -2.0 ** -8, 14)
    out.append(['constant', np.ones((NS, NS)), variance(), 5, np.zeros(2)])
    star('scale_2m30', 6, 2, 3, 3, 1, 2.0 ** -30, 2.0 ** -42, 14)
    out[-1][2] = out[-1][2] * 2.0 ** -60
    star('scale_2p30', 8, -3, 1, 2, 2, 2.0 ** 30, 2.0 ** 18, 14)
    out[-1][2] = out[-1][2] * 2.0 ** 60
    star('masked_nan', 9, 1, 1, 2, 1, 2.0, 2.0 ** -12, 13)
    out[-1][1][18:23, 25] = np.nan
    out[-1][1][21, 21] = np.nan
    star('masked_var', 10, -2, 2, 1, 2, 2.0, 2.0 ** -12, 13)
    v = out[-1][2]
    v[3:9, 4:30] = 0.0
    v[18, 22] = -1.0
    v[21, 19] = np.nan
    v[30, 5:12] = np.inf
    star('off_start', 11, 3, -4, 2, 2, 2.0, 2.0 ** -12, 14, start=(0.5, -1.0))
    star('far_start', 13, -5, 5, 1, 3, 1.0, 0.0, 0, start=(-1.0, 1.0))
    star('exact', 14, 0, 0, 0, 0, 1.0, 0.0, 0)
    assert len(out) == N_PSF_PROBE, len(out)
    for k in range(90):
        j = k % len(models)
        star('star_%02d' % k, j, int(rng.integers(-6, 7)), int(rng.integers(-6, 7)), int(rng.integers(0, 4)), int(rng.integers(0, 4)),
             2.0 ** int(rng.integers(-3, 6)), 2.0 ** -12 * int(rng.integers(-2, 5)), (0, 13, 14, 15, 12)[k % 5])
    return models, [tuple(c) for c in out]


GROUP_POS = ((-5.0, -4.0), (4.0, 5.0), (6.5, -6.0), (-3.0, 6.25))
N_GROUP_PROBE = 5


def group_cases(K):
    """(models, [(name, stamp, var, model index, positions (K, 2))]) for fit_groups_psf with K sources.  The first
    N_GROUP_PROBE: a source that rests on the +-8 px bound (status 1 in the modes that fit positions), a singular group (two sources at the same position), a
    NaN pixel with pixels masked through the variance, scales 2^-30 and 2^30; then seeded groups."""
    rng = np.random.default_rng(20260 + K)
    models = golden_stamps()
    out = []

    def group(name, j, pos4, F, b, nk, start=None, vscale=1.0):
        s = np.full((NS, NS), b)
        for k in range(K):
            y4, x4 = pos4[k]
            s = s + F[k] * resampled(models[j], y4 >> 2, x4 >> 2, y4 & 3, x4 & 3)
        if nk:
            s = s + rng.uniform(-1.0, 1.0, (NS, NS)) * 2.0 ** -nk * F[0]
        st = np.array([(0.25 * y, 0.25 * x) for y, x in pos4[:K]]) if start is None else np.array(start, dtype=float)[:K]
        out.append([name, s, rng.uniform(0.5, 1.5, (NS, NS)) * 2.0 ** -30 * vscale, j, np.clip(st, -8.0, 8.0)])

    base = [(int(4 * y), int(4 * x)) for y, x in GROUP_POS]
    amp = (2.0, 1.0, 0.5, 1.5)
    # (the source lies 11 px out and starts on the bound: every step towards it is refused by the domain)
    group('bound', 2, [(44, -16)] + base[1:], amp, 2.0 ** -12, 14, start=[(8.0, -4.0)] + list(GROUP_POS[1:]))
    group('singular', 5, [base[0], base[0]] + base[2:], amp, 2.0 ** -12, 14)
    group('masked', 9, base, amp, 2.0 ** -12, 14)
    out[-1][1][7, 11] = np.nan
    out[-1][2][3:9, 4:30] = 0.0
    out[-1][2][25, 25] = -1.0
    group('scale_2m30', 11, base, [a * 2.0 ** -30 for a in amp], 2.0 ** -42, 14, vscale=2.0 ** -60)
    group('scale_2p30', 13, base, [a * 2.0 ** 30 for a in amp], 2.0 ** 18, 14, vscale=2.0 ** 60)
    assert len(out) == N_GROUP_PROBE
    for k in range(67 if K == 2 else 3):
        pos4 = [(y + int(rng.integers(-6, 7)), x + int(rng.integers(-6, 7))) for y, x in base]
        F = [2.0 ** int(rng.integers(-1, 3)) * a for a in amp]
        start = [(0.25 * y + 0.25 * int(rng.integers(-2, 3)), 0.25 * x + 0.25 * int(rng.integers(-2, 3))) for y, x in pos4]
        group('group_%02d' % k, (3 * k + K) % len(models), pos4, F, 2.0 ** -12 * int(rng.integers(0, 4)), (14, 13, 0, 15)[k % 4],
              start=start if k % 2 else None)
    return models, [tuple(c) for c in out]


def share(n_probe, n, i, nvar):
    """the rows a variant runs: all the probes and every nvar-th of the rest, from the i-th on"""
    return list(range(n_probe)) + list(range(n_probe + i, n, nvar))


def observed_variants():
    """[(key, background, circular, with variance, rows or None for the whole set)]"""
    out = []
    n = len(moffat_cases())
    for i, (bg, circ, wv) in enumerate((b, c, w) for b in (True, False) for c in (True, False) for w in (True, False)):
        whole = bg and not circ and wv
        out.append(('b%dc%dv%d' % (bg, circ, wv), bg, circ, wv, None if whole else share(N_PROBE, n, i, 12)))
    return out


def psf_variants():
    """[(key, background, fixed_shift, given (psf_index and shift; without: one model stamp per star and, unless the
    shift is fixed, the start from the brightest pixels), with variance, rows or None)]"""
    out = []
    n = len(psf_cases()[1])
    combos = [(b, f, g, w) for b in (True, False) for f in (False, True) for g in (True, False) for w in (True, False)]
    for i, (bg, fx, gv, wv) in enumerate(combos):
        whole = bg and not fx and gv and wv
        out.append(('b%df%dg%dv%d' % (bg, fx, gv, wv), bg, fx, gv, wv, None if whole else share(N_PSF_PROBE, n, i, 16)))
    return out


def group_variants():
    """[(key, K, mode, background, with variance, rows or None)]"""
    out = []
    i = 0
    for K in (2, 3, 4):
        n = len(group_cases(K)[1])
        for mode in GROUP_MODES:
            for bg in (True, False):
                whole = K == 2 and mode == 'free' and bg
                out.append(('k%d_%s_b%d' % (K, mode, bg), K, mode, bg, i % 2 == 0, None if whole or K > 2 else share(N_GROUP_PROBE, n, i, 8)))
                i += 1
    return out


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype='<f8').tobytes())
    return h.hexdigest()


_CACHE = {}


def inputs():
    """every generated array, made once: {'moffat': (names, stamps, var), 'psf': (models, names, stars, var, index,
    shift), 'group<K>': (models, names, stamps, var, index, positions)}"""
    if not _CACHE:
        mc = moffat_cases()
        _CACHE['moffat'] = ([c[0] for c in mc], np.array([c[1] for c in mc]), np.array([c[2] for c in mc]))
        models, pc = psf_cases()
        _CACHE['psf'] = (models, [c[0] for c in pc], np.array([c[1] for c in pc]), np.array([c[2] for c in pc]),
                         np.array([c[3] for c in pc], dtype=np.int32), np.array([c[4] for c in pc]))
        for K in (2, 3, 4):
            models, gc = group_cases(K)
            _CACHE['group%d' % K] = (models, [c[0] for c in gc], np.array([c[1] for c in gc]), np.array([c[2] for c in gc]),
                                     np.array([c[3] for c in gc], dtype=np.int32), np.array([c[4] for c in gc]))
    return _CACHE


def digests():
    """{name: SHA-256} of the generated arrays of every entry point"""
    inp = inputs()
    out = {'sha256_moffat': _sha(inp['moffat'][1], inp['moffat'][2])}
    m, _, s, v, ix, sh = inp['psf']
    out['sha256_psf'] = _sha(m, s, v, ix, sh)
    for K in (2, 3, 4):
        m, _, s, v, ix, sh = inp['group%d' % K]
        out['sha256_group%d' % K] = _sha(m, s, v, ix, sh)
    return out


def names():
    inp = inputs()
    return {'names_moffat': inp['moffat'][0], 'names_psf': inp['psf'][1], 'names_group2': inp['group2'][1],
            'names_group3': inp['group3'][1], 'names_group4': inp['group4'][1]}


def _take(a, rows):
    return a if rows is None else a[rows]


def run_elliptical(ctx, first=None):
    """fit_stamps_elliptical in its device form: the entry point takes any data, the host wrapper refuses a NaN pixel"""
    import torch
    st = inputs()['moffat'][1][:first]
    dev = torch.device('cuda:0')
    ts = torch.from_numpy(np.ascontiguousarray(st, dtype=np.float64)).to(dev)
    tf = torch.full((len(st), 24), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_stamps_elliptical_device(len(st), ts.data_ptr(), tf.data_ptr())
    ctx.sync()
    return tf.cpu().numpy()


def run_observed(ctx, variant, first=None):
    _, bg, circ, wv, rows = variant
    _, st, var = inputs()['moffat']
    st, var = _take(st, rows)[:first], _take(var, rows)[:first]
    return ctx.fit_stamps_observed(st, var=var if wv else None, background=bg, circular=circ)


def run_psf(ctx, variant, first=None):
    _, bg, fx, gv, wv, rows = variant
    models, _, st, var, ix, sh = inputs()['psf']
    st, var, ix, sh = (_take(a, rows)[:first] for a in (st, var, ix, sh))
    if gv:
        return ctx.fit_stamps_psf(st, models, var=var if wv else None, psf_index=ix, shift=sh, background=bg, fixed_shift=fx)
    return ctx.fit_stamps_psf(st, models[ix], var=var if wv else None, shift=sh if fx else None, background=bg, fixed_shift=fx)


def run_group(ctx, variant, first=None):
    _, K, mode, bg, wv, rows = variant
    models, _, st, var, ix, sh = inputs()['group%d' % K]
    st, var, ix, sh = (_take(a, rows)[:first] for a in (st, var, ix, sh))
    return ctx.fit_groups_psf(st, models, sh, var=var if wv else None, psf_index=ix, background=bg, mode=mode)


def record(api, precisions=MODES):
    """The rows of the record from the library `api` loads: {key: (n, columns) float64}, keys ell_<mode>,
    obs_<mode>_<variant>, psf_<mode>_<variant>, grp_<mode>_<variant>."""
    out = {}
    for prec in precisions:
        ctx = api.Context(dim=128, pixscale=0.2, precision=prec)
        out['ell_%s' % prec] = run_elliptical(ctx)
        for v in observed_variants():
            out['obs_%s_%s' % (prec, v[0])] = run_observed(ctx, v)
        for v in psf_variants():
            out['psf_%s_%s' % (prec, v[0])] = run_psf(ctx, v)
        for v in group_variants():
            out['grp_%s_%s' % (prec, v[0])] = run_group(ctx, v)
        ctx.close()
    return out


def subcalls(api, prec):
    """[(key of the whole-set variant, k, rows of a call of its first k stamps)] for k in CALL_SIZES"""
    out = []
    ctx = api.Context(dim=128, pixscale=0.2, precision=prec)
    vo = [v for v in observed_variants() if v[-1] is None][0]
    vp = [v for v in psf_variants() if v[-1] is None][0]
    vg = [v for v in group_variants() if v[-1] is None][0]
    for k in CALL_SIZES:
        out.append(('ell_%s' % prec, k, run_elliptical(ctx, k)))
        out.append(('obs_%s_%s' % (prec, vo[0]), k, run_observed(ctx, vo, k)))
        out.append(('psf_%s_%s' % (prec, vp[0]), k, run_psf(ctx, vp, k)))
        out.append(('grp_%s_%s' % (prec, vg[0]), k, run_group(ctx, vg, k)))
    ctx.close()
    return out


def row_name(key, j):
    """the name of row j of the array `key`"""
    kind, _, var = key.split('_', 2) if key.count('_') >= 2 else (key.split('_')[0], None, None)
    nm = names()
    if kind == 'ell':
        return nm['names_moffat'][j]
    if kind == 'obs':
        rows = [v for v in observed_variants() if v[0] == var][0][-1]
        return nm['names_moffat'][j if rows is None else rows[j]]
    if kind == 'psf':
        rows = [v for v in psf_variants() if v[0] == var][0][-1]
        return nm['names_psf'][j if rows is None else rows[j]]
    v = [v for v in group_variants() if v[0] == var][0]
    return nm['names_group%d' % v[1]][j if v[-1] is None else v[-1][j]]
