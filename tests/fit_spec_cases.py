"""The star cubes of the bit-identity record of k_fit_spec (tests/golden/fit_rows_spec_gfx950.npz; fit_spectra_psf).
Shared by scripts/record_fit_rows.py --set spec, which writes the record, and tests/test_gpu_fit_spec_bits.py, which
holds a build to it.  The records of k_fit and of the other model fits, and their cases, are separate and unchanged.

As in fit_models_cases.py only generation parameters are kept, and every array comes from exactly rounded operations:
whole-pixel moves and two-term means of the golden stamps g9_profile*.npz (resampled), products by powers of two, and
Generator.uniform scaled by powers of two for noise and variances.  The record holds the SHA-256 of every generated
array; the test compares those first.

A set per number of layers nl in LAYERS: with 4 waves per star, nl = 1 and 2 leave waves without a layer, nl = 5 gives
one wave two layers and nl = 9 gives one wave three and the others two.  Every variant runs every star of its set.
The mixed context runs the fp64 kernel, so the record holds one array per variant and both modes are held to it.
"""
import hashlib
import os

import numpy as np

from fit_bits_cases import GOLDEN, MODES, NS, golden_stamps     # noqa: F401
from fit_models_cases import resampled

RECORD = os.path.join(GOLDEN, 'fit_rows_spec_gfx950.npz')
LAYERS = (1, 2, 5, 9)
N_CUBES = 4               # model cubes per nl
CALL_SIZES = (1, 2)       # calls of the first k stars (and the whole set, which is the record itself)
NFIT_SPEC, NFIT_SPEC_LAYER = 16, 10


def layer_x(nl):
    """the abscissa of the drift, -1 .. 1 in equal dyadic steps (nl - 1 in {1, 4, 8})"""
    return np.array([(2.0 * l - (nl - 1)) / (nl - 1) for l in range(nl)]) if nl > 1 else np.zeros(1)


def model_cubes(nl):
    """(N_CUBES, nl, 40, 40): golden stamps times a power of two that changes from layer to layer"""
    g = golden_stamps()
    return np.array([[g[(5 * c + 3 * l) % len(g)] * 2.0 ** ((l + c) % 3 - 1) for l in range(nl)] for c in range(N_CUBES)])


def spec_cases(nl):
    """[(name, cube (nl, 40, 40), var, model cube index, start (2,))] for fit_spectra_psf with nl layers: a star with
    one all-NaN layer (left out with layer status 2), with masked pixels (NaN, and through the variance), with an
    infinite pixel (its layer is left out), with every layer left out (refused), peaks 2^-30 and 2^30, a peak of 2^-50
    (refused), a star 12 px from its model (it ends on the bound); then seeded noisy stars, drifting and not."""
    rng = np.random.default_rng(20270 + nl)
    models = model_cubes(nl)
    x = layer_x(nl)
    out = []

    def star(name, c, pos4, drift, F, b, nk, start=None):
        """position pos4 (quarter pixels) + drift (whole pixels) x_l; amplitude F 2^-(l mod 2) and background b"""
        cube = np.empty((nl, NS, NS))
        for l in range(nl):
            y4, x4 = (int(pos4[0] + 4 * drift[0] * x[l]), int(pos4[1] + 4 * drift[1] * x[l]))
            Fl = F * 2.0 ** -(l % 2)
            cube[l] = Fl * resampled(models[c, l], y4 >> 2, x4 >> 2, y4 & 3, x4 & 3) + b
            if nk:
                cube[l] += rng.uniform(-1.0, 1.0, (NS, NS)) * 2.0 ** -nk * F
        st = np.array([0.25 * pos4[0], 0.25 * pos4[1]]) if start is None else np.array(start, dtype=float)
        out.append([name, cube, rng.uniform(0.5, 1.5, (nl, NS, NS)) * 2.0 ** -30, c, np.clip(st, -8.0, 8.0)])

    star('nan_layer', 0, (5, -6), (1, 0), 2.0, 2.0 ** -12, 14)
    out[-1][1][nl // 2] = np.nan
    star('masked', 1, (-7, 9), (0, 1), 2.0, 2.0 ** -12, 13)
    out[-1][1][:, 18:23, 25] = np.nan
    out[-1][1][0, 21, 21] = np.nan
    v = out[-1][2]
    v[:, 3:9, 4:30] = 0.0
    v[0, 18, 22] = -1.0
    v[nl - 1, 21, 19] = np.nan
    v[nl // 2, 30, 5:12] = np.inf
    star('inf_pixel', 2, (3, 2), (0, 0), 1.0, 2.0 ** -12, 14)
    out[-1][1][nl - 1, 7, 11] = np.inf
    star('all_left_out', 3, (0, 0), (0, 0), 1.0, 0.0, 14)
    out[-1][1][:, 5, 5] = -np.inf
    star('peak_2m30', 0, (9, 13), (1, -1), 2.0 ** -30, 2.0 ** -42, 14)
    out[-1][2] = out[-1][2] * 2.0 ** -60
    star('peak_2p30', 1, (-11, 6), (-1, 1), 2.0 ** 30, 2.0 ** 18, 14)
    out[-1][2] = out[-1][2] * 2.0 ** 60
    star('peak_2m50', 2, (0, 4), (0, 0), 2.0 ** -50, 0.0, 14)
    out[-1][2] = out[-1][2] * 2.0 ** -100
    star('far_12px', 3, (-48, 48), (0, 0), 8.0, 2.0 ** -13, 14, start=(-8.0, 8.0))
    for k in range(4):
        pos4 = (int(rng.integers(-24, 25)), int(rng.integers(-24, 25)))
        drift = (int(rng.integers(-1, 2)), int(rng.integers(-1, 2))) if k % 2 else (0, 0)
        st = (0.25 * pos4[0] + 0.25 * int(rng.integers(-2, 3)), 0.25 * pos4[1] + 0.25 * int(rng.integers(-2, 3)))
        star('star_%d' % k, k % N_CUBES, pos4, drift, 2.0 ** int(rng.integers(-3, 6)), 2.0 ** -12 * int(rng.integers(-2, 5)),
             (11, 12, 13, 10)[k], start=st if k >= 2 else None)
    return [tuple(c) for c in out]


def variants():
    """[(key, nl, background, drift, with variance, given (psf_index and shift; without: one model cube per star and
    the start from the brightest pixels of the collapsed images))]: background x drift x variance at nl = 5 and one of
    them with psf_index and shift; background x drift at nl = 2 and background at nl = 1, the variance alternating;
    the two opposite corners at nl = 9."""
    out = [('l5b%dd%dv%dg0' % (b, d, w), 5, b, d, w, False) for b in (True, False) for d in (True, False) for w in (True, False)]
    out.append(('l5b1d1v1g1', 5, True, True, True, True))
    out += [('l2b%dd%dv%dg0' % (b, d, (b + d) % 2), 2, b, d, (b + d) % 2 == 1, False) for b in (True, False) for d in (True, False)]
    out += [('l1b1d0v1g0', 1, True, False, True, False), ('l1b0d0v0g0', 1, False, False, False, False)]
    out += [('l9b1d1v1g0', 9, True, True, True, False), ('l9b0d0v0g0', 9, False, False, False, False)]
    return out


SUBCALL_KEYS = ('l5b1d1v1g0', 'l9b1d1v1g0', 'l5b1d1v1g1')


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype='<f8').tobytes())
    return h.hexdigest()


_CACHE = {}


def inputs():
    """every generated array, made once: {nl: (x, model cubes, names, cubes, var, index, start)}"""
    if not _CACHE:
        for nl in LAYERS:
            sc = spec_cases(nl)
            _CACHE[nl] = (layer_x(nl), model_cubes(nl), [c[0] for c in sc], np.array([c[1] for c in sc]),
                          np.array([c[2] for c in sc]), np.array([c[3] for c in sc], dtype=np.int32), np.array([c[4] for c in sc]))
    return _CACHE


def digests():
    """{name: SHA-256} of the generated arrays of every nl"""
    return {'sha256_spec%d' % nl: _sha(x, m, s, v, ix, sh) for nl, (x, m, _, s, v, ix, sh) in inputs().items()}


def names():
    return {'names_spec%d' % nl: inp[2] for nl, inp in inputs().items()}


def run(ctx, variant, first=None):
    """the rows of a variant, head and layers side by side: (n, 16 + 10 nl)"""
    _, nl, bg, drift, wv, given = variant
    x, models, _, st, var, ix, sh = inputs()[nl]
    st, var, ix, sh = (a[:first] for a in (st, var, ix, sh))
    kw = dict(var=var if wv else None, background=bool(bg), x=x if drift else None)
    if given:
        head, layers = ctx.fit_spectra_psf(st, models, psf_index=ix, shift=sh, **kw)
    else:
        head, layers = ctx.fit_spectra_psf(st, models[ix], **kw)
    return np.concatenate([head, layers.reshape(len(st), -1)], axis=1)


def record(api, prec):
    """The rows of the record from the library `api` loads, in the precision mode `prec`: {'spec_<variant>': rows}"""
    ctx = api.Context(dim=128, pixscale=0.2, precision=prec)
    out = {'spec_%s' % v[0]: run(ctx, v) for v in variants()}
    ctx.close()
    return out


def subcalls(api, prec):
    """[(key, k, rows of a call of the first k stars of that variant)] for k in CALL_SIZES"""
    ctx = api.Context(dim=128, pixscale=0.2, precision=prec)
    out = [('spec_%s' % v[0], k, run(ctx, v, k)) for v in variants() if v[0] in SUBCALL_KEYS for k in CALL_SIZES]
    ctx.close()
    return out


def row_name(key, j):
    """the name of row j of the array `key`"""
    nl = [v[1] for v in variants() if 'spec_' + v[0] == key][0]
    return names()['names_spec%d' % nl][j]
