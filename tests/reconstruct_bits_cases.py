"""The calls of the bit-identity record of the pipeline's host path (tests/golden/reconstruct_calls_gfx950.npz), shared by
scripts/record_reconstruct_calls.py, which writes the record, and tests/test_gpu_reconstruct_bits.py, which holds a build
to it.

Five rows (L0 within 9-29 m, one three_lgs row) at 495, 690 and 915 nm on grid_pixscale(dim).  Five rows at
chunk_tasks = 2 make chunks of 2, 2 and 1 rows on two lanes: lane 0 accumulates two chunks, lane 1 one, and the lane
sums are added in lane order.  Every case runs on a fresh context (a sequence: on one context, and every call of it
once more on a fresh one, `.cK` against `.fK`).  The cases:

  d128.mixed / d128.f64 / d512.mixed / d256.npl2   the default paths: full-size stage A and the thin-wave kernel; the
          series form with from_lines and the fused tip-tilt spectra; the series form with the several-direction kernel
  opt.*   options at 128^2 mixed (stage_a 2 alone, with head_fusion 0, with support_skip 0, with a row at L0 = 5 m;
          otf_mfma 0, mf_kernel 1, fft_conv 0, prune_eps 0, tier_eps 0, param_copy 0; chunk_tasks 2 with streams 2 and
          1; f64 with chunk_tasks 2)
  field / band / band_nopsf / band_pos / profile   the entry points at 128^2 (mixed, f64) and 512^2 mixed
  simul_psd.npl1/2, simul_psd_profile, psf_from_psd.ndir1/4, convolve   the stage-level calls at 128^2, both precisions
  out.*   output forms at 512^2 mixed: host outputs psf / sum / fit alone and together; device outputs, three calls
          queued back to back over two rotating buffer sets, then sync (the lean path); asynchronous host outputs, five
          calls in flight (one more than NTICKET) waited for in order
  seq.*   sequences at 512^2 mixed: wavelengths A, B, A; masks given, absent, given; npsflin 1, 2, 1; a stage-level call
          between two reconstruct calls; a refused call (MPSFR_E_GRID) between two good ones.  d0t_clears is recorded.

Every `fit` array and the band sums are kept in full (none is above HASH_ABOVE values), every array above HASH_ABOVE
values -- stamps, PSD images, the stamp sums over three wavelengths (4800 values: kept in full, they alone would put the
record above what a committed file may weigh) -- as the SHA-256 of its bytes.
With every case the record holds the number of timed scopes per kernel id of a second run under the `profile` option:
that the same kernels were queued the same number of times.
"""
import hashlib
import os

import numpy as np

from frame_bits_cases import GOLDEN, HASH_ABOVE, bits, digest, le  # noqa: F401  (one byte comparison for both records)

RECORD = os.path.join(GOLDEN, 'reconstruct_calls_gfx950.npz')
H = (100.0, 10000.0)
LB = np.array([495.0, 690.0, 915.0])
LB_B = np.array([520.0, 700.0, 880.0])
SEE = np.array([0.9, 1.1, 0.7, 0.8, 1.3])
GL = np.array([0.6, 0.45, 0.8, 0.7, 0.3])
L0 = np.array([22.0, 13.0, 27.0, 9.5, 28.5])
L0_SHORT = np.array([22.0, 5.0, 27.0, 9.5, 28.5])
THREE = np.array([0, 1, 0, 0, 0], np.uint8)
POS = [(0.0, 0.0), (25.0, -15.0)]
BANDS = [(495.0, 915.0), (600.0, 800.0)]
LAYERS = (np.array([0.0, 3000.0, 12000.0]), np.array([8.0, 15.0, 25.0]), np.array([0.3, 1.2, 2.5]))
CN2 = np.array([[0.5, 0.0, 0.5], [0.7, 0.0, 0.3], [0.2, 0.0, 0.8], [0.6, 0.0, 0.4], [0.9, 0.0, 0.1]])
_rng = np.random.default_rng(20240)
MREC = _rng.uniform(size=(80, 80)) < 0.5
MASKS = (MREC, ~MREC)
STAMPS = _rng.uniform(0.0, 1.0e3, (SEE.size, LB.size, 40, 40))
E_GRID = -3
OUT = ('psf', 'psf_sum', 'fit')


def inputs():
    """Every input array of the record's calls, by name, in a fixed order."""
    return [('lb', LB), ('lb_b', LB_B), ('see', SEE), ('gl', GL), ('l0', L0), ('l0_short', L0_SHORT), ('three', THREE),
            ('h', np.array(H)), ('pos', np.array(POS)), ('bands', np.array(BANDS)), ('cn2', CN2),
            ('mrec', MASKS[0]), ('mres', MASKS[1]), ('stamps', STAMPS)] + \
           [('layers%d' % k, a) for k, a in enumerate(LAYERS)]


def stored(name, a):
    """The output `name` as the record keeps it: in full, or the SHA-256 of its bytes above HASH_ABOVE values"""
    a = le(a)
    if a.size > HASH_ABOVE:
        return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()
    return a


def same(name, got, kept):
    want = stored(name, got)
    return want.dtype == kept.dtype and want.shape == kept.shape and bool(np.array_equal(bits(want), bits(kept)))


def _named(r, prefix=''):
    return {prefix + k: v for k, v in r.items() if v is not None}


def _rec(ctx, lb=LB, l0=L0, **kw):
    return ctx.reconstruct(lb, SEE, GL, l0, THREE, H, **kw)


def _call(**kw):
    return lambda api, ctx: _named(_rec(ctx, **kw))


def _band_w(api):
    return api.band_weights(LB, BANDS)


ENTRIES = {
    'field': lambda api, ctx: ctx.reconstruct_field(LB, SEE, GL, L0, THREE, H, POS),
    'band': lambda api, ctx: ctx.reconstruct_band(LB, _band_w(api), SEE, GL, L0, THREE, H),
    'band_nopsf': lambda api, ctx: ctx.reconstruct_band(LB, _band_w(api), SEE, GL, L0, THREE, H, want_psf=False),
    'band_pos': lambda api, ctx: ctx.reconstruct_band(LB, _band_w(api), SEE, GL, L0, THREE, H, positions=POS),
    'profile': lambda api, ctx: ctx.reconstruct_profile(LB, SEE, GL, L0, CN2, *LAYERS, three_lgs=THREE),
}


def _psd(ctx, npl):
    return ctx.simul_psd(SEE[0], GL[0], L0[0], False, H, npsflin=npl)


def _convolve(api, ctx):
    ctx.set_option('chunk_tasks', 2)
    return {'psf': ctx.convolve_stamps(LB, SEE, GL, L0, STAMPS)}


STAGE = {
    'simul_psd.npl1': lambda api, ctx: {'psd': ctx.simul_psd(SEE[1], GL[1], L0[1], True, H, npsflin=1)},
    'simul_psd.npl2': lambda api, ctx: {'psd': _psd(ctx, 2)},
    'simul_psd_profile': lambda api, ctx: {'psd': ctx.simul_psd_profile(SEE[0], L0[0], CN2[0], *LAYERS, positions=POS)},
    'psf_from_psd.ndir1': lambda api, ctx: {'psf': ctx.psf_from_psd(_psd(ctx, 1), LB)},
    'psf_from_psd.ndir4': lambda api, ctx: {'psf': ctx.psf_from_psd(_psd(ctx, 2), LB)},
    'convolve': _convolve,
}


def _device(api, ctx):
    """three device-output calls (rows rotated per call) over two buffer sets, no synchronisation between them"""
    import torch
    dev = torch.device('cuda:0')
    n, nl = SEE.size, LB.size
    sets = [[torch.full(s, -1.0, dtype=torch.float64, device=dev) for s in ((n, nl, 40, 40), (nl, 40, 40), (n, nl, api.NFIT))]
            for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(3):
        o = np.roll(np.arange(n), k)
        ctx.reconstruct_device(LB, SEE[o], GL[o], L0[o], THREE[o], H, 12.0, 1, None, *[t.data_ptr() for t in sets[k % 2]])
    ctx.sync()
    torch.cuda.synchronize()
    return {'set%d.%s' % (i, k): t.cpu().numpy() for i, s in enumerate(sets) for k, t in zip(OUT, s)}


def _async(api, ctx):
    pend = []
    for k in range(5):
        o = np.roll(np.arange(SEE.size), k)
        pend.append(ctx.reconstruct_async(LB, SEE[o], GL[o], L0[o], THREE[o], H))
    out = {}
    for k, p in enumerate(pend):
        out.update(_named(p.wait(), 'call%d.' % k))
    return out


OUTPUTS = {
    'out.host.psf': _call(want_sum=False, want_fit=False),
    'out.host.sum': _call(want_psf=False, want_fit=False),
    'out.host.fit': _call(want_psf=False, want_sum=False),
    'out.host.all': _call(),
    'out.device': _device,
    'out.async': _async,
}


def _refused(api, ctx):
    try:
        ctx.reconstruct(np.array([300.0]), SEE, GL, L0, THREE, H)
    except api.MpsfrError as e:
        return {'code': np.array([e.code], dtype=np.int32)}
    raise AssertionError('a wavelength whose crop exceeds the grid was accepted')


# sequences: the calls in order, each a function of (api, ctx)
SEQUENCES = {
    'seq.lam_aba': [_call(lb=lb) for lb in (LB, LB_B, LB)],
    'seq.masks': [_call(masks=m) for m in (MASKS, None, MASKS)],
    'seq.npl_121': [_call(npsflin=n) for n in (1, 2, 1)],
    'seq.stage_between': [_call(), STAGE['psf_from_psd.ndir1'], _call()],
    'seq.refused': [_call(), _refused, _call()],
}


def _opt(**opts):
    return (128, 'mixed', opts, _call())


def cases():
    """name -> (dim, precision, options, fn(api, ctx) -> {output: array}) or, for a sequence, a list of such fn"""
    plain = _call()
    c = {'d128.mixed': (128, 'mixed', {}, plain), 'd128.f64': (128, 'f64', {}, plain), 'd512.mixed': (512, 'mixed', {}, plain),
         'd256.npl2': (256, 'mixed', {}, _call(npsflin=2)),
         'opt.stage_a2': _opt(stage_a=2), 'opt.stage_a2.head_fusion0': _opt(stage_a=2, head_fusion=0),
         'opt.stage_a2.support_skip0': _opt(stage_a=2, support_skip=0),
         'opt.stage_a2.l0_5m': (128, 'mixed', {'stage_a': 2}, _call(l0=L0_SHORT)),
         'opt.otf_mfma0': _opt(otf_mfma=0), 'opt.mf_kernel1': _opt(mf_kernel=1), 'opt.fft_conv0': _opt(fft_conv=0),
         'opt.prune_eps0': _opt(prune_eps=0), 'opt.tier_eps0': _opt(tier_eps=0), 'opt.param_copy0': _opt(param_copy=0),
         'opt.chunk2.streams2': _opt(chunk_tasks=2, streams=2), 'opt.chunk2.streams1': _opt(chunk_tasks=2, streams=1),
         'opt.chunk2.f64': (128, 'f64', {'chunk_tasks': 2}, plain)}
    for tag, dim, prec in (('d128.mixed', 128, 'mixed'), ('d128.f64', 128, 'f64'), ('d512.mixed', 512, 'mixed')):
        for k, fn in ENTRIES.items():
            c['%s.%s' % (k, tag)] = (dim, prec, {}, lambda api, ctx, fn=fn: _named(fn(api, ctx)))
    for prec in ('mixed', 'f64'):
        for k, fn in STAGE.items():
            c['%s.%s' % (k, prec)] = (128, prec, {}, fn)
    for k, fn in OUTPUTS.items():
        c[k] = (512, 'mixed', {}, fn)
    for k, fns in SEQUENCES.items():
        c[k] = (512, 'mixed', {}, fns)
    return c


def context(api, case):
    dim, prec, opts = case[:3]
    ctx = api.Context(dim=dim, pixscale=api.grid_pixscale(dim), precision=prec)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def _clears(ctx):
    return np.array([int(ctx.debug_fetch('d0t_clears', (1,))[0])], dtype=np.int64)


def record(api, name, profile=False):
    """The outputs of the case `name`, host form: {'<name>.<output>': array}.  A sequence gives every call on its one
    context as '.cK.' and on a fresh context as '.fK.', and the context's d0t_clears at its end.  profile: the run is
    made under the `profile` option and '<name>.scopes', the timed scopes per kernel id, is all it returns."""
    case = cases()[name]
    ctx = context(api, case)
    if profile:
        ctx.set_option('profile', 1)
        ctx.profile_reset()
    out = {}
    if isinstance(case[3], list):
        for k, fn in enumerate(case[3]):
            out.update(_named(fn(api, ctx), '%s.c%d.' % (name, k)))
            if not profile:
                fresh = context(api, case)
                out.update(_named(fn(api, fresh), '%s.f%d.' % (name, k)))
                fresh.close()
        out[name + '.d0t_clears'] = _clears(ctx)
    else:
        out.update(_named(case[3](api, ctx), name + '.'))
    if profile:
        prof = ctx.profile()
        out = {name + '.scopes': np.array([prof[k][1] for k in ctx.profile_names()], dtype=np.int64)}
    ctx.close()
    return out


def held_to_fresh(keys):
    """the pairs (call on the sequence's context, same call on a fresh context) among the record's names"""
    return [(k, _fresh_name(k)) for k in keys if _fresh_name(k) != k and _fresh_name(k) in keys]


def _fresh_name(k):
    parts = k.split('.')
    if parts[0] == 'seq' and len(parts) > 2 and parts[2][0] == 'c' and parts[2][1:].isdigit():
        parts[2] = 'f' + parts[2][1:]
    return '.'.join(parts)
