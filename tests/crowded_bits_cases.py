"""The calls of the bit-identity record of the crowded-field fits (tests/golden/crowded_calls_gfx950.npz), shared by
scripts/record_crowded_calls.py, which writes the record, and tests/test_gpu_crowded_bits.py, which holds a build to it:
mpsfr_fit_frame_psf, mpsfr_fit_frame_psf_free, mpsfr_fit_cube_psf and mpsfr_fit_cube_psf_free on the smallest scenes
the suite owns, every case across one branch or loop border of the one-workgroup step kernels (k_ff_step, k_fr_step,
k_cf_step).  Nothing new is drawn:

  frame     frame_span_cases.live_lattice() (220 x 223, radius 3), its first 1024 stars and all 1089 with the constant,
            all 1089 without: nu on both sides of the 1024 threads.  Outputs: rows, head, resid.
  free      frame_free_ref.displaced_scene(True) (97 x 150, 34 stars): (var, background) in all four at the defaults;
            max_outer = 0; max_outer = 2 with max_iter = 3; max_step = 0.05 with max_outer = 1 (CLIPPED); max_move = 0.2
            with the TIGHT parameters of test_gpu_frame_free.py (BOUND); min_snr = 50 (some HELD) and 1e12 (nobody free:
            the outer loop ends in INIT); the image all NaN (nothing fitted); and the whole lattice with max_outer = 2:
            3268 unknowns, four trips of the 1024 threads.  Outputs: rows, shifts, head, resid.
  cube      cube_free_cases.cube(True) (3 layers) with and without the constant at layer_batch 0 and 1.  Outputs: rows,
            head, resid.
  cubefree  cube_free_cases.cube(True): (var, background) in all four; max_outer = 0; max_step = 0.05 with max_outer = 1;
            max_move = 0.2; two_layers('nan') (a dead layer); two_layers('faint') at min_snr 3 and 0 (one layer carries
            the star / both); frame_span_cases.deep_cube() (1025 layers) with max_outer 0 and 2: the loops over the
            layers and their sum past 1024.  Outputs: rows, pos, shifts, head, call, resid.

Every output of every call is in the record.  frame_bits_cases.stored keeps a frame above HASH_ABOVE values as the
SHA-256 of its bytes; here EVERY output above HASH_ABOVE values is kept so (kept() below) -- the residual frames and
cubes, and the rows and heads of the 1024- and 1089-star lists and of the 1025 layers, which in full would be 70 to
130 KB each --, every other array in full: the rows of all the 34-star cases among them.
"""
import os

import numpy as np

import cube_free_cases as Q
import frame_bits_cases as B
import frame_free_ref as G
import frame_span_cases as S
from frame_bits_cases import HASH_ABOVE, bits, digest, same, stored

RECORD = os.path.join(B.GOLDEN, 'crowded_calls_gfx950.npz')
MODES = B.MODES
CALLS = ('frame', 'free', 'cube', 'cubefree')
OUTPUTS = {'frame': ('rows', 'head', 'resid'), 'free': ('rows', 'shifts', 'head', 'resid'),
           'cube': ('rows', 'head', 'resid'), 'cubefree': ('rows', 'pos', 'shifts', 'head', 'call', 'resid')}
TIGHT = dict(max_iter=200, tol=1e-12, max_outer=12, pos_tol=1e-9, background=False)      # test_gpu_frame_free.py's
context = B.context
_SCENES = {}


def scene(key):
    """The input arrays of a case, once per key."""
    if key not in _SCENES:
        if key.startswith('lattice'):
            s = S.head_of(S.live_lattice(), int(key[7:]))
        elif key == 'displaced':
            s = G.displaced_scene(True)
        elif key == 'nan_image':
            s = G.displaced_scene(True)
            s = dict(s, image=np.full_like(s['image'], np.nan))
        elif key == 'cube':
            s = Q.cube(True)
        elif key == 'deep':
            s = S.deep_cube()
        else:
            s = Q.two_layers(key)
        _SCENES[key] = s
    return _SCENES[key]


def _var_back():
    return [('%s.%s' % ('var' if v else 'unit', 'back' if b else 'noback'), dict(with_var=v, background=b))
            for v in (True, False) for b in (True, False)]


def cases():
    """name -> (scene key, keyword arguments of the call's wrapper below), in the order of the record"""
    out = {}
    for name, (m, back) in (('1024_back', (1024, True)), ('1089_back', (1089, True)), ('1089_noback', (1089, False))):
        out['frame.' + name] = ('lattice%d' % m, dict(radius=S.LATTICE_RADIUS, background=back))
    for name, kw in _var_back():
        out['free.' + name] = ('displaced', kw)
    out['free.outer0'] = ('displaced', dict(max_outer=0))
    out['free.outer2_iter3'] = ('displaced', dict(max_outer=2, max_iter=3))
    out['free.clipped'] = ('displaced', dict(max_step=0.05, max_outer=1))
    out['free.bound'] = ('displaced', dict(TIGHT, max_move=0.2))
    out['free.snr50'] = ('displaced', dict(min_snr=50.0))
    out['free.snr1e12'] = ('displaced', dict(min_snr=1e12))
    out['free.nan'] = ('nan_image', {})
    out['free.lattice'] = ('lattice1089', dict(radius=S.LATTICE_RADIUS, background=True, max_outer=2))
    for back in (True, False):
        for batch in (0, 1):
            out['cube.%s.batch%d' % ('back' if back else 'noback', batch)] = ('cube', dict(background=back,
                                                                                           layer_batch=batch))
    for name, kw in _var_back():
        out['cubefree.' + name] = ('cube', kw)
    out['cubefree.outer0'] = ('cube', dict(max_outer=0))
    out['cubefree.clipped'] = ('cube', dict(max_step=0.05, max_outer=1))
    out['cubefree.bound'] = ('cube', dict(max_move=0.2))
    out['cubefree.nan_layer'] = ('nan', {})
    out['cubefree.faint_snr3'] = ('faint', dict(min_snr=3.0))
    out['cubefree.faint_snr0'] = ('faint', dict(min_snr=0.0))
    out['cubefree.deep_outer0'] = ('deep', dict(radius=S.DEEP_RADIUS, max_outer=0))
    out['cubefree.deep_outer2'] = ('deep', dict(radius=S.DEEP_RADIUS, max_outer=2))
    return out


FRAME_INPUTS = ('image', 'var', 'psf', 'index', 'origin', 'shift')
CUBE_INPUTS = ('cube', 'var', 'psf', 'index', 'origin', 'shift', 'layer_shift')


def inputs():
    """Every input array of the record's calls, by name, in a fixed order."""
    out = []
    for key in sorted({k for k, _ in cases().values()}):
        s = scene(key)
        out += [(key + '.' + k, s[k]) for k in (CUBE_INPUTS if 'cube' in s else FRAME_INPUTS)]
    return out


def kept(name, a):
    """The output `name` as the record keeps it: frame_bits_cases.stored with every output counted as a frame, that is
    the SHA-256 of its bytes above HASH_ABOVE values and the array in full below"""
    return stored(name + '.frame', a)


def equal(name, got, rec):
    """does the output `got` equal the record's entry `rec` for `name`, bit for bit?"""
    return same(name + '.frame', got, rec)


def _frame(ctx, s, with_var=True, **kw):
    return ctx.fit_frame_psf(s['image'], s['psf'], s['origin'], var=s['var'] if with_var else None, shift=s['shift'],
                             psf_index=s['index'], return_residual=True, **kw)


def _free(ctx, s, with_var=True, **kw):
    return ctx.fit_frame_psf_free(s['image'], s['psf'], s['origin'], var=s['var'] if with_var else None,
                                  shift=s['shift'], psf_index=s['index'], return_residual=True, **kw)


def _cube(ctx, c, with_var=True, **kw):
    return ctx.fit_cube_psf(c['cube'], c['psf'], c['origin'], var=c['var'] if with_var else None, shift=c['shift'],
                            layer_shift=c['layer_shift'], psf_index=c['index'], return_residual=True, **kw)


def _cubefree(ctx, c, with_var=True, **kw):
    return ctx.fit_cube_psf_free(c['cube'], c['psf'], c['origin'], var=c['var'] if with_var else None, shift=c['shift'],
                                 layer_shift=c['layer_shift'], psf_index=c['index'], return_residual=True, **kw)


def run(ctx, name):
    """The outputs of the case `name` on the context `ctx`, host form: {'<case>.<output>': array}; OUTPUTS names them in
    the order the call returns them"""
    key, kw = cases()[name]
    call = name.split('.')[0]
    arrays = {'frame': _frame, 'free': _free, 'cube': _cube, 'cubefree': _cubefree}[call](ctx, scene(key), **kw)
    assert len(arrays) == len(OUTPUTS[call])
    return {'%s.%s' % (name, o): a for o, a in zip(OUTPUTS[call], arrays)}


def record(ctx):
    """The outputs of every case of the record"""
    out = {}
    for name in cases():
        out.update(run(ctx, name))
    return out


DEVICE_CASES = ('frame.1089_back', 'free.var.back', 'cube.back.batch0', 'cubefree.var.back')


def run_device(ctx, name):
    """A case of DEVICE_CASES through device pointers: the names and arrays run() gives."""
    import torch
    dev = torch.device('cuda:0')
    key, kw = cases()[name]
    kw = {k: v for k, v in kw.items() if k != 'with_var'}     # (the device cases take the variance)
    s = scene(key)
    call = name.split('.')[0]
    layered = 'cube' in s
    t = {k: torch.from_numpy(np.ascontiguousarray(s[k])).to(dev) for k in (CUBE_INPUTS if layered else FRAME_INPUTS)}
    data = t['cube' if layered else 'image']
    n, npsf = len(s['origin']), len(s['psf'])
    lead = tuple(data.shape[:-2])                             # (nl,) of a cube, () of a frame
    ny, nx = data.shape[-2:]

    def new(*shape):
        return torch.full(shape, -1.0, dtype=torch.float64, device=dev)

    shapes = {'frame': dict(rows=(n, 8), head=(8,)), 'free': dict(rows=(n, 16), shifts=(n, 2), head=(12,)),
              'cube': dict(rows=lead + (n, 8), head=lead + (8,)),
              'cubefree': dict(rows=lead + (n, 8), pos=(n, 8), shifts=(n, 2), head=lead + (8,), call=(8,))}[call]
    o = {k: new(*shape) for k, shape in shapes.items()}
    o['resid'] = new(*data.shape)
    p = {k: v.data_ptr() for k, v in o.items()}
    common = dict(var_ptr=t['var'].data_ptr(), shift_ptr=t['shift'].data_ptr(), psf_index_ptr=t['index'].data_ptr(),
                  resid_ptr=p['resid'], **kw)
    if layered:
        common['layer_shift_ptr'] = t['layer_shift'].data_ptr()
    torch.cuda.synchronize()
    if call == 'frame':
        ctx.fit_frame_psf_device(ny, nx, data.data_ptr(), n, npsf, t['psf'].data_ptr(), t['origin'].data_ptr(),
                                 p['rows'], p['head'], **common)
    elif call == 'free':
        ctx.fit_frame_psf_free_device(ny, nx, data.data_ptr(), n, npsf, t['psf'].data_ptr(), t['origin'].data_ptr(),
                                      p['rows'], p['shifts'], p['head'], **common)
    elif call == 'cube':
        ctx.fit_cube_psf_device(lead[0], ny, nx, data.data_ptr(), n, npsf, t['psf'].data_ptr(), t['origin'].data_ptr(),
                                p['rows'], p['head'], **common)
    else:
        ctx.fit_cube_psf_free_device(lead[0], ny, nx, data.data_ptr(), n, npsf, t['psf'].data_ptr(),
                                     t['origin'].data_ptr(), p['rows'], p['head'], p['pos'], p['shifts'], p['call'],
                                     **common)
    ctx.sync()
    return {'%s.%s' % (name, k): o[k].cpu().numpy() for k in OUTPUTS[call]}


def record_device(ctx):
    out = {}
    for name in DEVICE_CASES:
        out.update(run_device(ctx, name))
    return out
