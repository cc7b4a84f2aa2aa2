"""The calls of the bit-identity record of the frame layer (tests/golden/frame_calls_gfx950.npz), shared by
scripts/record_frame_calls.py, which writes the record, and tests/test_gpu_frame_bits.py, which holds a build to it.

The inputs are the seeded scenes of the parity tests, nothing new:

  render  render_ref.scene() -- its pile of 300 stars makes one tile list longer than RENDER_SORT_CHUNK, so both sort
          paths of k_render_tiles run -- added to the image, added to zeros and subtracted from the image (subtract
          without an image is refused by the call); and the five stars of test_parity_on_degenerate_frames on 1 x 1,
          1 x 200 and 200 x 1, added and subtracted.  Outputs: the frame and the star rows.
  fit     frame_fit_ref.scene() on its 97 x 150 frame at radius 8 for (var, background) in all four combinations.
          Outputs: the star rows, the head, the residual frame.
  find    find_ref.scene() with and without var at half 2 and 3 (sep 3, the thresholds of the parity test).  Outputs:
          rows, origins, count, map.
  group   every scene of group_ref.scenes().  Outputs: labels, group rows, origins, shifts, counts.

A frame of more than HASH_ABOVE values (the 97 x 150 frames are noise: deflate leaves them at 114 KB each) is kept as
the SHA-256 of its little-endian bytes, a uint8 array of 32; every other array in full.  Values are compared by their
bytes (bits below), so that a NaN equals itself and -0 differs from +0.
"""
import hashlib
import os

import numpy as np

import find_ref
import frame_fit_ref
import group_ref
import render_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
RECORD = os.path.join(GOLDEN, 'frame_calls_gfx950.npz')
MODES = ('mixed', 'f64')
DIM = 128                                      # of the contexts: the frame calls do not depend on it
HASH_ABOVE = 4096
CALLS = ('render', 'fit', 'find', 'group')
RADIUS = 8.0
FIND_SEP, FIND_MAX = 3, 256
DEGENERATE = ((1, 1), (1, 200), (200, 1))


def degenerate(shape):
    """The stars and the image of tests/test_gpu_render.py::test_parity_on_degenerate_frames on `shape`."""
    rng = np.random.default_rng(shape[1])
    origin = np.array([[-20, -20], [-45, shape[1] - 30], [shape[0] - 5, -49], [-3, shape[1] // 2 - 20], [-60, 0]],
                      dtype=np.int32)
    shift, scale, index = rng.uniform(-8, 8, (5, 2)), rng.uniform(-50, 50, 5), np.array([3, 2, 1, 0, 2], dtype=np.int32)
    return dict(psf=render_ref.models(), origin=origin, shift=shift, scale=scale, index=index,
                image=rng.normal(size=shape), n=5)


def render_cases():
    """name -> (scene, image or None, subtract)"""
    s = render_ref.scene()
    cases = {'render.scene.add': (s, s['image'], False), 'render.scene.zeros': (s, None, False),
             'render.scene.sub': (s, s['image'], True)}
    for shape in DEGENERATE:
        d = degenerate(shape)
        for sub in (False, True):
            cases['render.%dx%d.%s' % (shape + ('sub' if sub else 'add',))] = (d, d['image'], sub)
    return cases


def fit_cases():
    """name -> (with_var, background)"""
    return {'fit.%s.%s' % ('var' if v else 'unit', 'back' if b else 'noback'): (v, b)
            for v in (True, False) for b in (True, False)}


def find_cases():
    """name -> (usevar, half)"""
    return {'find.%s.half%d' % ('var' if v else 'unit', h): (v, h) for v in (True, False) for h in (2, 3)}


def group_cases():
    return {'group.%s' % name: scene for name, scene in group_ref.scenes().items()}


def inputs():
    """Every input array of the record's calls, by name, in a fixed order."""
    out = []
    for name, (s, image, sub) in render_cases().items():
        out += [(name + '.' + k, s[k]) for k in ('psf', 'origin', 'shift', 'scale', 'index', 'image')]
    s = frame_fit_ref.scene()
    out += [('fit.' + k, s[k]) for k in ('image', 'var', 'psf', 'index', 'origin', 'shift')]
    s = find_ref.scene()
    out += [('find.' + k, s[k]) for k in ('image', 'var', 'psf')]
    for name, (pos, crit, shape) in group_cases().items():
        out += [(name + '.pos', pos), (name + '.crit_shape', np.array((crit,) + tuple(shape), dtype=np.float64))]
    return out


def le(a):
    a = np.ascontiguousarray(a)
    return np.ascontiguousarray(a, dtype=a.dtype.newbyteorder('<'))


def digest(arrays):
    h = hashlib.sha256()
    for name, a in arrays:
        h.update(name.encode())
        h.update(le(a).tobytes())
    return h.hexdigest()


def bits(a):
    """the bytes of `a` as a uint8 array with one more axis: what np.array_equal compares"""
    a = le(a)
    return a.reshape(-1).view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))


FRAMES = ('frame', 'resid', 'map')             # the outputs that are whole frames


def stored(name, a):
    """The output `name` as the record keeps it: in full, or the SHA-256 of its bytes for a frame above HASH_ABOVE
    values"""
    a = le(a)
    if name.rsplit('.', 1)[-1] in FRAMES and a.size > HASH_ABOVE:
        return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()
    return a


def same(name, got, kept):
    """does the output `got` equal the record's entry `kept` for `name`, bit for bit?"""
    want = stored(name, got)
    return want.dtype == kept.dtype and want.shape == kept.shape and bool(np.array_equal(bits(want), bits(kept)))


def context(api, prec):
    return api.Context(dim=DIM, pixscale=api.grid_pixscale(DIM), precision=prec)


def _render(ctx, s, image, sub):
    shape = None if image is not None else render_ref.FRAME
    return ctx.render_stars(s['psf'], s['origin'], s['scale'], shift=s['shift'], psf_index=s['index'], image=image,
                            shape=shape, subtract=sub, return_status=True)


def _fit(ctx, with_var, background):
    s = frame_fit_ref.scene()
    return ctx.fit_frame_psf(s['image'], s['psf'], s['origin'], var=s['var'] if with_var else None, shift=s['shift'],
                             psf_index=s['index'], radius=RADIUS, background=background, return_residual=True)


def _find(ctx, usevar, half):
    s = find_ref.scene()
    rows, origin, count, tmap = ctx.find_stars(s['image'], s['psf'], var=s['var'] if usevar else None, half=half,
                                               sep=FIND_SEP, threshold=find_ref.THRESHOLD[usevar], max_stars=FIND_MAX,
                                               return_map=True)
    assert 0 < count < FIND_MAX
    return rows, origin, np.array([count], dtype=np.int32), tmap


def record(ctx):
    """The outputs of every call of the record on the context `ctx`, host form: {'<case>.<output>': array}"""
    out = {}
    for name, (s, image, sub) in render_cases().items():
        out[name + '.frame'], out[name + '.rows'] = _render(ctx, s, image, sub)
    for name, (v, b) in fit_cases().items():
        out[name + '.rows'], out[name + '.head'], out[name + '.resid'] = _fit(ctx, v, b)
    for name, (v, h) in find_cases().items():
        out[name + '.rows'], out[name + '.origin'], out[name + '.count'], out[name + '.map'] = _find(ctx, v, h)
    for name, (pos, crit, shape) in group_cases().items():
        for k, a in zip(('label', 'groups', 'origin', 'shift', 'counts'), ctx.group_stars(pos, crit, shape)):
            out['%s.%s' % (name, k)] = a
    return out


DEVICE_CASES = ('render.scene.sub', 'fit.var.back', 'find.var.half3', 'group.field')


def record_device(ctx):
    """One case per call through device pointers: the same names and arrays as record() gives for DEVICE_CASES."""
    import torch
    dev = torch.device('cuda:0')

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def new(shape, dtype=torch.float64):
        return torch.full(shape, -1, dtype=dtype, device=dev)

    out = {}
    # render
    name = DEVICE_CASES[0]
    s, image, sub = render_cases()[name]
    ny, nx = image.shape
    t = {k: up(s[k]) for k in ('psf', 'origin', 'shift', 'scale', 'index')}
    tim, tout, trow = up(image), new((ny, nx)), new((s['n'], 4))
    torch.cuda.synchronize()
    ctx.render_stars_device(ny, nx, s['n'], len(s['psf']), t['psf'].data_ptr(), t['origin'].data_ptr(),
                            t['scale'].data_ptr(), tout.data_ptr(), image_ptr=tim.data_ptr(),
                            shift_ptr=t['shift'].data_ptr(), psf_index_ptr=t['index'].data_ptr(),
                            star_out_ptr=trow.data_ptr(), subtract=sub)
    ctx.sync()
    out[name + '.frame'], out[name + '.rows'] = tout.cpu().numpy(), trow.cpu().numpy()
    # fit
    name = DEVICE_CASES[1]
    s = frame_fit_ref.scene()
    ny, nx = s['image'].shape
    t = {k: up(s[k]) for k in ('image', 'var', 'psf', 'index', 'origin', 'shift')}
    trow, thead, tres = new((s['n'], 8)), new((8,)), new((ny, nx))
    torch.cuda.synchronize()
    ctx.fit_frame_psf_device(ny, nx, t['image'].data_ptr(), s['n'], len(s['psf']), t['psf'].data_ptr(),
                             t['origin'].data_ptr(), trow.data_ptr(), thead.data_ptr(), var_ptr=t['var'].data_ptr(),
                             shift_ptr=t['shift'].data_ptr(), psf_index_ptr=t['index'].data_ptr(),
                             resid_ptr=tres.data_ptr(), radius=RADIUS, background=True)
    ctx.sync()
    out[name + '.rows'], out[name + '.head'], out[name + '.resid'] = (a.cpu().numpy() for a in (trow, thead, tres))
    # find
    name = DEVICE_CASES[2]
    s = find_ref.scene()
    ny, nx = s['image'].shape
    t = {k: up(s[k]) for k in ('image', 'var', 'psf')}
    trow, tor, tct, tmap = new((FIND_MAX, 8)), new((FIND_MAX, 2), torch.int32), new((1,), torch.int32), new((ny, nx))
    torch.cuda.synchronize()
    ctx.find_stars_device(ny, nx, t['image'].data_ptr(), t['psf'].data_ptr(), 3, FIND_SEP, find_ref.THRESHOLD[True],
                          FIND_MAX, trow.data_ptr(), tct.data_ptr(), var_ptr=t['var'].data_ptr(),
                          origin_ptr=tor.data_ptr(), map_ptr=tmap.data_ptr())
    ctx.sync()
    n = int(tct.cpu().numpy()[0])
    out[name + '.rows'], out[name + '.origin'] = trow.cpu().numpy()[:n], tor.cpu().numpy()[:n]
    out[name + '.count'], out[name + '.map'] = tct.cpu().numpy(), tmap.cpu().numpy()
    # group
    name = DEVICE_CASES[3]
    pos, crit, shape = group_cases()[name]
    nstar = len(pos)
    tpos = up(pos)
    tlab, tgrp, tor = new((nstar,), torch.int32), new((nstar, 8), torch.int32), new((nstar, 2), torch.int32)
    tsh, tct = new((nstar, group_ref.MAX_GROUP, 2)), new((6,), torch.int32)
    torch.cuda.synchronize()
    ctx.group_stars_device(shape[0], shape[1], nstar, tpos.data_ptr(), 2, crit, nstar, tlab.data_ptr(), tgrp.data_ptr(),
                           tct.data_ptr(), origin_ptr=tor.data_ptr(), shift_ptr=tsh.data_ptr())
    ctx.sync()
    counts = tct.cpu().numpy()
    n = int(counts[0])
    from muse_psfr_amd._lib import group_shift_rows
    out[name + '.label'], out[name + '.groups'] = tlab.cpu().numpy(), tgrp.cpu().numpy()[:n]
    out[name + '.origin'], out[name + '.shift'] = tor.cpu().numpy()[:n], group_shift_rows(tsh.cpu().numpy(), counts)[:n]
    out[name + '.counts'] = counts
    return out
