"""Rate of the crowded-field fit of cubes (mpsfr_fit_cube_psf with on_device = 1) against the loop it replaces.

The scene is MUSE-like: a 320 x 320 frame, 2 000 stars of four model stamps at uniform random positions, fluxes
200 - 5000 on a sky of 7, var = 4 + model / 2 with Gaussian noise of that variance (the numbers of
scripts/frame_fit_rate.py), in 64 layers whose fluxes differ (every layer draws its own, times a factor that runs from
0.25 to 4 over the cube).  Radius 8, background on, tol 1e-10, max_iter 100, from a zero start, no residual cube.  The
layers are rendered by the library itself.

Measured in one process and one context, every array device resident, with device events on the context stream, in 5
regions per variant, the variants alternating within a round; the median region with its minimum and maximum:
  cube        (a) one mpsfr_fit_cube_psf call at layer_batch = 0 (the batch the library's budget of work memory gives)
  cube_b1     (b) the same at layer_batch = 1
  frames      (c) 64 device-form mpsfr_fit_frame_psf calls, one per layer: the loop a user writes without (a)
beside the iteration count of every layer, the time per layer-iteration of (a), and whether (a) and (c) return the
same bits.  The yardstick is (c); `verdict` says whether (a)'s range lies below (c)'s.  The script states numbers and is
not a pass criterion.

    python scripts/cube_fit_rate.py [K] [OUT.json] [NL] [NSTAR] [SIDE]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from muse_psfr_amd import NFRAMEFIT, Context, grid_pixscale  # noqa: E402
import render_ref as Y  # noqa: E402

WORK_BYTES = 256 << 20            # MPSFR_CUBE_FIT_WORK_BYTES


def budget_batch(nl, ny, nx, ns):
    """The batch layer_batch = 0 stands for: the header's per-layer work memory into its budget."""
    npix = ny * nx
    per = 8 * (2 * npix + 7 * ns + 4 * ((npix + 4095) // 4096) + 9) + 4 * (2 * ns + 5)
    return max(1, min(nl, WORK_BYTES // per))


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    nl = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    ns = int(sys.argv[4]) if len(sys.argv) > 4 else 2000
    side = int(sys.argv[5]) if len(sys.argv) > 5 else 320
    t0 = time.time()
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(25)
    psf = Y.models()
    pos = rng.uniform(0, side, (ns, 2))
    origin = (np.rint(pos) - 20).astype(np.int32)
    shift = pos - np.rint(pos)
    index = (np.arange(ns) % 4).astype(np.int32)
    factor = 4.0 ** np.linspace(-1.0, 1.0, nl)
    flux = rng.uniform(200, 5000, (nl, ns)) * factor[:, None]
    cube_psf = np.ascontiguousarray(np.broadcast_to(psf[:, None], (4, nl, 40, 40)))

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tps, tcp, tor, tsh, tfl, tix = (to_dev(a) for a in (psf, cube_psf, origin, shift, flux, index))
    model = torch.zeros((nl, side, side), dtype=torch.float64, device=dev)
    ctx = Context(dim=128, pixscale=grid_pixscale(128), precision='mixed')
    cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
    torch.cuda.synchronize()
    for l in range(nl):
        ctx.render_stars_device(side, side, ns, 4, tps.data_ptr(), tor.data_ptr(), tfl[l].data_ptr(),
                                model[l].data_ptr(), shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr())
    ctx.sync()
    var = 4.0 + model / 2.0
    cube = model + 7.0 + to_dev(rng.normal(size=(nl, side, side))) * torch.sqrt(var)
    rows = torch.empty((nl, ns, NFRAMEFIT), dtype=torch.float64, device=dev)
    head = torch.empty((nl, NFRAMEFIT), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    par = dict(radius=8.0, background=True, max_iter=100, tol=1e-10)

    def cube_call(batch):
        def call():
            ctx.fit_cube_psf_device(nl, side, side, cube.data_ptr(), ns, 4, tcp.data_ptr(), tor.data_ptr(),
                                    rows.data_ptr(), head.data_ptr(), var_ptr=var.data_ptr(), shift_ptr=tsh.data_ptr(),
                                    psf_index_ptr=tix.data_ptr(), layer_batch=batch, **par)
        return call

    def frames():
        for l in range(nl):
            ctx.fit_frame_psf_device(side, side, cube[l].data_ptr(), ns, 4, tps.data_ptr(), tor.data_ptr(),
                                     rows[l].data_ptr(), head[l].data_ptr(), var_ptr=var[l].data_ptr(),
                                     shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr(), **par)

    work = [('cube', cube_call(0)), ('cube_b1', cube_call(1)), ('frames', frames)]
    got = {}
    for label, call in work:                              # warm up; what each variant returns
        rows.fill_(-1.0)
        head.fill_(-1.0)
        torch.cuda.synchronize()
        call()
        ctx.sync()
        got[label] = (rows.cpu().numpy().copy(), head.cpu().numpy().copy())

    def same(a, b):
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    same_bits = all(same(got[k][i], got['frames'][i]) for k in ('cube', 'cube_b1') for i in (0, 1))
    h = got['cube'][1]
    times = {w[0]: [] for w in work}
    for _ in range(5):
        for label, call in work:
            ctx.sync()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(cs)
            for _ in range(K):
                call()
            b.record(cs)
            b.synchronize()
            times[label].append(a.elapsed_time(b) / K)
    ctx.sync()
    ctx.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    lo = {k: float(min(v)) for k, v in times.items()}
    hi = {k: float(max(v)) for k, v in times.items()}
    iters = h[:, 4].astype(int)
    if hi['cube'] < lo['frames']:
        verdict = 'the cube call is faster: its range lies below that of the frame calls'
    elif lo['cube'] > hi['frames']:
        verdict = 'the cube call is SLOWER: its range lies above that of the frame calls'
    else:
        verdict = 'the ranges overlap: no difference shown'
    out = dict(side=side, stars=ns, layers=nl, radius=8.0, background=True, max_iter=100, tol=1e-10,
               calls_per_region=K, regions=5,
               conditions='one MI355X, one process, one mixed-precision context (the fit is fp64 in both modes); every '
                          'array device resident; 5 regions of K calls per variant, the variants alternating, device '
                          'events on the context stream; median region with its minimum and maximum; no residual cube',
               budget_batch=budget_batch(nl, side, side, ns),
               cube_ms=med['cube'], cube_min=lo['cube'], cube_max=hi['cube'],
               cube_b1_ms=med['cube_b1'], cube_b1_min=lo['cube_b1'], cube_b1_max=hi['cube_b1'],
               frames_ms=med['frames'], frames_min=lo['frames'], frames_max=hi['frames'],
               frames_over_cube=med['frames'] / med['cube'], cube_b1_over_cube=med['cube_b1'] / med['cube'],
               verdict=verdict, same_bits_as_frames=same_bits,
               iterations=iters.tolist(), iterations_total=int(iters.sum()), iterations_min=int(iters.min()),
               iterations_max=int(iters.max()), head_status=sorted(set(h[:, 7].astype(int).tolist())),
               accepted_min=int(h[:, 6].min()), pixels_fitted_min=int(h[:, 3].min()),
               us_per_layer_iteration=1e3 * med['cube'] / float(iters.sum()),
               us_per_layer_iteration_frames=1e3 * med['frames'] / float(iters.sum()),
               ms_per_layer=med['cube'] / nl, ms_per_layer_frames=med['frames'] / nl, wall_s=time.time() - t0)
    for k in ('budget_batch', 'cube_ms', 'cube_min', 'cube_max', 'cube_b1_ms', 'frames_ms', 'frames_min', 'frames_max',
              'frames_over_cube', 'verdict', 'same_bits_as_frames', 'iterations_min', 'iterations_max',
              'us_per_layer_iteration', 'head_status'):
        print('%-30s %s' % (k, out[k]), flush=True)
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
