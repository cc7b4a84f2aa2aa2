"""Rate of the crowded-field fit (mpsfr_fit_frame_psf with on_device = 1): a 2048 x 2048 frame with 17 000 stars of four
model stamps at uniform positions, fluxes 200 - 5000 on a sky of 7, var = 4 + model / 2 with Gaussian noise of that
variance, radius 8, background on, from a zero start.

The frame is rendered by the library itself.  Timed, each by itself, in 5 regions of K calls with device events on the
context stream, the median region:
  solve       the call to tol = 1e-10 with room to get there: max_iter = 1000 (the steps queued behind the stop are
              no-ops)
  solve_100   the same at the default max_iter = 100
  iter_lo/hi  the call at max_iter = 10 and 30 with a tolerance no step can meet: (hi - lo) / 20 is one iteration
              -- one tile walk of the renderer, one projection, one frame reduction, one step kernel
  render      one mpsfr_render_stars over the same stars, in the same run
beside the iteration count, the pixels of the fit and the floor of the projection: 23 fp64 FMAs (a 16-tap FIR, its 4 row
weights, the weight and the two products) on each of the 3600 footprint pixels of every accepted star at the card's
nominal vector fp64 rate (78.6 TFLOP/s: 39.3e12 FMA/s).  The script states numbers and is not a pass criterion.

    python scripts/frame_fit_rate.py [K] [NSTAR] [OUT.json] [SIDE]
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

FMA_PER_S = 78.6e12 / 2
FMA_PER_PIXEL = 23.0
FOOTPRINT = 3600.0


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 17000
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    side = int(sys.argv[4]) if len(sys.argv) > 4 else 2048
    t0 = time.time()
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(17)
    psf = Y.models()
    pos = rng.uniform(0, side, (ns, 2))
    origin = (np.rint(pos) - 20).astype(np.int32)
    shift, flux = pos - np.rint(pos), rng.uniform(200, 5000, ns)
    index = (np.arange(ns) % 4).astype(np.int32)
    tps, tor, tsh, tfl, tix = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (psf, origin, shift, flux, index))
    model = torch.zeros((side, side), dtype=torch.float64, device=dev)
    ctx = Context(dim=128, pixscale=grid_pixscale(128), precision='mixed')
    cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
    torch.cuda.synchronize()
    ctx.render_stars_device(side, side, ns, 4, tps.data_ptr(), tor.data_ptr(), tfl.data_ptr(), model.data_ptr(),
                            shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr())
    ctx.sync()
    var = 4.0 + model / 2.0
    noise = torch.from_numpy(rng.normal(size=(side, side))).to(dev)
    frame = model + 7.0 + noise * torch.sqrt(var)
    other = torch.empty_like(frame)
    rows = torch.empty((ns, NFRAMEFIT), dtype=torch.float64, device=dev)
    head = torch.empty(NFRAMEFIT, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def fit(max_iter, tol):
        def call():
            ctx.fit_frame_psf_device(side, side, frame.data_ptr(), ns, 4, tps.data_ptr(), tor.data_ptr(), rows.data_ptr(),
                                     head.data_ptr(), var_ptr=var.data_ptr(), shift_ptr=tsh.data_ptr(),
                                     psf_index_ptr=tix.data_ptr(), radius=8.0, background=True, max_iter=max_iter,
                                     tol=tol)
        return call

    def render():
        ctx.render_stars_device(side, side, ns, 4, tps.data_ptr(), tor.data_ptr(), tfl.data_ptr(), other.data_ptr(),
                                image_ptr=frame.data_ptr(), shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr(),
                                subtract=True)

    work = [('solve', fit(1000, 1e-10)), ('solve_100', fit(100, 1e-10)), ('iter_lo', fit(10, 1e-300)),
            ('iter_hi', fit(30, 1e-300)), ('render', render)]
    heads = {}
    for label, call in work:                              # warm up; what the solve reports
        call()
        ctx.sync()
        heads[label] = head.cpu().numpy().copy()
        if label == 'solve':
            z = rows.cpu().numpy()[:, 0] - flux
            err = rows.cpu().numpy()[:, 1]
            overlap = rows.cpu().numpy()[:, 4]
    h, h100 = heads['solve'], heads['solve_100']
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
    per_iter = (med['iter_hi'] - med['iter_lo']) / 20.0
    nacc = float(h[6])
    out = dict(side=side, stars=ns, radius=8.0, background=True, calls_per_region=K, regions=5,
               conditions='one MI355X, one process, mixed-precision context (the fit is fp64 in both modes); every array '
                          'device resident; 5 regions of K calls each, median region; device events on the context '
                          'stream; the solve is tol 1e-10 with 1000 steps queued (solve_100: 100), an iteration is the difference of the '
                          'calls at 30 and 10 forced steps over 20; the render is one mpsfr_render_stars over the same '
                          'stars in the same run; fma_floor_ms is %g FMAs on 3600 footprint pixels of every accepted '
                          'star at 39.3e12 FMA/s' % FMA_PER_PIXEL,
               solve_ms=med['solve'], solve_min=min(times['solve']), solve_max=max(times['solve']),
               iterations=int(h[4]), head_status=int(h[7]), relative_residual=float(h[5]), accepted=int(nacc),
               solve_100_ms=med['solve_100'], solve_100_iterations=int(h100[4]), solve_100_status=int(h100[7]),
               solve_100_relative_residual=float(h100[5]),
               pixels_fitted=int(h[3]), fitted_background=float(h[0]), chi2_per_pixel=float(h[2] / h[3]),
               iter_lo_ms=med['iter_lo'], iter_hi_ms=med['iter_hi'], ms_per_iteration=per_iter,
               render_ms=med['render'], render_min=min(times['render']), render_max=max(times['render']),
               iteration_over_render=per_iter / med['render'],
               projection_fma_floor_ms=FMA_PER_PIXEL * FOOTPRINT * nacc / FMA_PER_S * 1e3,
               worst_flux_error=float(np.abs(z).max()), median_flux_error=float(np.median(np.abs(z))),
               median_conditional_error=float(np.median(err)), largest_overlap=float(overlap.max()),
               stars_with_overlap_above_2=int(np.sum(overlap > 2.0)), wall_s=time.time() - t0)
    for k in ('solve_ms', 'iterations', 'solve_100_ms', 'solve_100_iterations', 'ms_per_iteration', 'render_ms', 'iteration_over_render',
              'projection_fma_floor_ms', 'accepted', 'pixels_fitted', 'head_status'):
        print('%-26s %s' % (k, out[k]), flush=True)
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
