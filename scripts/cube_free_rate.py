"""Rate of the crowded-field fit of a cube with free positions (mpsfr_fit_cube_psf_free with on_device = 1) on the scene
of scripts/cube_fit_rate.py and by the method of scripts/frame_free_rate.py: a 320 x 320 frame, 2 000 stars of four
model stamps at uniform random positions, 64 layers whose fluxes differ (uniform in 200 - 5000 times a factor that runs
from 0.25 to 4 over the cube) on a sky of 7, var = 4 + model / 2 with Gaussian noise of that variance, radius 8,
background on, the layers rendered by the library itself.  The starts are the true positions displaced by a Gaussian of
0.1 px per axis.  One process and one context, every array device resident, device events on the context stream, 5
rounds, the variants alternating within a round; medians with their minimum and maximum.

  call         the whole call at its defaults (max_outer 8, pos_tol 1e-3, max_iter 100, tol 1e-10) from a zero start
  T(o, m)      a forced call at max_outer = o and max_iter = m with tolerances no step can meet (tol 1e-300, pos_tol
               1e-300, min_snr 0): every solve runs its m iterations, every outer step runs
  cube3        (a) one joint three-column iteration per layer -- the layered three-column walk and projection, the frame
               reduction and the joint step kernel --: ((T(2, 30) - T(1, 30)) - (T(2, 10) - T(1, 10))) / 20 / nl
  frames3      (c) the same difference through nl device-form mpsfr_fit_frame_psf_free calls, one per layer (a position
               per layer: the loop a user writes without (a)), per layer
  flux1        one flux-only layer-iteration of mpsfr_fit_cube_psf at layer_batch = 0: (T(30) - T(10)) / 20 / nl
The requirement of DESIGN.md section 27 is cube3 <= frames3 with (a)'s range below (c)'s; `verdict` says whether it
holds.  The script states numbers and is not a pass criterion.

    python scripts/cube_free_rate.py [K] [OUT.json] [NL] [NSTAR] [SIDE]
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
from muse_psfr_amd import (NCUBEFREE_CALL, NCUBEFREE_POS, NFRAMEFIT, NFRAMEFREE, NFRAMEFREE_HEAD, Context,  # noqa: E402
                           grid_pixscale)
import render_ref as Y  # noqa: E402


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 1
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
    start = shift + np.random.default_rng(18).normal(scale=0.1, size=shift.shape)

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tps, tcp, tor, tsh, tfl, tix, tst = (to_dev(a) for a in (psf, cube_psf, origin, shift, flux, index, start))
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

    def buf(*shape):
        return torch.empty(shape, dtype=torch.float64, device=dev)
    rows, head, prow, shifts, call_out = buf(nl, ns, NFRAMEFIT), buf(nl, NFRAMEFIT), buf(ns, NCUBEFREE_POS), buf(ns, 2), \
        buf(NCUBEFREE_CALL)
    frows, fshifts, fhead = buf(nl, ns, NFRAMEFREE), buf(nl, ns, 2), buf(nl, NFRAMEFREE_HEAD)
    torch.cuda.synchronize()

    def free(**kw):
        def call():
            ctx.fit_cube_psf_free_device(nl, side, side, cube.data_ptr(), ns, 4, tcp.data_ptr(), tor.data_ptr(),
                                         rows.data_ptr(), head.data_ptr(), prow.data_ptr(), shifts.data_ptr(),
                                         call_out.data_ptr(), var_ptr=var.data_ptr(), shift_ptr=tst.data_ptr(),
                                         psf_index_ptr=tix.data_ptr(), radius=8.0, background=True, **kw)
        return call

    def frames(**kw):
        def call():
            for l in range(nl):
                ctx.fit_frame_psf_free_device(side, side, cube[l].data_ptr(), ns, 4, tps.data_ptr(), tor.data_ptr(),
                                              frows[l].data_ptr(), fshifts[l].data_ptr(), fhead[l].data_ptr(),
                                              var_ptr=var[l].data_ptr(), shift_ptr=tst.data_ptr(),
                                              psf_index_ptr=tix.data_ptr(), radius=8.0, background=True, **kw)
        return call

    def flux_only(it):
        def call():
            ctx.fit_cube_psf_device(nl, side, side, cube.data_ptr(), ns, 4, tcp.data_ptr(), tor.data_ptr(),
                                    rows.data_ptr(), head.data_ptr(), var_ptr=var.data_ptr(), shift_ptr=tst.data_ptr(),
                                    psf_index_ptr=tix.data_ptr(), radius=8.0, background=True, max_iter=it, tol=1e-300)
        return call

    def forced(outer, it):
        return dict(max_outer=outer, max_iter=it, tol=1e-300, pos_tol=1e-300, min_snr=0.0)
    grid = [(o, m) for o in (1, 2) for m in (10, 30)]
    work = [('call', free())] + [('cube_%d_%d' % g, free(**forced(*g))) for g in grid] + \
        [('frames_%d_%d' % g, frames(**forced(*g))) for g in grid] + [('flux_10', flux_only(10)), ('flux_30', flux_only(30))]
    calls = {}
    for label, call in work:                              # warm up; what the calls report
        call()
        ctx.sync()
        if label == 'call' or label.startswith('cube'):
            calls[label] = call_out.cpu().numpy().copy()
        if label == 'call':
            got, pos_rows = shifts.cpu().numpy().copy(), prow.cpu().numpy().copy()
            overlap = rows.cpu().numpy()[:, :, 4].max(axis=0)
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
    t = {k: np.array(v) for k, v in times.items()}

    def second(name):                                     # per round: one three-column iteration of one layer
        return ((t[name + '_2_30'] - t[name + '_1_30']) - (t[name + '_2_10'] - t[name + '_1_10'])) / 20.0 / nl

    def stats(v):
        return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    cube3, frames3, flux1 = second('cube'), second('frames'), (t['flux_30'] - t['flux_10']) / 20.0 / nl
    c = calls['call']
    moved = pos_rows[:, 7] > 0
    quiet = moved & (overlap < 0.5)                       # (uniform positions put some stars on top of each other)
    out = dict(side=side, stars=ns, layers=nl, radius=8.0, background=True, calls_per_region=K, rounds=5,
               start_sigma_px=0.1,
               conditions='one MI355X, one process, mixed-precision context (the fit is fp64 in both modes); every array '
                          'device resident; 5 rounds, the variants alternating within a round, device events on the '
                          'context stream; forced calls at tol = pos_tol = 1e-300 and min_snr = 0 run every queued '
                          'iteration; an iteration is the second difference of forced calls between max_outer 2 and 1 '
                          'and max_iter 30 and 10, per round',
               call_ms=stats(t['call']), outer_steps=int(c[2]), inner_iterations=int(c[5]), call_status=int(c[6]),
               last_step_px=float(c[3]), free_in_last_step=int(c[4]), chi2_per_dof=float(c[0] / c[1]),
               forced_free_stars={k: int(v[4]) for k, v in calls.items() if k != 'call'},
               forced_ms={k: stats(v) for k, v in t.items() if k != 'call'},
               us_per_layer_iteration_cube_three_columns=stats(1e3 * cube3),
               us_per_layer_iteration_frames_three_columns=stats(1e3 * frames3),
               us_per_layer_iteration_flux_only=stats(1e3 * flux1),
               frames_over_cube=float(np.median(frames3) / np.median(cube3)),
               three_over_flux_only=float(np.median(cube3) / np.median(flux1)),
               verdict='the range of (a) lies below the range of (c)' if cube3.max() < frames3.min()
               else 'the ranges of (a) and (c) overlap' if np.median(cube3) <= np.median(frames3)
               else '(a) is above (c)',
               rms_start_error_px=float(np.sqrt(np.mean((start - shift)[moved] ** 2))),
               rms_final_error_px=float(np.sqrt(np.mean((got - shift)[moved] ** 2))),
               median_start_error_px=float(np.median(np.abs(start - shift)[quiet])),
               median_final_error_px=float(np.median(np.abs(got - shift)[quiet])),
               stars_with_overlap_below_half=int(quiet.sum()), stars_moved=int(moved.sum()), wall_s=time.time() - t0)
    for k in ('call_ms', 'outer_steps', 'inner_iterations', 'call_status', 'us_per_layer_iteration_cube_three_columns',
              'us_per_layer_iteration_frames_three_columns', 'us_per_layer_iteration_flux_only', 'frames_over_cube',
              'three_over_flux_only', 'verdict', 'rms_start_error_px', 'rms_final_error_px', 'median_start_error_px',
              'median_final_error_px', 'stars_with_overlap_below_half', 'stars_moved', 'wall_s'):
        print('%-44s %s' % (k, out[k]), flush=True)
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
