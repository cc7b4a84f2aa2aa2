"""Rates of the frame level of the PSF photometry (mpsfr_cut_stamps, mpsfr_fit_stamps_psf, mpsfr_render_stars, all with
on_device = 1) on two scenes of 20 000 stars: a 2048 x 2048 frame at a uniform density and a crowded 512 x 512 one.

The frame is rendered by the library itself from four Moffat model stamps shared through psf_index (sub-pixel shifts,
fluxes 100 - 1000), the stamps are cut at the rounded positions, fitted (background, free shift) and the fitted models
subtracted.  Each of the three calls is timed by itself: 5 regions of K calls, device events on the context stream,
the median region.  Reported per call: ms, stars/s and frame GB/s (the frame read and written once: 16 bytes per
pixel, over the time of the call) -- beside the time of a plain device copy of the frame measured in the same run and
the same traffic at the nominal 8 TB/s of HBM: the floor of anything that reads and writes the frame.  The script
states numbers and is not a pass criterion; it stops timing once `budget` seconds of wall time are spent.

    python scripts/render_rate.py [K] [NSTAR] [OUT.json] [BUDGET_S]
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
from muse_psfr_amd import NFIT_PSF, Context, grid_pixscale  # noqa: E402
import render_ref as Y  # noqa: E402

SCENES = (('uniform_2048', 2048), ('crowded_512', 512))
HBM_BYTES_PER_S = 8.0e12


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    budget = float(sys.argv[4]) if len(sys.argv) > 4 else 240.0
    t0 = time.time()
    dev = torch.device('cuda:0')
    psf = Y.models()
    out = dict(stars=ns, calls_per_region=K, regions=5,
               conditions='one MI355X, one process, mixed-precision context (the frame calls are fp64 in both modes); %d '
                          'stars on 4 model stamps shared through psf_index, positions uniform on the frame; every array '
                          'device resident; 5 regions of K calls each, median region; device events on the context '
                          'stream.  frame_gb_s counts the frame read and written once; copy_ms is a device copy of the '
                          'frame in the same run, floor_ms the same 16 bytes per pixel at 8 TB/s' % ns)
    ctx = Context(dim=128, pixscale=grid_pixscale(128), precision='mixed')
    cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
    for name, side in SCENES:
        rng = np.random.default_rng(side)
        pos = rng.uniform(0, side, (ns, 2))
        origin = (np.rint(pos) - 20).astype(np.int32)
        shift, scale = pos - np.rint(pos), rng.uniform(100, 1000, ns)
        index = (np.arange(ns) % 4).astype(np.int32)
        tps, tor, tsh, tsc, tix = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                                   for a in (psf, origin, shift, scale, index))
        frame = torch.empty((side, side), dtype=torch.float64, device=dev)
        resid = torch.empty_like(frame)
        stamps = torch.empty((ns, 40, 40), dtype=torch.float64, device=dev)
        fit = torch.empty((ns, NFIT_PSF), dtype=torch.float64, device=dev)
        fsc, fsh = torch.empty(ns, dtype=torch.float64, device=dev), torch.empty((ns, 2), dtype=torch.float64, device=dev)
        rows = torch.empty((ns, 4), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def render():
            ctx.render_stars_device(side, side, ns, 4, tps.data_ptr(), tor.data_ptr(), tsc.data_ptr(), frame.data_ptr(),
                                    shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr(), star_out_ptr=rows.data_ptr())

        def cut():
            ctx.cut_stamps_device(side, side, frame.data_ptr(), ns, tor.data_ptr(), stamps.data_ptr())

        def fit_stars():
            ctx.fit_stamps_psf_device(ns, stamps.data_ptr(), 4, tps.data_ptr(), fit.data_ptr(),
                                      psf_index_ptr=tix.data_ptr(), background=True)

        def subtract():
            ctx.render_stars_device(side, side, ns, 4, tps.data_ptr(), tor.data_ptr(), fsc.data_ptr(), resid.data_ptr(),
                                    image_ptr=frame.data_ptr(), shift_ptr=fsh.data_ptr(), psf_index_ptr=tix.data_ptr(),
                                    subtract=True)

        def copy():
            with torch.cuda.stream(cs):
                resid.copy_(frame)

        render()
        cut()
        fit_stars()
        with torch.cuda.stream(cs):
            fsc.copy_(fit[:, 0])
            fsh.copy_(torch.nan_to_num(fit[:, 1:3]).clamp(-8.0, 8.0))
            fsc.nan_to_num_(0.0, 0.0, 0.0)
        subtract()
        ctx.sync()
        f = fit.cpu().numpy()
        res = dict(side=side, stars_per_tile=float(ns * (60.0 + 31.0) ** 2 / side ** 2),
                   rendered=int(np.count_nonzero(rows.cpu().numpy()[:, 0] == 0)),
                   fits_converged=int(np.count_nonzero(f[:, 10].astype(int) & 3 == 0)),
                   residual_over_peak=float(resid.abs().max().item() / frame.max().item()))
        work = (('render', render), ('cut', cut), ('fit', fit_stars), ('subtract', subtract), ('copy', copy))
        times = {w[0]: [] for w in work}
        for _ in range(5):
            for label, call in work:
                if time.time() - t0 > budget:
                    continue
                ctx.sync()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(cs)
                for _ in range(K):
                    call()
                b.record(cs)
                b.synchronize()
                times[label].append(a.elapsed_time(b) / K)
        ctx.sync()
        nbytes = 16.0 * side * side
        for label, t in times.items():
            if not t:
                res[label] = dict(unmeasured='the time budget ran out')
                continue
            ms = float(np.median(t))
            res[label] = dict(ms_per_call=ms, min=min(t), max=max(t), regions=len(t))
            if label != 'copy':
                res[label]['stars_per_s'] = ns / (ms * 1e-3)
            if label != 'fit':
                res[label]['frame_gb_s'] = nbytes / (ms * 1e-3) / 1e9
            print('%-13s %-9s %9.3f ms (min %.3f max %.3f)  %s' % (
                name, label, ms, min(t), max(t), '  '.join('%s %.3g' % kv for kv in res[label].items()
                                                           if kv[0] in ('stars_per_s', 'frame_gb_s'))), flush=True)
        res['floor_ms'] = nbytes / HBM_BYTES_PER_S * 1e3
        out[name] = res
    ctx.close()
    out['wall_s'] = time.time() - t0
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
