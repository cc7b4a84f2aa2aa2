"""Rates of the star finder (mpsfr_find_stars with on_device = 1) on two scenes of 20 000 stars: a 2048 x 2048 frame at a
uniform density and a crowded 512 x 512 one, with and without the variance frame, at half = 3 and 7 (sep = half).

The frame is rendered by the library itself from one Moffat model stamp (sub-pixel shifts, fluxes 100 - 1000) onto a
background of 10 with unit-variance noise; the finder runs at threshold 5 (sigma with var; without var the statistic is
the amplitude, and the threshold 60 is about 5 sigma_H) into buffers of 65 536 rows.  Each setting is timed by itself:
5 regions of K calls, device events on the context stream, the median region.  Reported per call: ms, Mpixel/s, frame
GB/s (the planes the call reads -- image, var -- and the map it writes, once each: 16 or 24 bytes per pixel) and the
stars found -- beside the two floors: a plain device copy of the frame timed in the same run with the same bytes at the
nominal 8 TB/s of HBM, and the 5 (2 half + 1)^2 fp64 FMAs per pixel at the card's nominal vector fp64 rate (78.6 TFLOP/s:
39.3e12 FMA/s).  The script states numbers and is not a pass criterion; it stops timing once `budget` seconds of wall
time are spent.

    python scripts/find_rate.py [K] [NSTAR] [OUT.json] [BUDGET_S]
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
from muse_psfr_amd import NFIND, Context, grid_pixscale  # noqa: E402
import render_ref as Y  # noqa: E402

SCENES = (('uniform_2048', 2048), ('crowded_512', 512))
HBM_BYTES_PER_S = 8.0e12
FMA_PER_S = 78.6e12 / 2
MAX_STARS = 1 << 16


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    budget = float(sys.argv[4]) if len(sys.argv) > 4 else 240.0
    t0 = time.time()
    dev = torch.device('cuda:0')
    psf = Y.models()[:1]
    out = dict(stars=ns, calls_per_region=K, regions=5, max_stars=MAX_STARS,
               conditions='one MI355X, one process, mixed-precision context (the finder is fp64 in both modes); %d stars '
                          'of one model stamp, positions uniform on the frame, background 10, unit-variance noise; '
                          'threshold 5 with var, 60 without; sep = half; every array device resident; 5 regions of K '
                          'calls each, median region; device events on the context stream.  frame_gb_s counts image, var '
                          'and the map once each; copy_ms is a device copy of the frame in the same run, hbm_floor_ms '
                          'the counted bytes at 8 TB/s, fma_floor_ms 5 (2 half + 1)^2 FMAs per pixel at 39.3e12 FMA/s' % ns)
    ctx = Context(dim=128, pixscale=grid_pixscale(128), precision='mixed')
    cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
    for name, side in SCENES:
        rng = np.random.default_rng(side)
        pos = rng.uniform(0, side, (ns, 2))
        origin = (np.rint(pos) - 20).astype(np.int32)
        shift, scale = pos - np.rint(pos), rng.uniform(100, 1000, ns)
        index = np.zeros(ns, dtype=np.int32)
        back = 10.0 + rng.normal(size=(side, side))
        tps, tor, tsh, tsc, tix, frame = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                                          for a in (psf, origin, shift, scale, index, back))
        var = torch.ones_like(frame)
        other = torch.empty_like(frame)
        rows = torch.empty((MAX_STARS, NFIND), dtype=torch.float64, device=dev)
        org = torch.empty((MAX_STARS, 2), dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.render_stars_device(side, side, ns, 1, tps.data_ptr(), tor.data_ptr(), tsc.data_ptr(), frame.data_ptr(),
                                image_ptr=frame.data_ptr(), shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr())
        ctx.sync()

        def find(usevar, half):
            def call():
                ctx.find_stars_device(side, side, frame.data_ptr(), tps.data_ptr(), half, half, 5.0 if usevar else 60.0,
                                      MAX_STARS, rows.data_ptr(), count.data_ptr(),
                                      var_ptr=var.data_ptr() if usevar else None, origin_ptr=org.data_ptr())
            return call

        def copy():
            with torch.cuda.stream(cs):
                other.copy_(frame)

        work = [('var%d_half%d' % (usevar, half), find(usevar, half), usevar, half)
                for usevar in (1, 0) for half in (3, 7)] + [('copy', copy, 0, 0)]
        res = dict(side=side)
        found = {}
        for label, call, _, _ in work:                    # warm up; the stars found
            call()
            ctx.sync()
            if label != 'copy':
                found[label] = int(count.cpu().numpy()[0])
        times = {w[0]: [] for w in work}
        for _ in range(5):
            for label, call, _, _ in work:
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
        npix = float(side * side)
        for label, _, usevar, half in work:
            t = times[label]
            if not t:
                res[label] = dict(unmeasured='the time budget ran out')
                continue
            ms = float(np.median(t))
            nbytes = 16.0 * npix if label == 'copy' else (16.0 + 8.0 * usevar) * npix
            res[label] = dict(ms_per_call=ms, min=min(t), max=max(t), regions=len(t), mpixel_per_s=npix / ms / 1e3,
                              frame_gb_s=nbytes / (ms * 1e-3) / 1e9, hbm_floor_ms=nbytes / HBM_BYTES_PER_S * 1e3)
            if label != 'copy':
                res[label]['found'] = found[label]
                res[label]['fma_floor_ms'] = 5.0 * (2 * half + 1) ** 2 * npix / FMA_PER_S * 1e3
            print('%-13s %-11s %9.3f ms (min %.3f max %.3f)  %s' % (
                name, label, ms, min(t), max(t), '  '.join('%s %.4g' % kv for kv in res[label].items()
                                                           if kv[0] in ('mpixel_per_s', 'frame_gb_s', 'found',
                                                                        'hbm_floor_ms', 'fma_floor_ms'))), flush=True)
        out[name] = res
    ctx.close()
    out['wall_s'] = time.time() - t0
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
