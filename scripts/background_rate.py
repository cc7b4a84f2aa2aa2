"""Rates of the background map (mpsfr_frame_background with on_device = 1): a 2048 x 2048 frame at box 32 and at box 64 and
a cube of 64 layers of 320 x 320 at box 32, every array device resident.

The frames hold a gradient, unit-variance noise and 2 % of bright pixels for the clipping to reject (seeded).  Each
setting is timed by itself -- the mesh alone (mesh_out and head_out), and with the map, the rms map and a subtracted
frame written too -- beside two yardsticks taken in the same run on the same data: a device-to-device copy of the frame
(the traffic floor: the call must read the frame once) and find_stars at half 3 on it (per layer for the cube).  5
regions of K calls, device events on the context stream, the median region.  The script states numbers and is not a
pass criterion; it stops timing once `budget` seconds of wall time are spent.

    python scripts/background_rate.py [K] [OUT.json] [BUDGET_S]
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
from muse_psfr_amd import NBACK, NBACK_HEAD, NFIND, Context, grid_pixscale  # noqa: E402
import render_ref as Y  # noqa: E402

SCENES = (('frame_2048_box32', 1, 2048, 32), ('frame_2048_box64', 1, 2048, 64), ('cube_64x320_box32', 64, 320, 32))
MAX_STARS = 1 << 12


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    budget = float(sys.argv[3]) if len(sys.argv) > 3 else 240.0
    t0 = time.time()
    dev = torch.device('cuda:0')
    out = dict(calls_per_region=K, regions=5,
               conditions='one MI355X, one process, mixed-precision context (the call is fp64 in both modes); a gradient, '
                          'unit-variance noise, 2 % of pixels 50 above it; filter 3, kappa 3, max_clip 5; every array '
                          'device resident; 5 regions of K calls each, median region; device events on the context '
                          'stream.  copy_ms is a device copy of the frame (or cube) in the same run; find_ms is '
                          'find_stars at half 3, threshold 1e30 (no rows), once per layer')
    ctx = Context(dim=128, pixscale=grid_pixscale(128), precision='mixed')
    cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
    tps = torch.from_numpy(np.ascontiguousarray(Y.models()[0])).to(dev)
    for name, nl, side, box in SCENES:
        rng = np.random.default_rng(side + box)
        yy, xx = np.mgrid[:side, :side]
        data = 10.0 + 0.01 * yy - 0.005 * xx + rng.normal(size=(nl, side, side))
        data[rng.uniform(size=data.shape) < 0.02] += 50.0
        frame = torch.from_numpy(data).to(dev)
        other, bmap, rms = torch.empty_like(frame), torch.empty_like(frame), torch.empty_like(frame)
        m = -(-side // box)
        mesh = torch.empty((nl, m, m, NBACK), dtype=torch.float64, device=dev)
        head = torch.empty((nl, NBACK_HEAD), dtype=torch.float64, device=dev)
        rows = torch.empty((MAX_STARS, NFIND), dtype=torch.float64, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def mesh_only():
            ctx.frame_background_device(nl, side, side, frame.data_ptr(), mesh.data_ptr(), head.data_ptr(), box=box)

        def everything():
            ctx.frame_background_device(nl, side, side, frame.data_ptr(), mesh.data_ptr(), head.data_ptr(), box=box,
                                        map_ptr=bmap.data_ptr(), rms_ptr=rms.data_ptr(), apply_to_ptr=frame.data_ptr(),
                                        applied_ptr=other.data_ptr())

        def copy():
            with torch.cuda.stream(cs):
                other.copy_(frame)

        def find():
            for layer in range(nl):
                ctx.find_stars_device(side, side, frame[layer].data_ptr(), tps.data_ptr(), 3, 3, 1e30, MAX_STARS,
                                      rows.data_ptr(), count.data_ptr())

        work = [('mesh', mesh_only), ('mesh_and_maps', everything), ('copy', copy), ('find_half3', find)]
        for _, call in work:
            call()
            ctx.sync()
        passes = mesh.cpu().numpy()[..., 6]
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
        npix = float(nl * side * side)
        res = dict(layers=nl, side=side, box=box, cells=int(nl * m * m), mean_clip_passes=float(passes.mean()))
        for label, _ in work:
            t = times[label]
            if not t:
                res[label] = dict(unmeasured='the time budget ran out')
                continue
            ms = float(np.median(t))
            res[label] = dict(ms_per_call=ms, min=min(t), max=max(t), regions=len(t), mpixel_per_s=npix / ms / 1e3)
        for label in ('mesh', 'mesh_and_maps', 'find_half3'):
            if 'ms_per_call' in res[label] and 'ms_per_call' in res['copy']:
                res[label]['over_copy'] = res[label]['ms_per_call'] / res['copy']['ms_per_call']
        for label, _ in work:
            print('%-18s %-14s %s' % (name, label, '  '.join('%s %.4g' % kv for kv in res[label].items()
                                                             if not isinstance(kv[1], str))), flush=True)
        out[name] = res
    ctx.close()
    out['wall_s'] = time.time() - t0
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
