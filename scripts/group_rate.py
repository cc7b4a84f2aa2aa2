"""Rates of the friends-of-friends grouping (mpsfr_group_stars with on_device = 1) behind the star finder, on the two
scenes of scripts/find_rate.py: 20 000 stars on a 2048 x 2048 frame at a uniform density and on a crowded 512 x 512 one.

The frame is rendered by the library itself from one Moffat model stamp (sub-pixel shifts, fluxes 100 - 1000) onto a
background of 10 with unit-variance noise; the finder runs with the variance frame at half = sep = 3 and threshold 5
into buffers of 65 536 rows, and its star_out goes to the grouping as it is (stride 8, filler rows behind the count) at
crit = 2.5, 5 and 10 with max_groups = 65 536.  Each setting is timed by itself: 5 regions of K calls, device events on
the context stream, the median region.  Reported per call: ms, the six counts, and the time to read and write the
call's arrays once at the nominal 8 TB/s of HBM (positions 16 bytes per row read; label 4 bytes per row, group rows 32,
origins 8 and shifts 64 bytes per group row written) -- beside the find_stars call of the same run.  The capability is
new: the script states numbers and is not a pass criterion; it stops timing once `budget` seconds of wall time are
spent.

    python scripts/group_rate.py [K] [NSTAR] [OUT.json] [BUDGET_S]
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
from muse_psfr_amd import NFIND, NGROUP, Context, grid_pixscale  # noqa: E402
import render_ref as Y  # noqa: E402

SCENES = (('uniform_2048', 2048), ('crowded_512', 512))
CRITS = (2.5, 5.0, 10.0)
HBM_BYTES_PER_S = 8.0e12
MAX_STARS = 1 << 16


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    budget = float(sys.argv[4]) if len(sys.argv) > 4 else 240.0
    t0 = time.time()
    dev = torch.device('cuda:0')
    psf = Y.models()[:1]
    out = dict(stars=ns, calls_per_region=K, regions=5, max_stars=MAX_STARS, max_groups=MAX_STARS,
               conditions='one MI355X, one process, mixed-precision context (the grouping is the same in both modes); %d '
                          'stars of one model stamp, positions uniform on the frame, background 10, unit-variance '
                          'noise; find_stars with var at half = sep = 3, threshold 5; its %d rows of stride 8, fillers '
                          'included, are the input of group_stars; every array device resident; 5 regions of K calls '
                          'each, median region; device events on the context stream.  hbm_floor_ms: 16 bytes per input '
                          'row read, 4 per label and 104 per group row written, once each at 8 TB/s' % (ns, MAX_STARS))
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
        rows = torch.empty((MAX_STARS, NFIND), dtype=torch.float64, device=dev)
        org = torch.empty((MAX_STARS, 2), dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        label = torch.empty(MAX_STARS, dtype=torch.int32, device=dev)
        groups = torch.empty((MAX_STARS, NGROUP), dtype=torch.int32, device=dev)
        gorg = torch.empty((MAX_STARS, 2), dtype=torch.int32, device=dev)
        gsh = torch.empty((MAX_STARS, 4, 2), dtype=torch.float64, device=dev)
        counts = torch.zeros(6, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.render_stars_device(side, side, ns, 1, tps.data_ptr(), tor.data_ptr(), tsc.data_ptr(), frame.data_ptr(),
                                image_ptr=frame.data_ptr(), shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr())
        ctx.sync()

        def find():
            ctx.find_stars_device(side, side, frame.data_ptr(), tps.data_ptr(), 3, 3, 5.0, MAX_STARS, rows.data_ptr(),
                                  count.data_ptr(), var_ptr=var.data_ptr(), origin_ptr=org.data_ptr())

        def group(crit):
            def call():
                ctx.group_stars_device(side, side, MAX_STARS, rows.data_ptr(), NFIND, crit, MAX_STARS, label.data_ptr(),
                                       groups.data_ptr(), counts.data_ptr(), origin_ptr=gorg.data_ptr(),
                                       shift_ptr=gsh.data_ptr())
            return call

        work = [('find_stars', find)] + [('group_crit%g' % c, group(c)) for c in CRITS]
        res = dict(side=side)
        seen = {}
        for tag, call in work:                    # warm up; what the calls answer
            call()
            ctx.sync()
            seen[tag] = int(count.cpu().numpy()[0]) if tag == 'find_stars' else [int(v) for v in counts.cpu().numpy()]
        times = {w[0]: [] for w in work}
        for _ in range(5):
            for tag, call in work:
                if time.time() - t0 > budget:
                    continue
                ctx.sync()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(cs)
                for _ in range(K):
                    call()
                b.record(cs)
                b.synchronize()
                times[tag].append(a.elapsed_time(b) / K)
        ctx.sync()
        for tag, _ in work:
            t = times[tag]
            if not t:
                res[tag] = dict(unmeasured='the time budget ran out')
                continue
            ms = float(np.median(t))
            res[tag] = dict(ms_per_call=ms, min=min(t), max=max(t), regions=len(t))
            if tag == 'find_stars':
                res[tag]['found'] = seen[tag]
            else:
                nbytes = (16.0 + 4.0) * MAX_STARS + 104.0 * MAX_STARS
                res[tag].update(counts=seen[tag], hbm_floor_ms=nbytes / HBM_BYTES_PER_S * 1e3,
                                of_find_stars=ms / float(np.median(times['find_stars'])) if times['find_stars'] else None)
            print('%-13s %-14s %9.4f ms (min %.4f max %.4f)  %s' % (name, tag, ms, min(t), max(t), seen[tag]), flush=True)
        out[name] = res
    ctx.close()
    out['wall_s'] = time.time() - t0
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
