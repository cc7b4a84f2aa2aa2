"""Host wall time of queueing a device-form stamp call and a device-form frame call (on_device = 1: the call returns
once it is queued, so the time the host spends inside it is what a caller's loop pays per call).

  fit_stamps      mpsfr_fit_stamps on 200 stamps (Moffat profiles of varying width)
  fit_frame_psf   mpsfr_fit_frame_psf on a 64 x 64 frame with 8 stars of four model stamps, variance plane, shifts and
                  indices given, background on, max_iter = 20

Each call: 10 calls to warm up and a synchronise, then 5 regions of 50 calls with a host clock around the 50 calls and a
synchronise of the context between regions (outside the clock).  Printed per call: the five regions in us per call,
their median and their spread (largest - smallest).  The library is the tree's, or another build through
MPSFR_LIB_PATH; to compare two builds run the script once per build, alternating, in one visit of the machine.
The script states numbers and is not a pass criterion.

    python scripts/stamp_calls_host_time.py [OUT.json]
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
from muse_psfr_amd import NFIT, NFRAMEFIT, Context, grid_pixscale  # noqa: E402
from muse_psfr_amd._lib import LIB_PATH, load as load_lib  # noqa: E402
import render_ref as Y  # noqa: E402

REGIONS, CALLS, WARMUP = 5, 50, 10


def regions(ctx, call):
    for _ in range(WARMUP):
        call()
    ctx.sync()
    us = []
    for _ in range(REGIONS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        us.append((time.perf_counter() - t0) / CALLS * 1e6)
        ctx.sync()
    return {'us_per_call': [round(u, 2) for u in us], 'median': round(float(np.median(us)), 2),
            'spread': round(max(us) - min(us), 2)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(23)
    ctx = Context(dim=128, pixscale=grid_pixscale(128), precision='mixed')

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # 200 stamps: Moffat profiles, beta 2.5, widths 2 .. 5 pixels, centres within half a pixel of (20, 20)
    nstamp = 200
    p, q = np.meshgrid(np.arange(40.0), np.arange(40.0), indexing='ij')
    cen = 20.0 + rng.uniform(-0.5, 0.5, (nstamp, 2))
    alpha = rng.uniform(2.0, 5.0, nstamp)
    r2 = (p[None] - cen[:, 0, None, None]) ** 2 + (q[None] - cen[:, 1, None, None]) ** 2
    stamps = to_dev((1.0 + r2 / alpha[:, None, None] ** 2) ** -2.5)
    fit = torch.empty((nstamp, NFIT), dtype=torch.float64, device=dev)

    # a 64 x 64 frame with 8 stars, rendered by the library itself
    side, ns = 64, 8
    pos = rng.uniform(8, side - 8, (ns, 2))
    origin = (np.rint(pos) - 20).astype(np.int32)
    shift, flux = pos - np.rint(pos), rng.uniform(200, 5000, ns)
    index = (np.arange(ns) % 4).astype(np.int32)
    tps, tor, tsh, tfl, tix = (to_dev(a) for a in (Y.models(), origin, shift, flux, index))
    model = torch.zeros((side, side), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.render_stars_device(side, side, ns, 4, tps.data_ptr(), tor.data_ptr(), tfl.data_ptr(), model.data_ptr(),
                            shift_ptr=tsh.data_ptr(), psf_index_ptr=tix.data_ptr())
    ctx.sync()
    var = 4.0 + model / 2.0
    frame = model + 7.0 + to_dev(rng.normal(size=(side, side))) * torch.sqrt(var)
    rows = torch.empty((ns, NFRAMEFIT), dtype=torch.float64, device=dev)
    head = torch.empty(NFRAMEFIT, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def fit_stamps():
        ctx.fit_stamps_device(nstamp, stamps.data_ptr(), fit.data_ptr())

    def fit_frame():
        ctx.fit_frame_psf_device(side, side, frame.data_ptr(), ns, 4, tps.data_ptr(), tor.data_ptr(), rows.data_ptr(),
                                 head.data_ptr(), var_ptr=var.data_ptr(), shift_ptr=tsh.data_ptr(),
                                 psf_index_ptr=tix.data_ptr(), radius=8.0, background=True, max_iter=20, tol=1e-10)

    out = {'library': os.path.relpath(LIB_PATH, ROOT), 'build_id': load_lib().mpsfr_build_id().decode(),
           'regions': REGIONS, 'calls_per_region': CALLS,
           'fit_stamps': regions(ctx, fit_stamps), 'fit_frame_psf': regions(ctx, fit_frame)}
    # the calls did their work: a circular fit of every stamp, a solve that accepted the stars
    out['fit_stamps']['finite_rows'] = int(torch.isfinite(fit).all(dim=1).sum().item())
    out['fit_frame_psf']['stars_fitted'] = int((rows[:, 7] == 0).sum().item())
    print(json.dumps(out), flush=True)
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
