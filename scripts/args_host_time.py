"""Host time of the Python wrappers alone: Context methods on the stub library of tests/test_lib_calls_host.py (no
GPU, no libmpsfr.so), so that what is timed is the argument checks and the ctypes marshalling in front of a C call.

  fit_stamps_device, fit_frame_psf_device, fit_cube_psf_free_device   pointer-only arguments
  fit_frame_psf                                                       host form, a 64 x 64 frame with 8 stars
200 warm-up calls, then 5 regions of 2000 calls; printed per call as JSON: the regions in us per call, their median and
spread (largest - smallest).  To compare two versions of the package run the script once per version, alternating, each
in a fresh process; PACKAGE_ROOT is the directory that holds muse_psfr_amd/ (default: this tree).
    python scripts/args_host_time.py [PACKAGE_ROOT]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT)
from test_lib_calls_host import make_ctx  # noqa: E402

REGIONS, CALLS, WARMUP = 5, 2000, 200


def regions(ctx, call):
    us = []
    for k in range(REGIONS + 1):                 # (region 0: the warm-up)
        t0 = time.perf_counter()
        for _ in range(CALLS if k else WARMUP):
            call()
        us.append((time.perf_counter() - t0) / CALLS * 1e6)
        ctx.lib.calls.clear()                    # the stub's record of the calls, outside the clock
    us = us[1:]
    return {'us_per_call': [round(u, 3) for u in us], 'median': round(float(np.median(us)), 3),
            'spread': round(max(us) - min(us), 3)}


def main():
    ctx = make_ctx()
    rng = np.random.default_rng(5)
    frame, var = rng.normal(size=(64, 64)), rng.uniform(1.0, 2.0, (64, 64))
    psf = rng.uniform(size=(4, 40, 40))
    origin = rng.integers(-10, 30, (8, 2)).astype(np.int32)
    shift, index = rng.uniform(-0.5, 0.5, (8, 2)), (np.arange(8) % 4).astype(np.int32)
    calls = {
        'fit_stamps_device': lambda: ctx.fit_stamps_device(200, 0x1000, 0x2000),
        'fit_frame_psf_device': lambda: ctx.fit_frame_psf_device(
            64, 64, 0x1000, 8, 4, 0x2000, 0x3000, 0x4000, 0x5000, var_ptr=0x6000, shift_ptr=0x7000,
            psf_index_ptr=0x8000, radius=8.0, background=True, max_iter=20, tol=1e-10),
        'fit_cube_psf_free_device': lambda: ctx.fit_cube_psf_free_device(
            16, 64, 64, 0x1000, 8, 4, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, var_ptr=0x9000,
            shift_ptr=0xA000, psf_index_ptr=0xB000),
        'fit_frame_psf': lambda: ctx.fit_frame_psf(frame, psf, origin, var=var, shift=shift, psf_index=index),
    }
    print(json.dumps({name: regions(ctx, call) for name, call in calls.items()}), flush=True)


if __name__ == '__main__':
    main()
