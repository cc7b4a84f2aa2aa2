"""Rate of the Cn2-profile call (mpsfr_reconstruct_profile, device outputs) against the legacy call: 100 rows x 35
wavelengths at 512^2, npsflin = 1, both precisions.  Timed: the legacy call, the reference's two layers as a profile,
the same atmosphere as 8 layers (each of the two split into four identical quarters: what the mixing of 8 tables
costs, on the legacy call's own work), an 8-layer profile with per-row random weights (another atmosphere: the
pruning of the per-wavelength stage, which depends on the PSF, does other work), and that at 9 field positions.  Device events
round K calls; the median of 5 regions is reported, with the ratio of each profile call to the legacy one.

    python scripts/profile_rate.py [K] [OUT.json]

K: calls per timed region (default 10); OUT.json: also write the figures there as JSON.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from muse_psfr_amd import Context, direction_perf, grid_pixscale, synthetic_rows  # noqa: E402

H = (100, 10000)
REF_DIR = (0.628163, -0.326497)
H8 = [0.0, 300.0, 1000.0, 2500.0, 5000.0, 9000.0, 13000.0, 18000.0]
WS8 = [5.0, 8.0, 10.0, 14.0, 20.0, 30.0, 25.0, 12.0]
WD8 = [0.0, 0.4, -0.8, 1.2, 2.5, -2.0, 3.0, -0.3]


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    n, dim = 100, 512
    see, gl, l0 = synthetic_rows(n)
    three = np.zeros(n, np.uint8)
    lb = np.linspace(465, 930, 35)
    cn2_8 = np.random.default_rng(1).random((n, 8))
    cn2_2 = np.stack([gl, 1 - gl], axis=1)
    cn2_8same = np.repeat(cn2_2 / 4, 4, axis=1)
    h8same = [100.0] * 4 + [10000.0] * 4
    dir8same = [REF_DIR[0]] * 4 + [REF_DIR[1]] * 4
    pos9 = direction_perf(3).T
    dev = torch.device('cuda:0')
    out = {}
    for prec in ('mixed', 'f64'):
        ctx = Context(dim=dim, pixscale=grid_pixscale(dim), precision=prec)
        for label in ('legacy', 'profile2', 'profile8_legacy_atm', 'profile8', 'profile8_field9'):
            npos = 9 if label.endswith('field9') else 1
            lead = (n, npos) if npos > 1 else (n,)
            psf = torch.empty(lead + (lb.size, 40, 40), dtype=torch.float64, device=dev)
            fit = torch.empty(lead + (lb.size, 16), dtype=torch.float64, device=dev)
            psum = torch.empty(lead[1:] + (lb.size, 40, 40), dtype=torch.float64, device=dev)
            ptrs = (psf.data_ptr(), psum.data_ptr(), fit.data_ptr())

            def call():
                if label == 'legacy':
                    ctx.reconstruct_device(lb, see, gl, l0, three, H, 12.0, 1, None, *ptrs)
                elif label == 'profile2':
                    ctx.reconstruct_profile_device(lb, see, gl, l0, cn2_2, H, (12.0, 12.0), REF_DIR, three, 1, None,
                                                   None, *ptrs)
                elif label == 'profile8_legacy_atm':
                    ctx.reconstruct_profile_device(lb, see, gl, l0, cn2_8same, h8same, 12.0, dir8same, three, 1, None,
                                                   None, *ptrs)
                elif label == 'profile8':
                    ctx.reconstruct_profile_device(lb, see, gl, l0, cn2_8, H8, WS8, WD8, three, 1, None, None, *ptrs)
                else:
                    ctx.reconstruct_profile_device(lb, see, gl, l0, cn2_8, H8, WS8, WD8, three, 0, pos9, None, *ptrs)
            for _ in range(3):
                call()
            ctx.sync()
            times = []
            for _ in range(5):
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ctx.wait_event(a.cuda_event)
                for _ in range(K):
                    call()
                ctx.stream_wait(torch.cuda.current_stream().cuda_stream)
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b) / K)
            ms = float(np.median(times))
            ns = n * npos * lb.size
            out['%s_%s' % (prec, label)] = dict(ms_per_call=ms, min=min(times), max=max(times),
                                                stamps_per_s=ns / ms * 1e3)
            print('%-6s %-16s %8.3f ms per call (min %.3f max %.3f)  %.2f M stamps/s' % (
                prec, label, ms, min(times), max(times), ns / ms / 1e3), flush=True)
        for label in ('profile2', 'profile8_legacy_atm', 'profile8', 'profile8_field9'):
            r = out['%s_%s' % (prec, label)]['ms_per_call'] / out['%s_legacy' % prec]['ms_per_call']
            out['%s_%s_over_legacy' % (prec, label)] = r
            print('%s: %s / legacy = %.3f' % (prec, label, r), flush=True)
        ctx.close()
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
