"""Rate of the field-resolved call (mpsfr_reconstruct_field, device outputs): 100 rows x 35 wavelengths at 512^2,
1 and 9 positions, both precisions.  Device events round K calls; the median of 5 regions is reported, with the
ratio of the 9-position call to the 1-position one (each (row, position) pair does the work of one row, so
about 9 is expected).  The averaged npsflin = 1 and npsflin = 3 calls are timed the same way for comparison.

    python scripts/field_rate.py [K] [OUT.json]

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


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    n, dim = 100, 512
    see, gl, l0 = synthetic_rows(n)
    three = np.zeros(n, np.uint8)
    lb = np.linspace(465, 930, 35)
    dev = torch.device('cuda:0')
    out = {}
    for prec in ('mixed', 'f64'):
        ctx = Context(dim=dim, pixscale=grid_pixscale(dim), precision=prec)
        for label, npos in (('field1', 1), ('field9', 9), ('avg1', 1), ('avg9', 9)):
            pos = direction_perf(3).T if npos == 9 else np.zeros((1, 2))
            psf = torch.empty((n, npos, lb.size, 40, 40), dtype=torch.float64, device=dev)
            fit = torch.empty((n, npos, lb.size, 16), dtype=torch.float64, device=dev)
            psum = torch.empty((npos, lb.size, 40, 40), dtype=torch.float64, device=dev)

            def call():
                if label.startswith('field'):
                    ctx.reconstruct_field_device(lb, see, gl, l0, three, H, 12.0, pos, None, psf.data_ptr(),
                                                 psum.data_ptr(), fit.data_ptr())
                else:
                    ctx.reconstruct_device(lb, see, gl, l0, three, H, 12.0, 3 if npos == 9 else 1, None,
                                           psf.data_ptr(), psum.data_ptr(), fit.data_ptr())
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
            ns = n * (npos if label.startswith('field') else 1) * lb.size
            out['%s_%s' % (prec, label)] = dict(ms_per_call=ms, min=min(times), max=max(times),
                                                stamps_per_s=ns / ms * 1e3)
            print('%-6s %-7s %8.3f ms per call (min %.3f max %.3f)  %.2f M stamps/s' % (
                prec, label, ms, min(times), max(times), ns / ms / 1e3), flush=True)
        out['%s_ratio_9_to_1' % prec] = out['%s_field9' % prec]['ms_per_call'] / out['%s_field1' % prec]['ms_per_call']
        print('%s: 9 positions / 1 position = %.2f' % (prec, out['%s_ratio_9_to_1' % prec]), flush=True)
        ctx.close()
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
