"""Rate of the elliptical Moffat fit (mpsfr_fit_stamps_elliptical) against the circular one (mpsfr_fit_stamps) on the
3500 stamps of one bench step: 100 rows x 35 wavelengths at 512^2, made by a device-output reconstruct.  Both fits
run on_device = 1 on those stamps, in both precisions, alternated in one process: 5 regions of K calls of each,
timed with device events on the context's stream; the median region is reported, with the mean iteration counts (fit_out[7] of the
circular rows, fit_out[10] of the elliptical ones: LM passes + polish passes).

    python scripts/fit_ell_rate.py [K] [OUT.json]

K: calls per timed region (default 10); OUT.json: also write the figures there as JSON.  Kernel times: run it under
rocprofv3 --kernel-trace --stats (k_fit / k_fit_ell).
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from muse_psfr_amd import NFIT, NFIT_ELL, Context, grid_pixscale, synthetic_rows  # noqa: E402

H = (100, 10000)


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    n, dim = 100, 512
    see, gl, l0 = synthetic_rows(n)
    three = np.zeros(n, np.uint8)
    lb = np.linspace(465, 930, 35)
    ns = n * lb.size
    dev = torch.device('cuda:0')
    out = {}
    for prec in ('mixed', 'f64'):
        ctx = Context(dim=dim, pixscale=grid_pixscale(dim), precision=prec)
        psf = torch.empty((n, lb.size, 40, 40), dtype=torch.float64, device=dev)
        psum = torch.empty((lb.size, 40, 40), dtype=torch.float64, device=dev)
        fit = torch.empty((n, lb.size, NFIT), dtype=torch.float64, device=dev)
        fc = torch.empty((ns, NFIT), dtype=torch.float64, device=dev)
        fe = torch.empty((ns, NFIT_ELL), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.reconstruct_device(lb, see, gl, l0, three, H, 12.0, 1, None, psf.data_ptr(), psum.data_ptr(),
                               fit.data_ptr())
        ctx.sync()

        def circular():
            rc = ctx.lib.mpsfr_fit_stamps(ctx._h, ns, C.c_void_p(psf.data_ptr()), C.c_void_p(fc.data_ptr()), 1)
            assert rc == 0, rc

        def elliptical():
            ctx.fit_stamps_elliptical_device(ns, psf.data_ptr(), fe.data_ptr())

        for _ in range(3):
            circular()
            elliptical()
        ctx.sync()
        # both fits are queued on the context's stream: the events are recorded there
        cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
        times = {'circular': [], 'elliptical': []}
        for _ in range(5):
            for label, call in (('circular', circular), ('elliptical', elliptical)):
                ctx.sync()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(cs)
                for _ in range(K):
                    call()
                b.record(cs)
                b.synchronize()
                times[label].append(a.elapsed_time(b) / K)
        ctx.sync()
        its = {'circular': float(fc[:, 7].mean()), 'elliptical': float(fe[:, 10].mean())}
        st_e = fe[:, 18].cpu().numpy().astype(int)
        for label, t in times.items():
            ms = float(np.median(t))
            out['%s_%s' % (prec, label)] = dict(ms_per_call=ms, min=min(t), max=max(t), us_per_stamp=ms / ns * 1e3,
                                                mean_iterations=its[label])
            print('%-6s %-10s %8.3f ms per %d stamps (min %.3f max %.3f)  %.3f us/stamp  %.2f iterations' % (
                prec, label, ms, ns, min(t), max(t), ms / ns * 1e3, its[label]), flush=True)
        r = out['%s_elliptical' % prec]['ms_per_call'] / out['%s_circular' % prec]['ms_per_call']
        out['%s_elliptical_over_circular' % prec] = r
        out['%s_elliptical_status_counts' % prec] = {int(k): int(v) for k, v in zip(*np.unique(st_e, return_counts=True))}
        ba = (fe[:, 8] / fe[:, 7]).cpu().numpy()
        print('%s: elliptical / circular = %.3f; status %s; b/a %.4f .. %.4f' % (
            prec, r, out['%s_elliptical_status_counts' % prec], ba.min(), ba.max()), flush=True)
        ctx.close()
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
