"""Rate of the PSF energy metrics (mpsfr_stamp_metrics, on_device = 1) on the 35 000 device-resident stamps of the
bench configuration's count (1000 rows x 35 wavelengths at 512^2, made by device-output reconstructs), with the default
radii / boxes / fractions of psf_metrics at 0.2 arcsec per pixel, beside two yardsticks taken in the same process:

  * mpsfr_fit_stamps_elliptical on the same stamps (the existing stamp-level consumer), and
  * the copy of those stamps to the host -- what a caller pays today before integrating them in NumPy -- into pinned
    memory (the best case) and into pageable memory (what `tensor.cpu()` does).

The three are alternated: 5 regions of K calls each; kernels are timed with device events on the context's stream, the
copies with events on torch's stream; the median region is reported.  The kernel reads every stamp once: bytes / time
against the device's measured streaming bandwidth says how far it is from the floor of that read.

    python scripts/metrics_rate.py [K] [OUT.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from muse_psfr_amd import NFIT, NFIT_ELL, NMET_HEAD, Context, grid_pixscale, synthetic_rows  # noqa: E402
from muse_psfr_amd.psfrec import METRIC_BOXES, METRIC_FRACTIONS, METRIC_RADII  # noqa: E402

H = (100, 10000)
STREAM_BW = 6.29e12          # measured float4-copy bandwidth of the device [B/s]


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    n, part, dim = 1000, 100, 512
    see, gl, l0 = synthetic_rows(n)
    three = np.zeros(n, np.uint8)
    lb = np.linspace(465, 930, 35)
    ns = n * lb.size
    radii = np.array(METRIC_RADII) / 0.2
    boxes = np.array(METRIC_BOXES) / 0.2
    fracs = np.array(METRIC_FRACTIONS)
    nout = NMET_HEAD + radii.size + boxes.size + fracs.size
    dev = torch.device('cuda:0')
    out = dict(stamps=ns, stamp_bytes=ns * 1600 * 8, radii_px=radii.tolist(), boxes_px=boxes.tolist(),
               fractions=fracs.tolist(), calls_per_region=K, regions=5, stream_bw_bytes_per_s=STREAM_BW,
               conditions='one MI355X, one process; stamps of 1000 synthetic rows x 35 wavelengths (465-930 nm) at '
                          '512^2, device resident; the calls alternated, 5 regions of K calls each, median region; '
                          'kernels timed with device events on the context stream, copies on the torch stream')
    for prec in ('mixed', 'f64'):
        ctx = Context(dim=dim, pixscale=grid_pixscale(dim), precision=prec)
        psf = torch.empty((n, lb.size, 40, 40), dtype=torch.float64, device=dev)
        psum = torch.empty((lb.size, 40, 40), dtype=torch.float64, device=dev)
        fit = torch.empty((n, lb.size, NFIT), dtype=torch.float64, device=dev)
        fe = torch.empty((ns, NFIT_ELL), dtype=torch.float64, device=dev)
        met = torch.empty((ns, nout), dtype=torch.float64, device=dev)
        pinned = torch.empty(psf.shape, dtype=torch.float64, pin_memory=True)
        torch.cuda.synchronize()
        for a in range(0, n, part):
            b = a + part
            ctx.reconstruct_device(lb, see[a:b], gl[a:b], l0[a:b], three[a:b], H, 12.0, 1, None, psf[a:b].data_ptr(),
                                   psum.data_ptr(), fit[a:b].data_ptr())
            ctx.sync()
        cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
        ts = torch.cuda.current_stream(dev)

        def metrics():
            ctx.stamp_metrics_device(ns, psf.data_ptr(), met.data_ptr(), radii, boxes, fracs)

        def elliptical():
            ctx.fit_stamps_elliptical_device(ns, psf.data_ptr(), fe.data_ptr())

        def copy_pinned():
            pinned.copy_(psf, non_blocking=True)

        def copy_pageable():
            psf.cpu()

        work = (('metrics', metrics, cs), ('fit_elliptical', elliptical, cs), ('copy_to_pinned_host', copy_pinned, ts),
                ('copy_to_pageable_host', copy_pageable, ts))
        for _, call, _ in work:
            call()
        ctx.sync()
        torch.cuda.synchronize()
        times = {label: [] for label, _, _ in work}
        for _ in range(5):
            for label, call, stream in work:
                ctx.sync()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(K):
                    call()
                b.record(stream)
                b.synchronize()
                times[label].append(a.elapsed_time(b) / K)
        ctx.sync()
        res = {}
        for label, t in times.items():
            ms = float(np.median(t))
            res[label] = dict(ms_per_call=ms, min=min(t), max=max(t), us_per_stamp=ms / ns * 1e3,
                              stamp_bytes_per_s=out['stamp_bytes'] / (ms * 1e-3))
            print('%-6s %-22s %9.3f ms per %d stamps (min %.3f max %.3f)  %.1f GB/s of stamps' % (
                prec, label, ms, ns, min(t), max(t), res[label]['stamp_bytes_per_s'] / 1e9), flush=True)
        res['metrics_share_of_stream_bw'] = res['metrics']['stamp_bytes_per_s'] / STREAM_BW
        res['metrics_over_copy_to_pinned_host'] = res['metrics']['ms_per_call'] / res['copy_to_pinned_host']['ms_per_call']
        res['metrics_over_fit_elliptical'] = res['metrics']['ms_per_call'] / res['fit_elliptical']['ms_per_call']
        m = met.cpu().numpy()
        res['status_counts'] = {int(k): int(v) for k, v in zip(*np.unique(m[:, 6].astype(int), return_counts=True))}
        res['median_sqe_first_box'] = float(np.median(m[:, NMET_HEAD + radii.size]))
        res['median_r_ee50_px'] = float(np.median(m[:, NMET_HEAD + radii.size + boxes.size]))
        print('%s: metrics / copy to pinned host = %.3f, metrics / elliptical fit = %.3f, %.2f%% of the streaming '
              'bandwidth; status %s' % (prec, res['metrics_over_copy_to_pinned_host'], res['metrics_over_fit_elliptical'],
                                        100 * res['metrics_share_of_stream_bw'], res['status_counts']), flush=True)
        out[prec] = res
        ctx.close()
        del psf, pinned, fe, met, fit
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
