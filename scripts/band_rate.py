"""Band-integrated PSFs against today's route: 100 rows on the bench's 512^2 context and the native 1280^2 one,
5 nm steps over 490-930 nm (89 wavelengths) and 3 bands (white light, a 100 nm top-hat, a triangular filter).

  (a) reconstruct_band: the per-wavelength stamps reduced on the GPU (K_BAND_REDUCE), only the band stamps fitted;
  (b) today's route: reconstruct with host psf and fit, the NumPy reduction, then fit_stamps of the band stamps.

For both: the GPU time per call (device outputs, device events round K calls, median of 5 regions), the kernel
table of the library's own profiling ids (K_BAND_REDUCE runs under "stamp_sum"), the effective bandwidth of the
reduction, and the end-to-end wall time with host outputs (median of 5 calls).

    python scripts/band_rate.py [K] [OUT.json] [--quick]

K: calls per timed region (default 10); OUT.json: also write the figures there as JSON; --quick: one region, one
wall-time call (a profiler run).
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from muse_psfr_amd import Context, band_weights, grid_pixscale, synthetic_rows  # noqa: E402

H = (100, 10000)
HBM_TBS = 6.3          # achievable HBM bandwidth of the MI355X (measuring guide), TB/s


def _gpu_ms(ctx, call, K, regions):
    for _ in range(3):
        call()
    ctx.sync()
    times = []
    for _ in range(regions):
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
    return float(np.median(times)), min(times), max(times)


def _kernel_table(ctx, call, ncall):
    ctx.set_option('profile', 1)
    call()
    ctx.sync()
    ctx.profile_reset()
    for _ in range(ncall):
        call()
        ctx.sync()
    prof = {k: (ms / ncall, n / ncall) for k, (ms, n) in ctx.profile().items() if n}
    ctx.set_option('profile', 0)
    return prof


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    quick = '--quick' in sys.argv
    K = int(args[0]) if args else 10
    out_path = args[1] if len(args) > 1 else None
    regions, nwall = (1, 1) if quick else (5, 5)
    n = 100
    see, gl, l0 = synthetic_rows(n)
    three = np.zeros(n, np.uint8)
    lb = np.arange(490.0, 931.0, 5.0)
    tri = (np.array([600.0, 650.0, 700.0]), np.array([0.0, 1.0, 0.0]))
    w = band_weights(lb, [(490.0, 930.0), (600.0, 700.0), tri])
    wn = w / w.sum(axis=1, keepdims=True)
    nl, nb = lb.size, len(w)
    dev = torch.device('cuda:0')
    out = dict(rows=n, nl=nl, nband=nb)
    for dim, prec in ((512, 'mixed'), (1280, 'mixed'), (512, 'f64')):
        key = '%d_%s' % (dim, prec)
        ctx = Context(dim=dim, pixscale=grid_pixscale(dim), precision=prec)
        bpsf = torch.empty((n, nb, 40, 40), dtype=torch.float64, device=dev)
        bsum = torch.empty((nb, 40, 40), dtype=torch.float64, device=dev)
        bfit = torch.empty((n, nb, 16), dtype=torch.float64, device=dev)
        psf = torch.empty((n, nl, 40, 40), dtype=torch.float64, device=dev)
        fit = torch.empty((n, nl, 16), dtype=torch.float64, device=dev)

        def call_a():
            ctx.reconstruct_band_device(lb, w, see, gl, l0, three, H, 12.0, 1, None, None, bpsf.data_ptr(),
                                        bsum.data_ptr(), bfit.data_ptr())

        def call_b():
            ctx.reconstruct_device(lb, see, gl, l0, three, H, 12.0, 1, None, psf.data_ptr(), None, fit.data_ptr())
        res = {}
        for route, call in (('a', call_a), ('b', call_b)):
            ms, lo, hi = _gpu_ms(ctx, call, K, regions)
            res['gpu_ms_' + route] = ms
            res['gpu_ms_%s_min' % route], res['gpu_ms_%s_max' % route] = lo, hi
            res['kernels_' + route] = _kernel_table(ctx, call, 3 if quick else 10)
        # the reduction: K_STAMP_SUM of route (a) is K_BAND_REDUCE per chunk (+ the sum over lanes, [lanes][nband])
        t_red = res['kernels_a'].get('stamp_sum', (0.0, 0))[0]
        nbytes = n * nl * 1600 * (8 if prec == 'f64' else 4) + n * nb * 1600 * 8
        res['band_reduce_ms'] = t_red
        res['band_reduce_bytes'] = nbytes
        res['band_reduce_tbs'] = nbytes / (t_red * 1e-3) / 1e12 if t_red > 0 else None
        # end to end, host outputs
        wall_a, wall_b, parts = [], [], []
        ctx.reconstruct_band(lb, w, see, gl, l0, three, H)
        for _ in range(nwall):
            t0 = time.perf_counter()
            ctx.reconstruct_band(lb, w, see, gl, l0, three, H)
            wall_a.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            r = ctx.reconstruct(lb, see, gl, l0, three, H, want_sum=False)
            t1 = time.perf_counter()
            band = np.einsum('bl,tlij->tbij', wn, r['psf'])
            band.sum(axis=0)
            t2 = time.perf_counter()
            ctx.fit_stamps(band.reshape(-1, 40, 40))
            t3 = time.perf_counter()
            wall_b.append(t3 - t0)
            parts.append((t1 - t0, t2 - t1, t3 - t2))
        res['wall_ms_a'] = 1e3 * float(np.median(wall_a))
        res['wall_ms_b'] = 1e3 * float(np.median(wall_b))
        p = np.median(np.array(parts), axis=0) * 1e3
        res['wall_ms_b_parts'] = dict(reconstruct=p[0], numpy_reduce=p[1], fit_stamps=p[2])
        out[key] = res
        print('%-10s GPU/call (a) %.3f ms  (b) %.3f ms | reduce %.1f us, %.1f MB, %s TB/s (%s of %.1f) | '
              'wall (a) %.2f ms  (b) %.2f ms = %.2f reconstruct + %.2f numpy + %.2f fit' % (
                  key, res['gpu_ms_a'], res['gpu_ms_b'], 1e3 * t_red, nbytes / 1e6,
                  '%.2f' % res['band_reduce_tbs'] if res['band_reduce_tbs'] else '-',
                  '%.0f%%' % (100 * res['band_reduce_tbs'] / HBM_TBS) if res['band_reduce_tbs'] else '-', HBM_TBS,
                  res['wall_ms_a'], res['wall_ms_b'], p[0], p[1], p[2]), flush=True)
        for route in ('a', 'b'):
            print('   kernels (%s): %s' % (route, ', '.join('%s %.1f us x%.0f' % (k, 1e3 * v[0], v[1]) for k, v in
                                                        sorted(res['kernels_' + route].items(),
                                                               key=lambda kv: -kv[1][0]))), flush=True)
        ctx.close()
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1, default=float)


if __name__ == '__main__':
    main()
