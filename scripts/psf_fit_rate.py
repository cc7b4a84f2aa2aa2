"""Rate of the PSF-model fit of observed stars (mpsfr_fit_stamps_psf, on_device = 1) on a few thousand device-resident
stars: the four variants (without / with background, free / fixed shift) in both precisions, beside
mpsfr_fit_stamps_observed(circular, background) on the same stars in the same run for scale.

The stars are those of tests/psf_fit_ref.noisy_stars (Moffat and golden model stamps, shifts within +-3 px, variance
plane, 3 % NaN pixels), repeated to the count; the 24 model stamps are shared through psf_index.  The calls are
alternated: 5 regions of K calls each, timed with device events on the context's stream; the median region is reported.
It reports a number and is not a pass criterion.

    python scripts/psf_fit_rate.py [K] [NSTAR] [OUT.json]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from muse_psfr_amd import NFIT_ELL, NFIT_PSF, Context, grid_pixscale  # noqa: E402
import psf_fit_ref as R  # noqa: E402

VARIANTS = (('free', False, False), ('free_back', True, False), ('fixed', False, True), ('fixed_back', True, True))


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    data, var, psf, truth = R.noisy_stars(True)
    rep = np.arange(ns) % len(data)
    dev = torch.device('cuda:0')
    out = dict(stars=ns, calls_per_region=K, regions=5,
               conditions='one MI355X, one process; %d device-resident stars (the %d stars of tests/psf_fit_ref.py '
                          'repeated: variance plane, 3 %% NaN pixels, background), %d model stamps shared through '
                          'psf_index; the calls alternated, 5 regions of K calls each, median region; device events on '
                          'the context stream' % (ns, len(data), len(psf)))
    for prec in ('mixed', 'f64'):
        ctx = Context(dim=128, pixscale=grid_pixscale(128), precision=prec)
        td, tv = (torch.from_numpy(np.ascontiguousarray(a[rep])).to(dev) for a in (data, var))
        tp = torch.from_numpy(np.ascontiguousarray(psf)).to(dev)
        tix = torch.from_numpy(rep.astype(np.int32)).to(dev)
        tsh = torch.from_numpy(np.ascontiguousarray((np.round(truth[:, 1:3] * 8) / 8)[rep])).to(dev)
        tf = torch.empty((ns, NFIT_PSF), dtype=torch.float64, device=dev)
        to = torch.empty((ns, NFIT_ELL), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
        work = [('observed_circular_back', 18, 10, to, lambda: ctx.fit_stamps_observed_device(
            ns, td.data_ptr(), to.data_ptr(), tv.data_ptr(), background=True, circular=True))]
        for name, back, fixed in VARIANTS:
            work.append(('psf_%s' % name, 10, 5, tf, lambda b=back, f=fixed: ctx.fit_stamps_psf_device(
                ns, td.data_ptr(), len(psf), tp.data_ptr(), tf.data_ptr(), var_ptr=tv.data_ptr(),
                psf_index_ptr=tix.data_ptr(), shift_ptr=tsh.data_ptr() if f else None, background=b, fixed_shift=f)))
        res = {}
        for label, istat, iit, buf, call in work:
            call()
            ctx.sync()
            f = buf.cpu().numpy()
            res[label] = dict(converged=int(np.count_nonzero(f[:, istat].astype(int) & 3 == 0)),
                              median_iterations=float(np.median(f[:, iit])))
        times = {w[0]: [] for w in work}
        for _ in range(5):
            for label, _, _, _, call in work:
                ctx.sync()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(cs)
                for _ in range(K):
                    call()
                b.record(cs)
                b.synchronize()
                times[label].append(a.elapsed_time(b) / K)
        ctx.sync()
        for label, t in times.items():
            ms = float(np.median(t))
            res[label].update(ms_per_call=ms, min=min(t), max=max(t), stars_per_s=ns / (ms * 1e-3))
            print('%-6s %-26s %9.3f ms per %d stars (min %.3f max %.3f)  %10.0f stars/s  converged %d, median '
                  'iterations %.0f' % (prec, label, ms, ns, min(t), max(t), res[label]['stars_per_s'],
                                       res[label]['converged'], res[label]['median_iterations']), flush=True)
        out[prec] = res
        ctx.close()
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
