"""Rate of the PSF-model fit of star cubes (mpsfr_fit_spectra_psf, on_device = 1) on 256 device-resident stars of 32
layers: with the background, without and with the drift, in both precisions of a context (the kernel is fp64 in both),
beside mpsfr_fit_stamps_psf(free shift, background) on the same 8192 stamps in the same run for scale.

The stars are 8 cubes of tests/psf_spec_ref.make_star (Moffat models of FWHM 4.5 -> 2.6 px, peak pixel at 20 sigma per
layer, variance cube, 3 % NaN pixels), repeated to the count; the 8 model cubes are shared through psf_index.  The calls
are alternated: 5 regions of K calls each, timed with device events on the context's stream; the median region is
reported.  It reports a number and is not a pass criterion.

    python scripts/spec_fit_rate.py [K] [NSTAR] [NL] [OUT.json]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from muse_psfr_amd import NFIT_PSF, NFIT_SPEC, NFIT_SPEC_LAYER, Context, grid_pixscale  # noqa: E402
import psf_spec_ref as SR  # noqa: E402


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    nl = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    rng = np.random.default_rng(21)
    made = [SR.make_star(rng, nl, 20, True, True) for _ in range(8)]
    cubes, var, psf = (np.array([m[i] for m in made]) for i in range(3))
    x = made[0][3]
    rep = np.arange(ns) % len(made)
    dev = torch.device('cuda:0')
    out = dict(stars=ns, layers=nl, stamps=ns * nl, calls_per_region=K, regions=5,
               conditions='one MI355X, one process; %d device-resident star cubes of %d layers (8 cubes of '
                          'tests/psf_spec_ref.make_star repeated: peak pixel at 20 sigma per layer, variance cube, 3 %% '
                          'NaN pixels, background), 8 model cubes shared through psf_index, the default start; '
                          'fit_stamps_psf on the same %d stamps; the calls alternated, 5 regions of K calls each, median '
                          'region; device events on the context stream' % (ns, nl, ns * nl))
    for prec in ('mixed', 'f64'):
        ctx = Context(dim=128, pixscale=grid_pixscale(128), precision=prec)
        td, tv = (torch.from_numpy(np.ascontiguousarray(a[rep])).to(dev) for a in (cubes, var))
        tp = torch.from_numpy(np.ascontiguousarray(psf)).to(dev)
        tix = torch.from_numpy(rep.astype(np.int32)).to(dev)
        # the single-stamp fit: stamp (star, layer) against model stamp (its cube, layer)
        tix1 = torch.from_numpy((rep[:, None] * nl + np.arange(nl)[None, :]).astype(np.int32).ravel()).to(dev)
        tf = torch.empty((ns, NFIT_SPEC + NFIT_SPEC_LAYER * nl), dtype=torch.float64, device=dev)
        t1 = torch.empty((ns * nl, NFIT_PSF), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
        work = [('stamps_psf_free_back', 10, 5, t1, lambda: ctx.fit_stamps_psf_device(
            ns * nl, td.data_ptr(), len(made) * nl, tp.data_ptr(), t1.data_ptr(), var_ptr=tv.data_ptr(),
            psf_index_ptr=tix1.data_ptr(), background=True))]
        for name, xx in (('spectra_back', None), ('spectra_back_drift', x)):
            work.append((name, 10, 9, tf, lambda xx=xx: ctx.fit_spectra_psf_device(
                ns, nl, td.data_ptr(), len(made), tp.data_ptr(), tf.data_ptr(), var_ptr=tv.data_ptr(),
                psf_index_ptr=tix.data_ptr(), background=True, x=xx)))
        res = {}
        for label, istat, iit, buf, call in work:
            call()
            ctx.sync()
            f = buf.cpu().numpy()
            res[label] = dict(converged=int(np.count_nonzero(f[:, istat].astype(int) & 3 == 0)), rows=int(len(f)),
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
            res[label].update(ms_per_call=ms, min=min(t), max=max(t), stamps_per_s=ns * nl / (ms * 1e-3),
                              stars_per_s=ns / (ms * 1e-3) if label.startswith('spectra') else None)
            print('%-6s %-22s %9.3f ms per %d stamps (min %.3f max %.3f)  %10.0f stamps/s  converged %d of %d, median '
                  'iterations %.0f' % (prec, label, ms, ns * nl, min(t), max(t), res[label]['stamps_per_s'],
                                       res[label]['converged'], res[label]['rows'], res[label]['median_iterations']),
                  flush=True)
        out[prec] = res
        ctx.close()
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
