"""Rate of the PSF-model fit of blended stars (mpsfr_fit_groups_psf, on_device = 1) on a few thousand device-resident
groups: K = 2, 3, 4 sources, the three modes (free, common, fixed) with a background, in both precisions, beside
mpsfr_fit_stamps_psf(free shift, background) on the same number of stamps in the same run for scale.

The groups are those of tests/psf_group_ref.groups (Moffat and golden model stamps, positions within +-6 px, variance
plane, 3 % NaN pixels), repeated to the count; the 12 model stamps of a size are shared through psf_index.  The calls
are alternated: 5 regions of N calls each, timed with device events on the context's stream; the median region is
reported.  It reports a number and is not a pass criterion.

    python scripts/group_fit_rate.py [N] [NSTAMP] [OUT.json]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from muse_psfr_amd import NFIT_GROUP, NFIT_PSF, Context, grid_pixscale  # noqa: E402
import psf_group_ref as G  # noqa: E402


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    dev = torch.device('cuda:0')
    out = dict(stamps=ns, calls_per_region=N, regions=5,
               conditions='one MI355X, one process; %d device-resident stamps (the %d groups of each size of '
                          'tests/psf_group_ref.py repeated: variance plane, 3 %% NaN pixels, background), the model '
                          'stamps shared through psf_index; the calls alternated, 5 regions of N calls each, median '
                          'region; device events on the context stream' % (ns, G.NGROUP))
    rep = np.arange(ns) % G.NGROUP
    for prec in ('mixed', 'f64'):
        ctx = Context(dim=128, pixscale=grid_pixscale(128), precision=prec)
        cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
        tix = torch.from_numpy(rep.astype(np.int32)).to(dev)
        tg = torch.empty((ns, NFIT_GROUP), dtype=torch.float64, device=dev)
        tf = torch.empty((ns, NFIT_PSF), dtype=torch.float64, device=dev)
        keep, work = [], []
        for K in G.SIZES:
            data, var, psf, F, pos, b = G.groups(K, True)
            td, tv = (torch.from_numpy(np.ascontiguousarray(a[rep])).to(dev) for a in (data, var))
            tp = torch.from_numpy(np.ascontiguousarray(psf)).to(dev)
            keep += [td, tv, tp]
            if K == G.SIZES[0]:            # the single-star fit on the same stamps, for scale
                work.append(('psf_free_back', 10, 5, tf, lambda d=td, v=tv, p=tp: ctx.fit_stamps_psf_device(
                    ns, d.data_ptr(), G.NGROUP, p.data_ptr(), tf.data_ptr(), var_ptr=v.data_ptr(),
                    psf_index_ptr=tix.data_ptr())))
            for mode in G.MODES:
                tsh = torch.from_numpy(np.ascontiguousarray(G.given_positions(pos, mode)[rep])).to(dev)
                keep.append(tsh)
                work.append(('group_k%d_%s_back' % (K, mode), 4, 3, tg,
                             lambda d=td, v=tv, p=tp, s=tsh, k=K, m=mode: ctx.fit_groups_psf_device(
                                 ns, k, d.data_ptr(), G.NGROUP, p.data_ptr(), s.data_ptr(), tg.data_ptr(),
                                 var_ptr=v.data_ptr(), psf_index_ptr=tix.data_ptr(), background=True, mode=m)))
        torch.cuda.synchronize()
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
                for _ in range(N):
                    call()
                b.record(cs)
                b.synchronize()
                times[label].append(a.elapsed_time(b) / N)
        ctx.sync()
        for label, t in times.items():
            ms = float(np.median(t))
            res[label].update(ms_per_call=ms, min=min(t), max=max(t), stamps_per_s=ns / (ms * 1e-3))
            print('%-6s %-26s %9.3f ms per %d stamps (min %.3f max %.3f)  %10.0f stamps/s  converged %d, median '
                  'iterations %.0f' % (prec, label, ms, ns, min(t), max(t), res[label]['stamps_per_s'],
                                       res[label]['converged'], res[label]['median_iterations']), flush=True)
        out[prec] = res
        ctx.close()
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
