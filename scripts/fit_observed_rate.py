"""Rate of the weighted Moffat fit of observed stars (mpsfr_fit_stamps_observed, on_device = 1) on a few thousand
device-resident stamps: the four variants (circular / elliptical, without / with background) in both precisions, on
noisy stamps with a variance plane and masked pixels and on the same stars without noise (var = NULL, nothing
masked), beside mpsfr_fit_stamps_elliptical on the noise-free stamps in the same run for scale.

The calls are alternated: 5 regions of K calls each, timed with device events on the context's stream; the median
region is reported.

    python scripts/fit_observed_rate.py [K] [NSTAMP] [OUT.json]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from muse_psfr_amd import NFIT_ELL, Context, grid_pixscale  # noqa: E402
import moffat_ell_ref as M  # noqa: E402

VARIANTS = (('circular', True, False), ('circular_back', True, True), ('elliptical', False, False),
            ('elliptical_back', False, True))


def stamps(n, seed=7):
    """n stars as in tests/moffat_obs_ref.noisy_stamps (FWHM 3-8 px, n 1.8-4, b/a 0.6-1, peak SNR 30-1000, 2 % NaN
    pixels, one 3 x 3 block of var = 0 and, for the variants that fit one, a background of -2 ... 5 % of the peak):
    (clean, noisy, var, noisy on its background).  The variants without a background term get the stars without one:
    on a pedestal such a fit has no finite minimum for some stars (n -> 1/2 with a vanishing width imitates the
    pedestal) and ends at the iteration cap."""
    rng = np.random.default_rng(seed)
    clean, noisy, var = np.empty((n, 40, 40)), np.empty((n, 40, 40)), np.empty((n, 40, 40))
    back = np.empty(n)
    for k in range(n):
        peak = rng.uniform(0.5, 2)
        p0, q0 = 19.5 + rng.uniform(-2, 2, 2)
        m = M.stamp(peak, p0, q0, rng.uniform(3, 8), rng.uniform(0.6, 1), rng.uniform(0, 180), rng.uniform(1.8, 4))
        snr = 10 ** rng.uniform(np.log10(30), np.log10(1000))
        va = (peak / snr) ** 2 * (0.2 + 0.8 * m / peak)
        d = m + rng.normal(size=m.shape) * np.sqrt(va)
        d[rng.uniform(size=m.shape) < 0.02] = np.nan
        i, j = rng.integers(3, 34, 2)
        va[i:i + 3, j:j + 3] = 0.0
        clean[k], noisy[k], var[k], back[k] = m, d, va, rng.uniform(-0.02, 0.05) * peak
    return clean, noisy, var, noisy + back[:, None, None]


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    clean, noisy, var, noisy_back = stamps(ns)
    dev = torch.device('cuda:0')
    out = dict(stamps=ns, calls_per_region=K, regions=5,
               conditions='one MI355X, one process; %d device-resident stamps; noisy: variance plane, 2 %% NaN pixels, '
                          'a 3 x 3 block of var = 0, a background where one is fitted; clean: the same stars without '
                          'noise, var = NULL; the '
                          'calls alternated, 5 regions of K calls each, median region; device events on the context '
                          'stream' % ns)
    for prec in ('mixed', 'f64'):
        ctx = Context(dim=128, pixscale=grid_pixscale(128), precision=prec)
        tc, tn, tv, tb = (torch.from_numpy(a).to(dev) for a in (clean, noisy, var, noisy_back))
        tf = torch.empty((ns, NFIT_ELL), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        cs = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)
        work = [('fit_stamps_elliptical_clean', lambda: ctx.fit_stamps_elliptical_device(ns, tc.data_ptr(),
                                                                                       tf.data_ptr()))]
        for name, circ, back in VARIANTS:
            work.append(('observed_%s_noisy' % name, lambda c=circ, b=back: ctx.fit_stamps_observed_device(
                ns, (tb if b else tn).data_ptr(), tf.data_ptr(), tv.data_ptr(), background=b, circular=c)))
            work.append(('observed_%s_clean' % name, lambda c=circ, b=back: ctx.fit_stamps_observed_device(
                ns, tc.data_ptr(), tf.data_ptr(), None, background=b, circular=c)))
        res = {}
        for label, call in work:
            call()
            ctx.sync()
            f = tf.cpu().numpy()
            res[label] = dict(converged=int(np.count_nonzero(f[:, 18].astype(int) & 3 == 0)),
                              median_iterations=float(np.median(f[:, 10])))
        times = {label: [] for label, _ in work}
        for _ in range(5):
            for label, call in work:
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
            res[label].update(ms_per_call=ms, min=min(t), max=max(t), stamps_per_s=ns / (ms * 1e-3))
            print('%-6s %-34s %9.3f ms per %d stamps (min %.3f max %.3f)  %10.0f stamps/s  converged %d, median '
                  'iterations %.0f' % (prec, label, ms, ns, min(t), max(t), res[label]['stamps_per_s'],
                                       res[label]['converged'], res[label]['median_iterations']), flush=True)
        out[prec] = res
        ctx.close()
    if out_path:
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
