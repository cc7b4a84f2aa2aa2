#!/usr/bin/env python
"""Record the outputs of the crowded-field fits for the cases of tests/crowded_bits_cases.py, on the GPU of this machine.

mpsfr_fit_frame_psf, mpsfr_fit_frame_psf_free, mpsfr_fit_cube_psf and mpsfr_fit_cube_psf_free, host form, a mixed
context (the calls are fp64 in both modes), into tests/golden/crowded_calls_gfx950.npz: every output array, those of
more than 4096 values as the SHA-256 of their bytes, with the SHA-256 of the inputs and the architecture.  Every call
runs twice, on two contexts.  No array may be left out: one whose two runs differ is named and the script writes no
record and exits 1 (none is expected: no sum of these calls depends on the scheduling).

    python scripts/record_crowded_calls.py [--out FILE]
    python scripts/record_crowded_calls.py --compare [FILE]

Run it on the build whose bits are to be kept -- before a change to frame_fit_impl.h, frame_free_impl.h, frame_free.hip,
cube_free.hip or what they share that must not move any -- and commit the file; tests/test_gpu_crowded_bits.py then
holds every later build to it.  --compare prints the arrays of the loaded library's outputs that differ from a record,
in both precision modes and through device pointers, and exits 1 if any does.  MPSFR_LIB_PATH selects another build of
the library (muse_psfr_amd._build.build_library(out=...) makes one with the same flags).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import crowded_bits_cases as C     # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--compare', nargs='?', const='', default=None)
    args = ap.parse_args()
    import muse_psfr_amd as api
    from muse_psfr_amd import _lib
    import torch
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]
    sha = C.digest(C.inputs())
    if args.compare is not None:
        ref = np.load(args.compare or C.RECORD)
        assert str(ref['inputs_sha256']) == sha, 'the inputs differ from those of the record'
        names = [k for k in ref.files if k.split('.')[0] in C.CALLS]
        bad = 0
        for prec in C.MODES:
            ctx = C.context(api, prec)
            for form, got in (('host', C.record(ctx)), ('device', C.record_device(ctx))):
                keys = names if form == 'host' else sorted(got)
                differ = [k for k in keys if k not in got or not C.equal(k, got[k], ref[k])]
                print('%-6s %-6s %3d arrays, %d differ%s' % (prec, form, len(keys), len(differ),
                                                             ': ' + ', '.join(differ) if differ else ''), flush=True)
                bad += len(differ)
            ctx.close()
        print('library %s: %s' % (_lib.LIB_PATH, 'DIFFERS' if bad else 'bit-identical'))
        return 1 if bad else 0
    runs = []
    for _ in range(2):
        ctx = C.context(api, 'mixed')
        runs.append(C.record(ctx))
        ctx.close()
    unstable = [k for k, a in runs[0].items() if not np.array_equal(C.bits(a), C.bits(runs[1][k]))]
    print('arrays that differ between the two runs: %s' % (', '.join(unstable) or 'none'))
    if unstable:
        print('no record written: every array has to be in it')
        return 1
    rec = {k: C.kept(k, a) for k, a in runs[0].items()}
    out = args.out or C.RECORD
    np.savez_compressed(out, arch=np.array(arch), inputs_sha256=np.array(sha), hash_above=np.array(C.HASH_ABOVE), **rec)
    hashed = sum(1 for k, a in runs[0].items() if rec[k].shape != np.shape(a))
    print('%s: %d arrays (%d of them kept as SHA-256), %d bytes' % (out, len(rec), hashed, os.path.getsize(out)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
