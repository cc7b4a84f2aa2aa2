#!/usr/bin/env python
"""Record the 16-column rows of the circular Moffat fit (k_fit) for the seeded set of tests/fit_bits_cases.py, in mixed
and f64 mode, standalone (double stamps) and inside a reconstruct (float and double stamps), on the GPU of this
machine:

    python scripts/record_fit_rows.py [--out tests/golden/fit_rows_gfx950.npz]
    python scripts/record_fit_rows.py --compare tests/golden/fit_rows_gfx950.npz

Run it on the build whose bits are to be kept -- before a change to k_fit that must not move any -- and commit the
file; tests/test_gpu_fit_bits.py then holds every later build to it with np.array_equal.  --compare prints, per
key, how many rows of the loaded library differ from a record, and exits 1 if any does.  MPSFR_LIB_PATH selects
another build of the library.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import fit_bits_cases as C     # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=C.RECORD)
    ap.add_argument('--compare', default=None)
    args = ap.parse_args()
    import muse_psfr_amd as api
    from muse_psfr_amd import _lib
    import torch
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]
    rows = C.record(api)
    st = C.stamps()
    if args.compare:
        ref = np.load(args.compare)
        assert str(ref['stamps_sha256']) == C.digest(st), 'the stamps differ from those of the record'
        bad = 0
        for k in sorted(rows):
            a, b = rows[k], ref[k]
            d = int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=1).sum()) if a.shape == b.shape else -1
            print('%-28s %4d rows, %d differ' % (k, len(a), d))
            bad += d != 0
        print('library %s: %s' % (_lib.LIB_PATH, 'DIFFERS' if bad else 'bit-identical'))
        return 1 if bad else 0
    names = np.array([n for n, _ in C.cases()])
    np.savez_compressed(args.out, stamps_sha256=np.array(C.digest(st)), names=names, arch=np.array(arch),
                        call_lbda=C.CALL_LBDA, call_seeing=C.CALL_SEEING, call_gl=C.CALL_GL, call_l0=C.CALL_L0, **rows)
    print('%s: %d stamps, %d arrays, %d bytes' % (args.out, len(st), len(rows), os.path.getsize(args.out)))
    for k in sorted(rows):
        r = rows[k]
        print('%-28s %4d rows; status %s; iterations %g..%g' % (k, len(r), sorted(set(r[:, 14].astype(int))), r[:, 7].min(),
                                                              r[:, 7].max()))
    return 0


if __name__ == '__main__':
    sys.exit(main())
