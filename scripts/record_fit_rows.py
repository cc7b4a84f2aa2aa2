#!/usr/bin/env python
"""Record the rows of the fit kernels for seeded sets of stamps, in mixed and f64 mode, on the GPU of this machine.

--set circular (the default): the 16-column rows of the circular Moffat fit (k_fit) for tests/fit_bits_cases.py,
standalone (double stamps) and inside a reconstruct (float and double stamps), into tests/golden/fit_rows_gfx950.npz.
--set models: the rows of fit_stamps_elliptical, fit_stamps_observed, fit_stamps_psf and fit_groups_psf in all their
variants for tests/fit_models_cases.py, into tests/golden/fit_rows_models_gfx950.npz.
--set spec: the rows of fit_spectra_psf (k_fit_spec), head and layers side by side, for tests/fit_spec_cases.py, into
tests/golden/fit_rows_spec_gfx950.npz.  Both modes run the fp64 kernel: the record holds one array per variant, the
two modes must agree to be recorded, and --compare holds each of them to it.

    python scripts/record_fit_rows.py [--set models|spec] [--out FILE]
    python scripts/record_fit_rows.py [--set models|spec] --compare [FILE]

Run it on the build whose bits are to be kept -- before a change to a fit kernel that must not move any -- and commit
the file; tests/test_gpu_fit_bits.py, tests/test_gpu_fit_models_bits.py and tests/test_gpu_fit_spec_bits.py then hold
every later build to it with np.array_equal.  --compare prints, per key, how many rows of the loaded library differ from a record, and exits 1 if
any does.  MPSFR_LIB_PATH selects another build of the library (muse_psfr_amd._build.build_library(out=...) makes one
with the same flags).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import fit_bits_cases as C     # noqa: E402
import fit_models_cases as M   # noqa: E402
import fit_spec_cases as S     # noqa: E402

STATUS_COLUMN = {'rows': 14, 'call': 14, 'ell': 18, 'obs': 18, 'psf': 10, 'grp': 4, 'spec': 10}
ITER_COLUMN = {'rows': 7, 'call': 7, 'ell': 10, 'obs': 10, 'psf': 5, 'grp': 3, 'spec': 9}


def same(a, b):
    """per row: every column equal, NaN equal to NaN"""
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all(axis=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--set', choices=('circular', 'models', 'spec'), default='circular')
    ap.add_argument('--out', default=None)
    ap.add_argument('--compare', nargs='?', const='', default=None)
    args = ap.parse_args()
    import muse_psfr_amd as api
    from muse_psfr_amd import _lib
    import torch
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]
    if args.set == 'circular':
        default, rows = C.RECORD, C.record(api)
        st = C.stamps()
        meta = dict(stamps_sha256=np.array(C.digest(st)), names=np.array([n for n, _ in C.cases()]), call_lbda=C.CALL_LBDA,
                    call_seeing=C.CALL_SEEING, call_gl=C.CALL_GL, call_l0=C.CALL_L0)
        digests = {'stamps_sha256': C.digest(st)}
    else:
        cases = M if args.set == 'models' else S
        default, rows = cases.RECORD, (M.record(api) if cases is M else S.record(api, 'f64'))
        digests = cases.digests()
        meta = {k: np.array(v) for k, v in digests.items()}
        meta.update({k: np.array(v) for k, v in cases.names().items()})
    # what is held to the record: (key of the record, label, rows); the spec set again in the mixed mode
    held = [(k, k, rows[k]) for k in sorted(rows)]
    if args.set == 'spec':
        held += [(k, k + ' [mixed]', v) for k, v in sorted(S.record(api, 'mixed').items())]
    if args.compare is not None:
        ref = np.load(args.compare or default)
        for k, v in digests.items():
            assert str(ref[k]) == v, 'the stamps differ from those of the record (%s)' % k
        bad = 0
        for k, label, a in held:
            b = ref[k]
            d = int((~same(a, b)).sum()) if a.shape == b.shape else -1
            print('%-28s %4d rows, %d differ' % (label, len(a), d))
            bad += d != 0
        print('library %s: %s' % (_lib.LIB_PATH, 'DIFFERS' if bad else 'bit-identical'))
        return 1 if bad else 0
    for k, label, v in held:
        assert same(v, rows[k]).all(), 'the modes differ (%s)' % label
    out = args.out or default
    np.savez_compressed(out, arch=np.array(arch), **meta, **rows)
    print('%s: %d arrays, %d rows, %d bytes' % (out, len(rows), sum(len(r) for r in rows.values()), os.path.getsize(out)))
    for k in sorted(rows):
        r, kind = rows[k], k.split('_')[0]
        print('%-28s %4d rows; status %s; iterations %g..%g' % (k, len(r), sorted(set(r[:, STATUS_COLUMN[kind]].astype(int))),
                                                              r[:, ITER_COLUMN[kind]].min(), r[:, ITER_COLUMN[kind]].max()))
    return 0


if __name__ == '__main__':
    sys.exit(main())
