#!/usr/bin/env python
"""Record the final stamps of the convolution stage for a seeded set of inputs, in mixed and f64 mode, on the GPU of this machine.

Context.convolve_stamps (k_khat + k_conv_fft) on the eight stamps of tests/conv_bits_cases.py -- two tasks, two wavelengths,
a Moffat-like and a "hard" input class -- into tests/golden/conv_stamps_gfx950.npz: the mixed outputs as float32 (they are
float values; checked), the f64 outputs as float64, both as byte planes (conv_bits_cases.planes), with the SHA-256 of the
inputs, the architecture and the parameters.

    python scripts/record_conv_stamps.py [--out FILE]
    python scripts/record_conv_stamps.py --compare [FILE]

Run it on the build whose bits are to be kept -- before a change to k_conv_fft or the line transforms that must not move
any -- and commit the file; tests/test_gpu_conv_bits.py then holds every later build to it with np.array_equal.
--compare prints, per mode, how many elements of the loaded library's outputs differ from a record, and exits 1 if any
does.  MPSFR_LIB_PATH selects another build of the library (muse_psfr_amd._build.build_library(out=...) makes one with
the same flags).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import conv_bits_cases as C     # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--compare', nargs='?', const='', default=None)
    args = ap.parse_args()
    import muse_psfr_amd as api
    from muse_psfr_amd import _lib
    import torch
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]
    pre, par = C.inputs()
    got = C.record(api)
    if args.compare is not None:
        ref = np.load(args.compare or C.RECORD)
        assert str(ref['inputs_sha256']) == C.digest(pre), 'the inputs differ from those of the record'
        bad = 0
        for prec in C.MODES:
            a, b = got['out_%s' % prec], C.values(ref['out_%s' % prec], prec, pre.shape).astype(np.float64)
            d = int((a != b).sum())
            print('%-10s %6d elements, %d differ' % ('out_' + prec, a.size, d))
            bad += d != 0
        print('library %s: %s' % (_lib.LIB_PATH, 'DIFFERS' if bad else 'bit-identical'))
        return 1 if bad else 0
    rec = {}
    for prec in C.MODES:
        a = got['out_%s' % prec]
        assert np.all(np.isfinite(a))
        rec['out_%s' % prec] = C.planes(a, prec)
        assert np.array_equal(C.values(rec['out_%s' % prec], prec, a.shape).astype(np.float64), a), (
            'the %s outputs are not %s values' % (prec, C.DTYPE[prec].__name__))
    out = args.out or C.RECORD
    np.savez_compressed(out, arch=np.array(arch), inputs_sha256=np.array(C.digest(pre)), dim=np.array(C.DIM),
                        grid=np.array(C.GRID), shape=np.array(pre.shape), lbda=C.LBDA, tasks=C.TASKS, classes=np.array(C.CLASSES),
                        seed=np.array(C.SEED), **rec)
    print('%s: %d stamps per mode, %d bytes' % (out, pre.shape[0] * pre.shape[1], os.path.getsize(out)))
    for prec in C.MODES:
        a = got['out_%s' % prec]
        print('out_%-6s peaks %s' % (prec, np.array2string(a.max(axis=(-1, -2)).ravel(), precision=4)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
