#!/usr/bin/env python
"""Record the outputs of the pipeline calls of tests/reconstruct_bits_cases.py, on the GPU of this machine.

mpsfr_reconstruct, _field, _band, _profile, mpsfr_simul_psd, _simul_psd_profile, mpsfr_psf_from_psd and
mpsfr_convolve_stamps under the options, output forms and call sequences of the cases, into
tests/golden/reconstruct_calls_gfx950.npz: every array in full (the fits, the band sums), above 4096 values as the SHA-256
of its bytes (stamps, PSD images, stamp sums), with the SHA-256 of the inputs, the architecture, debug_fetch('d0t_clears') of the sequences and, from a
second run under the `profile` option, the timed scopes per kernel id.  Every case runs twice, on fresh contexts; an
array whose two runs differ is named and left out of the record (none is expected).  The record is valid only if no
`psf` and no `fit` array is left out: otherwise nothing is written and the exit code is 2.

    python scripts/record_reconstruct_calls.py [--out FILE]
    python scripts/record_reconstruct_calls.py --compare [FILE]

Run it on the build whose bits are to be kept -- before a change to the host path of mpsfr_api.cpp that must not move
any -- and commit the file; tests/test_gpu_reconstruct_bits.py then holds every later build to it.  --compare prints the
arrays of the loaded library's outputs that differ from a record, per precision mode, and exits 1 if any does.
MPSFR_LIB_PATH selects another build of the library (muse_psfr_amd._build.build_library(out=...) makes one with the same
flags).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import reconstruct_bits_cases as C     # noqa: E402


def run_all(api):
    out = {}
    for name in C.cases():
        out.update(C.record(api, name))
        out.update(C.record(api, name, profile=True))
    return out


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
        meta = ('arch', 'inputs_sha256', 'hash_above')
        got = run_all(api)
        bad = 0
        for prec in ('mixed', 'f64'):
            keys = [k for k in ref.files if k not in meta and C.cases()[case_of(k)][1] == prec]
            differ = [k for k in keys if k not in got or not C.same(k, got[k], ref[k])]
            print('%-6s %3d arrays, %d differ%s' % (prec, len(keys), len(differ), ': ' + ', '.join(differ) if differ else ''))
            bad += len(differ)
        loose = [a for a, b in C.held_to_fresh(sorted(got)) if not np.array_equal(C.bits(got[a]), C.bits(got[b]))]
        print('calls of a sequence that differ from the call on a fresh context: %s' % (', '.join(loose) or 'none'))
        bad += len(loose)
        print('library %s: %s' % (_lib.LIB_PATH, 'DIFFERS' if bad else 'bit-identical'))
        return 1 if bad else 0
    runs = [run_all(api) for _ in range(2)]
    rec, unstable = {}, []
    for k, a in runs[0].items():
        if np.array_equal(C.bits(a), C.bits(runs[1][k])):
            rec[k] = C.stored(k, a)
        else:
            unstable.append(k)
    loose = [a for a, b in C.held_to_fresh(sorted(runs[0])) if not np.array_equal(C.bits(runs[0][a]), C.bits(runs[0][b]))]
    print('arrays that differ between the two runs: %s' % (', '.join(unstable) or 'none'))
    print('calls of a sequence that differ from the call on a fresh context: %s' % (', '.join(loose) or 'none'))
    if any(k.rsplit('.', 1)[-1] in ('psf', 'fit') for k in unstable) or loose:
        print('no record written: a psf or fit array does not repeat')
        return 2
    out = args.out or C.RECORD
    np.savez_compressed(out, arch=np.array(arch), inputs_sha256=np.array(sha), hash_above=np.array(C.HASH_ABOVE), **rec)
    hashed = sum(1 for k, a in runs[0].items() if k in rec and rec[k].shape != np.shape(a))
    print('%s: %d arrays (%d of them kept as SHA-256), %d bytes' % (out, len(rec), hashed, os.path.getsize(out)))
    return 0


def case_of(key):
    """the case a record key belongs to: the longest case name that is a prefix of it"""
    return max((n for n in C.cases() if key.startswith(n + '.')), key=len)


if __name__ == '__main__':
    sys.exit(main())
