"""Compare the device ISA of the legacy stage-A kernels between a git revision and the working tree.

    python tools/isa_legacy_diff.py [REV] [--files F,..] [--kernels REGEX]      (default REV: HEAD)

Compiles stage_a.hip and stage_a2.hip of both trees to gfx950 assembly with the flags of _build.py and compares
k_ao_tables, k_psd_rowfft, k_psd_image and k_patch_gen as a legacy call instantiates them (profile instantiations,
*_profile kernels, are skipped).  Kernels that became variadic templates (k_psd_rowfft<N, F64, Mix...> with an
empty pack) have another mangled name: the names, label numbers and comments are normalised away, so what is
compared is the instructions and the kernel descriptor.  Exit status 1 if any kernel differs.

--files / --kernels select other translation units of muse_psfr_amd/csrc and other kernels, e.g.
    python tools/isa_legacy_diff.py --files stamps --kernels 'k_fit<'
for the circular Moffat fit after its device helpers moved into fit_common.h.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from muse_psfr_amd._build import FLAGS, _hipcc  # noqa: E402

KERNELS = re.compile(r'(k_ao_tables|k_psd_rowfft|k_psd_image|k_patch_gen)')


def compile_tree(src, out, files):
    for f in files:
        subprocess.check_call([_hipcc()] + FLAGS + ['--cuda-device-only', '-S', '-x', 'hip',
                                                    os.path.join(src, 'muse_psfr_amd', 'csrc', f + '.hip'),
                                                    '-o', os.path.join(out, f + '.s')], stderr=subprocess.DEVNULL)


def legacy_name(sym):
    """The mangled name a kernel had before its Mix... pack: an empty pack 'JE' and the trailing 'DpT<k>_' dropped."""
    return re.sub(r'DpT\d_$', '', re.sub(r'JE(?=E)', '', sym))


def kernels(path, pattern=KERNELS):
    text = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', text, re.S | re.M):
        sym, body = m.group(1), m.group(2)
        name = subprocess.run(['c++filt', sym], capture_output=True, text=True).stdout
        if not pattern.search(name) or '_profile' in name or 'double const*, int' in name:
            continue
        d = re.search(r'\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel' % re.escape(sym), text, re.S)
        s = body + '\n--descriptor--\n' + (d.group(1) if d else '')
        s = re.sub(r'BB\d+_', 'BB_', s).replace(sym, 'KERNEL')
        s = '\n'.join(re.sub(r'\s+', ' ', ln.split(';')[0]).strip() for ln in s.split('\n'))
        out[legacy_name(sym)] = (name.strip(), s)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('rev', nargs='?', default='HEAD')
    ap.add_argument('--files', default='stage_a,stage_a2', help='translation units (csrc/<name>.hip), comma-separated')
    ap.add_argument('--kernels', default=KERNELS.pattern, help='regular expression on the demangled kernel names')
    args = ap.parse_args()
    rev, files, pattern = args.rev, args.files.split(','), re.compile(args.kernels)
    with tempfile.TemporaryDirectory() as tmp:
        old_src, old_s, new_s = (os.path.join(tmp, d) for d in ('src', 'old', 'new'))
        for d in (old_src, old_s, new_s):
            os.makedirs(d)
        arch = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'muse_psfr_amd/csrc', 'include'],
                              capture_output=True, check=True).stdout
        subprocess.run(['tar', '-x', '-C', old_src], input=arch, check=True)
        compile_tree(old_src, old_s, files)
        compile_tree(ROOT, new_s, files)
        bad = 0
        for f in files:
            a, b = kernels(os.path.join(old_s, f + '.s'), pattern), kernels(os.path.join(new_s, f + '.s'), pattern)
            for sym in sorted(a):
                same = sym in b and a[sym][1] == b[sym][1]
                bad += not same
                print('%-8s %s' % ('same' if same else 'DIFFERS', a[sym][0]))
        print('%d legacy kernel(s) differ' % bad)
        return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
