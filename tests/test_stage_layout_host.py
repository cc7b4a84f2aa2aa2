"""The staging-buffer layout of the stamp, frame and cube calls (muse_psfr_amd/csrc/stage_layout.h), checked on the CPU.

tests/stage_layout_check.cpp includes nothing of the project but that header.  It declares the arrays of every call of
stamp_calls.cpp at small counts, with every subset of the optional arrays absent, and compares offsets and totals with
the rule of DESIGN.md ("The entry layer") restated on its own; it also checks alignment and that no two arrays overlap.
Built with the address and undefined-behaviour sanitizers and run directly."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# call -> optional arrays among those it stages (mpsfr_fit_cube_psf: the host form's per-call and per-batch arrays)
OPTIONALS = {
    'fit_stamps': 0,
    'fit_stamps_elliptical': 0,
    'fit_stamps_observed': 1,        # var
    'fit_stamps_psf': 3,             # var, shift, psf_index
    'fit_groups_psf': 2,             # var, psf_index
    'fit_spectra_psf': 3,            # var, shift, psf_index
    'stamp_metrics': 1,              # centers
    'cut_stamps': 2,                 # var, var_out
    'render_stars': 4,               # image_in, shift, psf_index, star_out
    'find_stars': 3,                 # var, map_out, origin_out
    'frame_background': 5,           # var, apply_to, map_out, rms_out, applied_out
    'group_stars': 2,                # shift_out, origin_out
    'fit_frame_psf': 5,              # var, shift, scale0, psf_index, resid_out
    'fit_frame_psf_free': 5,
    'fit_cube_psf': 6,               # shift, layer_shift, psf_index, var, scale0, resid_out
    'fit_cube_psf_free': 6,
}
NSIZES = 2      # the sets of counts the program walks: (nstar, nl, nb) = (1, 1, 1) and (3, 3, 2) on a 5 x 7 frame


def test_stage_layout_follows_the_documented_rule(tmp_path):
    cxx = shutil.which('c++') or '/opt/rocm/llvm/bin/clang++'
    assert os.path.exists(cxx), 'no host C++ compiler (c++ or /opt/rocm/llvm/bin/clang++)'
    exe = str(tmp_path / 'stage_layout_check')
    # the sanitizer runtimes inside the binary (clang's default), so that it needs nothing loaded ahead of it
    version = subprocess.run([cxx, '--version'], capture_output=True, text=True, check=True).stdout
    static = [] if 'clang' in version else ['-static-libasan', '-static-libubsan']
    subprocess.run([cxx, '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', *static, '-g',
                    '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'muse_psfr_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'stage_layout_check.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    walked = {}
    total = None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == 'call':
            walked[w[1]] = (int(w[2]), int(w[3]))
        elif w[0] == 'cases':
            total = (int(w[1]), int(w[3]), int(w[5]))
    want = {name: (NSIZES << nopt, NSIZES * ((1 << nopt) - 1)) for name, nopt in OPTIONALS.items()}
    assert walked == want
    assert total == (sum(a for a, _ in want.values()), sum(b for _, b in want.values()), 0)
