"""psd_to_psf (psfrec.py:689-807) without a GPU: the host helpers against the reference's values (g8),
the refusals made in Python before any context exists, and the C entry point's argument check."""
import os

import numpy as np
import pytest

from conftest import ROOT


def test_exports_and_helpers_equal_the_reference(golden):
    from muse_psfr_amd import crop, interpolate, psd_to_psf, pupil_mask, seeing2r01  # noqa: F401
    g = golden('g8_psd_to_psf')
    for i in range(4):
        radius, width, oc = g['pupil_mask_args%d' % i]
        width = int(width) if i < 3 else width          # psf_muse passes dim / 2, a float
        m = pupil_mask(radius, width, oc=oc, inverse=bool(g['pupil_mask_inv%d' % i]))
        assert m.dtype.kind == 'i'
        np.testing.assert_array_equal(m, g['pupil_mask%d' % i])
    np.testing.assert_array_equal(crop(g['arr'], 12, 5), g['crop_out'])
    np.testing.assert_allclose(interpolate(g['arr'], g['interp_pos']), g['interp_out'], rtol=1e-14, atol=0)
    np.testing.assert_allclose(interpolate(g['arr'], g['interp_pts'], method='linear'), g['interp_pts_out'],
                               rtol=1e-14, atol=0)
    for (lb, z), want in zip(g['s2r_args'], g['s2r_out']):
        np.testing.assert_allclose(seeing2r01(g['s2r_seeing'], lb, z), want, rtol=1e-14, atol=0)


def test_interpolate_refusals():
    from muse_psfr_amd import interpolate
    a = np.ones((8, 8))
    with pytest.raises(NotImplementedError, match='FIXME'):
        interpolate(a, np.mgrid[:4, :4], method='cubic')
    with pytest.raises(ValueError, match='out of bounds'):
        interpolate(a, np.mgrid[:4, :4] * 3.0)
    with pytest.raises(ValueError, match='out of bounds'):
        interpolate(a, -0.5 + np.mgrid[:4, :4])


@pytest.fixture
def no_context(monkeypatch):
    """Any attempt to create a GPU context fails the test: the refusals must come first."""
    from muse_psfr_amd import psfrec

    def boom(*a, **k):
        raise AssertionError('a context was requested')
    monkeypatch.setattr(psfrec, 'get_context', boom)
    monkeypatch.setattr(psfrec, 'Context', boom)


def test_refusals_are_made_before_any_context(no_context):
    from muse_psfr_amd import psd_to_psf, pupil_mask
    psd = np.ones((256, 256))
    pup = pupil_mask(64, 128, oc=0.14)
    lb = 500e-9
    fovnum = (lb / (2 * 8.0)) * 256 / (4.85e-6)
    with pytest.raises(NotImplementedError):
        psd_to_psf(psd, pup, 8.0, lb, samp=2, FoV=1.5 * fovnum)
    with pytest.raises(NotImplementedError):
        psd_to_psf(psd, pup, 8.0, np.array([lb, 2 * lb]), samp=2, FoV=fovnum)
    with pytest.raises(ValueError, match='samp'):
        psd_to_psf(psd, pup, 8.0, lb, samp=3)
    with pytest.raises(ValueError, match='phase_static'):
        psd_to_psf(psd, pup, 8.0, lb, phase_static=np.zeros((64, 64)))
    with pytest.raises(ValueError, match='grid'):
        psd_to_psf(np.zeros((200, 200)), pupil_mask(50, 100), 8.0, lb)
    with pytest.raises(ValueError, match='dimnum'):
        psd_to_psf(psd, pup, 8.0, lb, samp=1.5)                 # dimnum = 192
    with pytest.raises(ValueError, match='dimnum'):
        psd_to_psf(np.zeros((512, 512)), pupil_mask(150, 300), 8.0, lb, samp=1.0)   # dimnum 300


def test_refusal_logs_the_reference_messages(no_context, caplog):
    import logging
    from muse_psfr_amd import psd_to_psf, pupil_mask
    pup = pupil_mask(100, 200)
    with caplog.at_level(logging.INFO, logger='muse_psfr_amd.psfrec'):
        with pytest.raises(ValueError):
            psd_to_psf(np.zeros((256, 256)), pup, 8.0, 5e-7, samp=1.0, phase_static=np.zeros((3, 3)))
    msgs = [r.getMessage() for r in caplog.records]
    assert any('PSD horizon must be at least two time larger' in m for m in msgs)
    assert any('PSF should be at least nyquist sampled' in m for m in msgs)
    assert any('pup and static phase must have the same number of pixels' in m for m in msgs)


def test_c_entry_point_refuses_a_null_context(tmp_path):
    """mpsfr_psd_to_psf is declared in the plain-C header and refuses a NULL context with MPSFR_E_INVALID
    and a message, without a GPU."""
    import shutil
    import subprocess
    from muse_psfr_amd._build import build_library
    lib = build_library(force=False, verbose=False)
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    src = tmp_path / 'p2p_c.c'
    src.write_text(
        '#include "mpsfr.h"\n'
        '#include <stdio.h>\n'
        'int main(void) {\n'
        '    double psd[4] = {0}, pup[1] = {1}, lb[1] = {5e-7}, out[4];\n'
        '    int rc = mpsfr_psd_to_psf(NULL, 1, psd, 1, pup, NULL, 8.0, 1, lb, 128, out, 0);\n'
        '    printf("rc=%d msg=%s\\n", rc, mpsfr_last_error());\n'
        '    return rc == MPSFR_E_INVALID && mpsfr_last_error()[0] ? 0 : 1;\n'
        '}\n')
    exe = tmp_path / 'p2p_c'
    libdir = os.path.dirname(lib)
    subprocess.run([gcc, '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    str(src), '-L', libdir, '-lmpsfr', '-Wl,-rpath,' + libdir, '-o', str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert 'ctx is NULL' in r.stdout
