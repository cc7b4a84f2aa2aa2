"""GPU: `bench.py --dump-outputs DIR` writes what its timed steps computed -- the fit table and the stamp sum of
the last timed step, the same as one call of the library on the bench's inputs -- and a second run with the same
arguments writes the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import H, ROOT

pytestmark = pytest.mark.gpu

ROWS, NL, DIM, STEPS = 12, 5, 128, 5
ARGS = ['--steps', str(STEPS), '--warmup', '1', '--prime', '4', '--rows', str(ROWS), '--dim', str(DIM),
        '--nl', str(NL), '--cpu-rows', '0', '--f64-steps', '0', '--unpruned-steps', '0', '--host-steps', '0',
        '--e2e-steps', '0', '--native-steps', '0', '--profile-steps', '0', '--min-seconds', '0']


def _bench(out):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + ARGS + ['--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_dumps_what_its_timed_steps_computed(tmp_path):
    import muse_psfr_amd as api
    out = _bench(tmp_path / 'a')
    assert out['steps'] == STEPS and out['ms_per_step'] > 0
    assert sorted(os.listdir(tmp_path / 'a')) == ['fit.npy', 'psf_sum.npy']
    fit, psum = np.load(tmp_path / 'a' / 'fit.npy'), np.load(tmp_path / 'a' / 'psf_sum.npy')
    assert fit.dtype == np.float64 and fit.shape == (ROWS, NL, api.NFIT)
    assert psum.dtype == np.float64 and psum.shape == (NL, 40, 40)
    see, gl, l0 = api.synthetic_rows(ROWS)
    ctx = api.Context(dim=DIM, pixscale=api.grid_pixscale(DIM), precision='mixed')
    r = ctx.reconstruct(np.linspace(465.0, 930.0, NL), see, gl, l0, np.zeros(ROWS, np.uint8), H, 12.0, 1,
                        want_psf=False)
    ctx.close()
    np.testing.assert_array_equal(fit, r['fit'])
    np.testing.assert_allclose(psum, r['psf_sum'], rtol=1e-13)
    _bench(tmp_path / 'b')
    for name in ('fit', 'psf_sum'):
        np.testing.assert_array_equal(np.load(tmp_path / 'b' / (name + '.npy')),
                                      np.load(tmp_path / 'a' / (name + '.npy')))
