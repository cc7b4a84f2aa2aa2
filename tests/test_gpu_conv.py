"""GPU: the convolution stage alone (K_KHAT / K_MOFFAT_KERNELS, K_CONV_FFT / K_CONV) through
Context.convolve_stamps, on stamps the atmosphere model never produces, against the fp64 reference of
tests/tail_ref.py (scipy.signal.fftconvolve 'same', the call the reference itself makes).

Contexts: mixed (FFT form), mixed with "fft_conv" 0 (direct form) and f64, at the pixel scales 0.2 and
grid_pixscale(512): the kernels are 2.6 times wider in pixels at the second.  `dim` does not enter this stage.

Tolerances are the project's own for final stamps (tests/test_gpu_parity.py): 2e-5 (mixed) and 1e-9 (f64) of the
peak of the EXPECTED output stamp, per stamp.  Every case is compared; none is skipped.

No input class needed a bound of its own: the hardest one, the +-1 checkerboard (all its energy at the Nyquist
frequency of both axes, where the kernel spectra are 1e-3 or less, so that the expected output is only what the
stamp's edges leave, 8e-3 of the input's amplitude at the finer pixel scale, while the fp32 rounding of the
transforms scales with the input) measured 1.3e-5 in the FFT form; every other class stays below 5e-7 (mixed) and
8e-11 (f64).  The worst value per class goes to the margins file under 'conv_alone'.
"""
import numpy as np
import pytest

import tail_ref as T
from conftest import record_margin

pytestmark = pytest.mark.gpu

TOL = {'mixed': 2e-5, 'f64': 1e-9}
CONTEXTS = [('mixed', 1), ('mixed', 0), ('f64', 1)]
LB = np.array([465.0, 700.0, 930.0])
# two tasks whose tip-tilt kernels differ by a factor of six in width (gamma 0.13 / 0.78 px at 0.2 arcsec/px)
TASKS = np.array([(0.6, 0.9, 25.0), (2.0, 0.1, 10.0)])
_cache = {}


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _pixscales(api):
    return (0.2, api.grid_pixscale(512))


def _ctx(api, prec, fft, ps):
    ctx = api.Context(dim=128, pixscale=ps, precision=prec)
    if not fft:
        ctx.set_option('fft_conv', 0)
    return ctx


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _errors(got, want):
    """max |got - want| over each stamp, relative to the peak (largest modulus) of the expected stamp"""
    assert got.shape == want.shape
    return np.abs(got - want).max(axis=(-1, -2)) / np.abs(want).max(axis=(-1, -2))


def impulse_positions():
    edge = (0, 1, 19, 20, 38, 39)
    pos = {(a, b) for a in edge for b in range(40)} | {(a, b) for a in range(40) for b in edge}
    rest = [(a, b) for a in range(40) for b in range(40) if (a, b) not in pos]
    rng = np.random.default_rng(40)
    pick = rng.choice(len(rest), 200, replace=False)
    pos = sorted(pos) + [rest[k] for k in sorted(pick)]
    assert len(pos) == 444 + 200 and all(c in pos for c in ((0, 0), (0, 39), (39, 0), (39, 39)))
    return pos


@pytest.mark.parametrize('prec,fft', CONTEXTS)
def test_impulse_responses_at_every_edge_position(api, prec, fft):
    """A single 1 at (a, b): the four corners, every position of rows and columns 0, 1, 19, 20, 38, 39 and a seeded
    random 200 of the rest, each through both tasks' tip-tilt kernels and all three wavelengths' instrument kernels
    in ONE call (task 2 i + j is position i with the parameters of TASKS[j]): by linearity these reach every input
    index path -- both rows of a row pair, the crop between the two convolutions, the un-aliased window [20, 60) of
    the 64-long circular convolution -- and a mix-up of the task / wavelength index of the kernel spectra shows."""
    pos = impulse_positions()
    pre = np.zeros((2 * len(pos), LB.size, 40, 40))
    for i, (a, b) in enumerate(pos):
        pre[2 * i:2 * i + 2, :, a, b] = 1.0
    par = np.tile(TASKS, (len(pos), 1))
    for ps in _pixscales(api):
        want = _cached(('impulse', ps), lambda: T.final_stamps(LB, par[:, 0], par[:, 1], par[:, 2], pre, ps))
        ctx = _ctx(api, prec, fft, ps)
        got = ctx.convolve_stamps(LB, par[:, 0], par[:, 1], par[:, 2], pre)
        ctx.close()
        err = _errors(got, want)
        worst = np.unravel_index(err.argmax(), err.shape)
        print('impulse %s fft=%d ps=%.4f: worst %.3e at position %s task %d wavelength %d' %
              (prec, fft, ps, err.max(), pos[worst[0] // 2], worst[0] % 2, worst[1]))
        record_margin('conv_alone', **{'impulse_%s_fft%d' % (prec, fft): err.max()})
        assert np.all(np.isfinite(got))
        assert err.max() < TOL[prec], (ps, pos[worst[0] // 2], worst, err.max())


def structured_stamps():
    rng = np.random.default_rng(41)
    noise = rng.random((40, 40))
    i, j = np.indices((40, 40))
    ring = np.ones((40, 40))
    ring[1:-1, 1:-1] = 0.0
    return [('noise', noise), ('checkerboard', np.where((i + j) % 2 == 0, 1.0, -1.0)), ('ring', ring),
            ('constant', np.ones((40, 40))), ('negative', noise - 0.75), ('peak_1e6', 1e6 * noise),
            ('peak_1e-6', 1e-6 * noise)]


@pytest.mark.parametrize('prec,fft', CONTEXTS)
def test_stamps_with_structure_at_the_edge(api, prec, fft):
    """Uniform noise, a +-1 checkerboard (all energy in the packed DC / Nyquist column), the outermost ring of
    pixels, a constant (expected: the kernels' partial sums, falling off towards the zero padding), a stamp with
    negative values, peaks of 1e6 and 1e-6; each class through both tasks and the three wavelengths in one call."""
    classes = structured_stamps()
    pre = np.array([np.broadcast_to(s, (LB.size, 40, 40)) for _, s in classes for _ in range(2)])
    par = np.tile(TASKS, (len(classes), 1))
    bad = []
    for ps in _pixscales(api):
        want = _cached(('structured', ps), lambda: T.final_stamps(LB, par[:, 0], par[:, 1], par[:, 2], pre, ps))
        ctx = _ctx(api, prec, fft, ps)
        got = ctx.convolve_stamps(LB, par[:, 0], par[:, 1], par[:, 2], pre)
        ctx.close()
        assert np.all(np.isfinite(got))
        err = _errors(got, want)
        for k, (name, s) in enumerate(classes):
            e = err[2 * k:2 * k + 2]
            print('%s %s fft=%d ps=%.4f: worst %.3e (peak of the expected output %.3e)' %
                  (name, prec, fft, ps, e.max(), np.abs(want[2 * k:2 * k + 2]).max()))
            record_margin('conv_alone', **{'%s_%s_fft%d' % (name, prec, fft): e.max()})
            if not e.max() < TOL[prec]:
                bad.append((name, ps, e.max()))
    assert not bad, bad


@pytest.mark.parametrize('prec,fft', CONTEXTS)
def test_kernel_parameter_range(api, prec, fft):
    """The corners of the SPARTA window (seeing 0.3 / 2.5, GL 0.02 / 0.98, L0 8.1 / 29.9), L0 below and above the
    coeffL0 table (0.5 and 250 m: the np.interp clamp of psfrec.py:897), and the wavelengths 465, 930 and -- outside
    the range the instrument polynomial was fitted on, where the library must extrapolate as the reference does --
    400 and 1000 nm (oracle: FWHM 0.277 / 0.324 arcsec, beta 1.99 / 2.15, both positive)."""
    lb = np.array([400.0, 465.0, 930.0, 1000.0])
    fw, be = T.O.muse_intrinsic_psf(lb)
    assert np.all(fw > 0) and np.all(be > 0)
    par = np.array([(0.3, 0.02, 8.1), (2.5, 0.98, 29.9), (0.3, 0.98, 29.9), (2.5, 0.02, 8.1), (1.0, 0.5, 0.5),
                    (1.0, 0.5, 250.0), (2.5, 0.02, 0.5), (0.3, 0.98, 250.0)])
    rng = np.random.default_rng(42)
    base = T.moffat_stamp(1.0, 19.6, 20.3, 4.0, 2.5)
    pre = np.array([[base + 0.1 * rng.random((40, 40)) for _ in lb] for _ in par])
    for ps in _pixscales(api):
        want = _cached(('range', ps), lambda: T.final_stamps(lb, par[:, 0], par[:, 1], par[:, 2], pre, ps))
        ctx = _ctx(api, prec, fft, ps)
        got = ctx.convolve_stamps(lb, par[:, 0], par[:, 1], par[:, 2], pre)
        ctx.close()
        err = _errors(got, want)
        print('range %s fft=%d ps=%.4f: worst per task %s' % (prec, fft, ps, err.max(axis=1)))
        record_margin('conv_alone', **{'range_%s_fft%d' % (prec, fft): err.max()})
        assert np.all(np.isfinite(got))
        assert err.max() < TOL[prec], (ps, err)


@pytest.mark.parametrize('prec,fft', CONTEXTS)
def test_ground_layer_fraction_one_is_the_identity_tiptilt_kernel(api, prec, fft):
    """GL = 1: the tip-tilt width is 0 and the kernel is the identity, the limit GL -> 1 (the reference's
    Moffat2DKernel(0, 2) is NaN there; the host floors the width at a tiny positive value).  The call equals the reference with the tip-tilt step left out, and the call at GL = 1 - 1e-12."""
    rng = np.random.default_rng(43)
    pre = T.moffat_stamp(1.0, 19.6, 20.3, 4.0, 2.5) + 0.1 * rng.random((LB.size, 40, 40))
    for ps in _pixscales(api):
        want = T.final_stamps(LB, 1.0, 1.0, 20.0, pre, ps, tiptilt=False)
        ctx = _ctx(api, prec, fft, ps)
        one = ctx.convolve_stamps(LB, [1.0], [1.0], [20.0], pre)
        near = ctx.convolve_stamps(LB, [1.0], [1.0 - 1e-12], [20.0], pre)
        ctx.close()
        assert np.all(np.isfinite(one)) and np.all(np.isfinite(near))
        e1, e2, e12 = _errors(one, want).max(), _errors(near, want).max(), _errors(one, near).max()
        print('GL=1 %s fft=%d ps=%.4f: %.3e, GL=1-1e-12: %.3e, between them %.3e' % (prec, fft, ps, e1, e2, e12))
        record_margin('conv_alone', **{'gl_one_%s_fft%d' % (prec, fft): max(e1, e2, e12)})
        assert max(e1, e2, e12) < TOL[prec]


def test_reconstruct_with_ground_layer_fraction_one(api):
    """A 512^2 row with GL = 1 (all turbulence in the ground layer): finite stamps, a status 0 fit."""
    ctx = api.Context(dim=512, pixscale=api.grid_pixscale(512), precision='mixed')
    r = ctx.reconstruct(LB, [1.0, 1.0], [1.0, 0.7], [20.0, 20.0])
    ctx.close()
    assert np.all(np.isfinite(r['psf'])) and np.all(np.isfinite(r['psf_sum'])) and np.all(np.isfinite(r['fit']))
    assert np.all(r['fit'][:, :, 14] == 0)
    assert np.all(r['psf'][0].max(axis=(-1, -2)) > r['psf'][1].max(axis=(-1, -2)))      # no tip-tilt blur: sharper


def test_the_same_spectra_inside_a_call(api):
    """The tip-tilt spectra come from trailing workgroups of K_PATCH_ROWS ("head_fusion" 1), from K_KHAT
    ("head_fusion" 0) or, in convolve_stamps, from K_KHAT again.  One 512^2 mixed call of 3 rows x 3 wavelengths:
    all three give the same final stamps bit for bit.  The arithmetic is the same in every pair: khat_body
    (conv_frames.h) is one inline body compiled with the same flags into both kernels; a host-output reconstruct
    and convolve_stamps both run k_conv_fft<float, double>; and `pre` is fetched as the float64 of float values, so
    its way back into convolve_stamps is exact."""
    see, gl, l0 = np.array([0.5, 1.0, 2.2]), np.array([0.9, 0.6, 0.1]), np.array([28.0, 20.0, 9.0])
    ps = api.grid_pixscale(512)
    ctx = api.Context(dim=512, pixscale=ps, precision='mixed')
    r1 = ctx.reconstruct(LB, see, gl, l0)
    pre1 = ctx.debug_fetch('pre', (3, LB.size, 40, 40))
    ctx.set_option('head_fusion', 0)
    r0 = ctx.reconstruct(LB, see, gl, l0)
    pre0 = ctx.debug_fetch('pre', (3, LB.size, 40, 40))
    alone = ctx.convolve_stamps(LB, see, gl, l0, pre0)
    ctx.close()
    assert np.array_equal(pre1.astype(np.float32).astype(np.float64), pre1)
    assert np.array_equal(pre1, pre0)
    assert np.array_equal(r0['psf'], alone)
    assert np.array_equal(r1['psf'], r0['psf'])
    want = T.final_stamps(LB, see, gl, l0, pre0, ps)
    err = _errors(alone, want).max()
    record_margin('conv_alone', in_call_mixed=err)
    assert err < TOL['mixed']
