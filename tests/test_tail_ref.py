"""CPU checks of tests/tail_ref.py, the fp64 references the GPU tests of the tail kernels compare with."""
import numpy as np

import psfr_oracle as O
import tail_ref as T


def test_fftconvolve_reference_against_the_direct_sum():
    """final_stamps (scipy.signal.fftconvolve, as the reference) against the oracle's direct zero-padded sums, on
    random stamps and on impulses at the corners, an edge and the middle: 1e-13 of the output's peak."""
    rng = np.random.default_rng(5)
    lb = np.array([465.0, 930.0])
    for ps, (see, gl, l0) in ((0.2, (0.3, 0.98, 8.1)), (0.0762, (2.5, 0.02, 29.9))):
        stamps = [rng.random((40, 40))]
        for a, b in ((0, 0), (0, 39), (39, 0), (39, 39), (39, 17), (20, 20)):
            s = np.zeros((40, 40))
            s[a, b] = 1.0
            stamps.append(s)
        for s in stamps:
            pre = np.stack([s, s])
            got = T.final_stamps(lb, see, gl, l0, pre, ps)
            want = O.convolve_final_psf(lb, see, gl, l0, pre, ps)
            for k in range(2):
                assert np.abs(got[k] - want[k]).max() < 1e-13 * want[k].max()
    # an impulse through the instrument kernel alone gives the kernel's cut-out exactly
    s = np.zeros((1, 40, 40))
    s[0, 39, 0] = 1.0
    got = T.final_stamps([700.0], 1.0, 1.0, 20.0, s, 0.2, tiptilt=False)[0]
    ker = T.kernels([700.0], 1.0, 0.5, 20.0, 0.2)[1][0]
    assert np.array_equal(O.convolve_same(s[0], ker)[19:, :21], ker[:21, 20:])     # out[i, j] = ker[i - 19, j + 20]
    want = O.convolve_same(s[0], ker)
    assert np.abs(got - want).max() < 1e-15


def test_moffat_jacobian_against_central_differences():
    for v in ((1.3, 19.3, 20.4, 5.0, 0.4), (0.7, 3.3, 35.6, 2.0, 1 / 1.1), (1.0, -0.4, 12.0, 12.0, 0.125),
              (2.0, 20.0, 20.0, 30.0, 0.05)):
        v = np.array(v)
        J = T.moffat_jacobian(v)
        for k in range(5):
            h = 1e-6 * max(abs(v[k]), 1.0)
            vp, vm = v.copy(), v.copy()
            vp[k] += h
            vm[k] -= h
            fd = ((T.moffat_vw(vp) - T.moffat_vw(vm)) / (2 * h)).ravel()
            assert np.abs(J[:, k] - fd).max() < 1e-8 * max(np.abs(fd).max(), 1.0), (v, k)


def test_kappa_reproduces_the_table_of_the_design_notes():
    """Spot values of the ill-conditioning number of exact Moffats, centre (19.5, 19.5)."""
    for fw, n, want in ((5, 2.5, 5.1), (2, 20, 1.5e3), (12, 8, 27), (1.5, 8, 666), (45, 1.1, 2.0), (20, 50, 838)):
        assert abs(T.kappa(1.0, 19.5, 19.5, fw, n) / want - 1) < 0.04, (fw, n)
    assert abs(T.kappa(3.0, 19.5, 19.5, 5, 2.5) / T.kappa(1.0, 19.5, 19.5, 5, 2.5) - 1) < 1e-9   # peak-independent


def test_perturbed_cases_have_one_minimum_and_the_oracles_error_columns():
    """Every perturbed stamp is a yardstick: MINPACK reaches the same minimum to 1e-9 from the truth and from the
    truth x 1.05; and tail_ref.fit's error columns are those of oracle.moffat_fit(errors=True) (its own start, its
    own variables) where that start converges too (the centred cases)."""
    cases = T.perturbed_cases()
    assert len(cases) == 8
    keys = ('peak', 'p0', 'q0', 'fwhm', 'n')
    for name, truth, stamp in cases:
        a = T.fit(stamp, truth)
        b = T.fit(stamp, tuple(1.05 * x for x in truth))
        for k in keys:
            assert abs(a[k] - b[k]) < 1e-9 * max(abs(a[k]), 1.0), (name, k)
        assert abs(a['chi2'] / b['chi2'] - 1) < 1e-9
        assert max(abs(a[k] - t) for k, t in zip(keys, truth)) > 1e-5, name      # not the truth: a real test
        if name.endswith('centre'):
            o = O.moffat_fit(stamp, 1.0, errors=True)
            assert abs(o['n'] - a['n']) < 1e-8 and abs(o['fwhm'] - a['fwhm']) < 1e-8
            for ko, ka in (('err_peak', 'err_peak'), ('err_alpha', 'err_alpha'), ('err_n', 'err_n'),
                           ('err_fwhm', 'err_fwhm'), ('flux', 'flux'), ('chi2', 'chi2')):
                assert abs(o[ko] / a[ka] - 1) < 1e-6, (name, ko)
            assert abs(o['err_center'][0] / a['err_p0'] - 1) < 1e-6
