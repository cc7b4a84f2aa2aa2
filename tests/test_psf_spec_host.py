"""CPU: the fp64 yardstick of the PSF-model fit of star cubes (tests/psf_spec_ref.py) -- its Jacobian, the elimination
formulas of mpsfr_fit_spectra_psf against the joint solution, its minimum, the default start -- and the argument
validation of the Python wrappers (no GPU call)."""
import numpy as np
import pytest

import psf_spec_ref as SR

VARIANTS = SR.VARIANTS
IDS = ['%s-%s' % ('back' if b else 'noback', 'drift' if d else 'nodrift') for b, d in VARIANTS]


@pytest.mark.parametrize('back,drift', VARIANTS, ids=IDS)
def test_jacobian_against_central_differences(back, drift):
    ss, fits = SR.yardstick(back, drift)
    prob = SR.problem(ss[0], back, drift)
    v = fits[0]['v'] + 0.05 * np.arange(1, prob.nvar + 1) / prob.nvar
    _, J = prob.residual(v, True)
    for k in range(prob.nvar):
        h = 1e-6 * max(1.0, abs(v[k]))
        e = np.zeros(prob.nvar)
        e[k] = h
        num = (prob.residual(v + e) - prob.residual(v - e)) / (2 * h)
        assert np.abs(num - J[:, k]).max() <= 1e-6 * max(np.abs(J[:, k]).max(), 1e-30), k


@pytest.mark.parametrize('back,drift', VARIANTS, ids=IDS)
def test_elimination_reaches_the_joint_minimum_with_its_errors(back, drift):
    """Variable projection against the joint problem: theta and F within 1e-5 sigma, every error within 1e-6 relative."""
    ss, fits = SR.yardstick(back, drift)
    for s, ref in zip(ss, fits):
        prob = SR.problem(s, back, drift)
        el = SR.eliminated(prob, SR.start_of(s, back))
        nt, lay = prob.nt, prob.layers
        assert np.abs(el['theta'][:nt] - ref['theta'][:nt]).max() <= 1e-5 * ref['err_theta'][:nt].min()
        assert np.all(np.abs(el['F'][lay] - ref['F'][lay]) <= 1e-5 * ref['err_F'][lay])
        assert np.allclose(el['err_theta'][:nt], ref['err_theta'][:nt], rtol=1e-6, atol=0)
        assert np.allclose(el['err_F'][lay], ref['err_F'][lay], rtol=1e-6, atol=0)
        if back:
            assert np.all(np.abs(el['b'][lay] - ref['b'][lay]) <= 1e-5 * ref['err_b'][lay])
            assert np.allclose(el['err_b'][lay], ref['err_b'][lay], rtol=1e-6, atol=0)
        assert abs(el['chi2'] - ref['chi2']) <= 1e-9 * ref['chi2']
        assert np.allclose(el['chi2_l'], ref['chi2_l'], rtol=1e-8, atol=0)
        assert el['dof'] == ref['dof'] == ref['npix'] - (nt + prob.nlin * len(lay))


@pytest.mark.parametrize('back,drift', VARIANTS, ids=IDS)
def test_a_restart_reaches_the_same_minimum_inside_the_domain(back, drift):
    ss, fits = SR.yardstick(back, drift)
    for s, ref in zip(ss, fits):
        prob = SR.problem(s, back, drift)
        again = SR.joint_fit(prob, ref['theta'][:2] + np.array([0.3, -0.3]))
        nt = prob.nt
        assert np.all(np.abs(again['theta'][:nt] - ref['theta'][:nt]) <= 1e-6 * ref['err_theta'][:nt])
        assert np.all(np.abs(again['F'] - ref['F']) <= 1e-6 * np.where(ref['err_F'] > 0, ref['err_F'], 1.0))
        assert prob.inside(ref['theta'])
        # the gradient vanishes at the yardstick's point
        r, J = prob.residual(ref['v'], True)
        assert np.abs(J.T @ r).max() <= 1e-7 * np.abs(J).max() * np.sqrt(r @ r)


@pytest.mark.parametrize('back,drift', VARIANTS, ids=IDS)
def test_default_start_of_the_bright_stars_is_near_the_minimum(back, drift):
    for uneven in (False, True):
        ss, fits = SR.yardstick(back, drift, uneven)
        for s, ref in zip(ss, fits):
            if s['snr'] < 20:
                continue
            st = SR.default_start(s['cube'], s['var'], s['psfs'], back)
            assert np.abs(st - ref['theta'][:2]).max() <= 1.0


def test_left_out_layer_and_counts_of_the_shared_stars():
    ss, fits = SR.yardstick(True, False)
    k, l = SR.NAN_LAYER
    prob = SR.problem(ss[k], True, False)
    assert not prob.fitted[l] and prob.fitted.sum() == prob.nl - 1 and prob.n_used[l] == 0
    assert fits[k]['F'][l] == 0 and fits[k]['nlayers'] == prob.nl - 1
    assert [len(s['cube']) for s in ss] == list(SR.NLAYERS)
    assert len(SR.uneven_stars(True, True)[0]['cube']) == 2 * SR.WAVES + 3


def test_wrapper_argument_validation():
    from muse_psfr_amd import _lib, fit_star_spectra_with_psf
    cube = np.ones((2, 3, 40, 40))
    psf = np.ones((2, 3, 40, 40))
    args = _lib.spectra_fit_arguments
    cu, va, ps, ix, sh, xx, flags = args(cube, None, psf, None, None, True, None)
    assert cu.shape == (2, 3, 40, 40) and va is None and ps.shape == (2, 3, 40, 40) and ix is None and sh is None
    assert xx is None and flags == _lib.FIT_BACKGROUND
    cu, va, ps, ix, sh, xx, flags = args(cube[0], cube[0], psf[:1], [0], [[1.0, -2.0]], False, [-1, 0, 1])
    assert cu.shape == (1, 3, 40, 40) and va.shape == cu.shape and ix.dtype == np.int32 and sh.shape == (1, 2)
    assert flags == _lib.FIT_DRIFT and xx.dtype == np.float64
    bad = [
        dict(cubes=np.ones((3, 40, 41))),
        dict(cubes=np.ones((40, 40))),
        dict(var=np.ones((2, 2, 40, 40))),
        dict(psf=np.ones((2, 4, 40, 40))),
        dict(psf=np.ones((3, 3, 40, 40))),                     # no index and npsf != n
        dict(psf_index=[0, 2]),
        dict(psf_index=[0.0, 1.0]),
        dict(shift=[[0, 0], [9, 0]]),
        dict(shift=[[0, 0], [np.nan, 0]]),
        dict(shift=[0, 0]),
        dict(background=1),
        dict(x=[0, 0, 0]),
        dict(x=[-1, 0, 1.5]),
        dict(x=[-1, 0, np.nan]),
        dict(x=[-1, 1]),
    ]
    for kw in bad:
        full = dict(cubes=cube, var=None, psf=psf, psf_index=None, shift=None, background=True, x=None)
        full.update(kw)
        with pytest.raises(ValueError):
            args(full['cubes'], full['var'], full['psf'], full['psf_index'], full['shift'], full['background'], full['x'])
    with pytest.raises(ValueError):
        args(np.ones((1, 1, 40, 40)), None, np.ones((1, 1, 40, 40)), None, None, True, [0.5])      # drift needs 2 layers
    with pytest.raises(ValueError):
        _lib._spec_layers(_lib.MAX_SPEC_LAYERS + 1)
    lb = [500.0, 700.0, 900.0]
    for kw in (dict(fit_back=1), dict(drift='yes'), dict(pixscale=0.0), dict(lbda=[500.0, 700.0]),
               dict(lbda=[500.0, np.nan, 900.0]), dict(lbda=[700.0] * 3, drift=True)):
        full = dict(lbda=lb)
        full.update(kw)
        lbda = full.pop('lbda')
        with pytest.raises(ValueError):
            fit_star_spectra_with_psf(cube, psf, lbda, **full)
