"""CPU: the yardstick of the PSF-model fit of blended stars (tests/psf_group_ref.py) against its own definition, and the
Python layer of mpsfr_fit_groups_psf.

* the analytic Jacobian of the three modes equals central differences to 1e-6 (relative to the largest entry of its
  column);
* the yardstick's floor on the shared groups, every (K, back, mode) and every group: a restart 0.3 px off reaches the
  same minimum to <= 1e-6 formal sigma, SciPy reports convergence, every fitted position stays inside the domain, the
  Marquardt-scaled normal matrix is well conditioned, and the pulls of the groups whose model is exact are of order 1;
* fitted as a single star, the brightest source of a blend of two is off by more than 5 of the group fit's sigma on at
  least half of the groups: the point of the feature;
* header constants, the export, the argument helpers, the marshalling of the four call shapes (through the recording
  library of tests/test_lib_calls_host.py), and fit_star_groups_with_psf's bucketing, routing and row order.
"""
import os
import re

import numpy as np
import pytest

import psf_fit_ref as R
import psf_group_ref as G
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec
from test_lib_calls_host import CTX, DEV, DEVP, NULL, OUT, STAMPS, VAR, I, V, expect, make_ctx


def test_jacobian_against_central_differences():
    worst = 0.0
    for K, back, mode in ((2, True, 'free'), (3, False, 'common'), (4, True, 'free'), (4, True, 'common'),
                          (3, True, 'fixed')):
        data, var, psf, F, pos, b = G.groups(K, back)
        for g in (0, 3, 7):
            given = G.given_positions(pos[g], mode)
            x = G.start(np.nan_to_num(data[g]), None, psf[g], given, back, mode)
            if mode == 'free':
                x[1:3 * K:3] += 0.137
                x[2:3 * K:3] -= 0.291
            elif mode == 'common':
                x[K:K + 2] += (0.137, -0.291)
            _, J = G.model(psf[g], x, given, back, mode, jac=True)
            for c in range(len(x)):
                h = 1e-5 * max(abs(x[c]), 1.0) if np.max(np.abs(J[..., c])) <= 1.0 else 1e-5
                xp, xm = x.copy(), x.copy()
                xp[c] += h
                xm[c] -= h
                num = (G.model(psf[g], xp, given, back, mode) - G.model(psf[g], xm, given, back, mode)) / (2 * h)
                worst = max(worst, float(np.max(np.abs(num - J[..., c])) / np.max(np.abs(J[..., c]))))
    print('Jacobian against central differences: %.2e' % worst)
    assert worst <= 1e-6


@pytest.mark.parametrize('back', [False, True])
@pytest.mark.parametrize('K', G.SIZES)
def test_floor_of_the_yardstick_on_the_shared_groups(K, back):
    for mode in G.MODES:
        data, var, psf, F, pos, b, given, fits = G.yardstick(K, back, mode)
        assert len(fits) == G.NGROUP == 12
        assert np.isnan(data).mean() > 0.02 and np.any(var == 0)
        worst, cond, pulls = 0.0, 0.0, []
        for g, f in enumerate(fits):                        # every group: none is left out
            assert f['npix'] == R.used_pixels(data[g], var[g]).sum()
            assert np.all(np.abs(f['pos']) < R.MAX_SHIFT)
            assert np.max(np.abs(f['pos'] - pos[g])) < 0.5
            cond = max(cond, f['cond'])
            if mode != 'fixed':
                assert f['status'] > 0
                x0 = f['x'].copy()
                x0[G.i_flux(K, mode)] *= 1.01
                if mode == 'free':
                    x0[1:3 * K:3] += 0.3
                    x0[2:3 * K:3] -= 0.3
                else:
                    x0[K:K + 2] += (0.3, -0.3)
                h = G.fit(data[g], var[g], psf[g], given[g], back, mode, x0=x0)
                worst = max(worst, float(np.max(np.abs(h['x'] - f['x']) / f['err'])))
                assert abs(h['chi2'] - f['chi2']) <= 1e-9 * f['chi2']
            else:
                sol = G.linear_solve(data[g], var[g], psf[g], given[g], back)
                assert np.max(np.abs(f['x'] - sol)) <= 1e-11 * np.max(np.abs(sol))
            if g % 4 == 3 and mode == 'free':               # the model is exact for these groups
                pulls.extend(((f['F'] - F[g]) / f['err_F']).tolist())
                pulls.extend(((f['pos'] - pos[g]) / f['err_pos']).ravel().tolist())
        print('K=%d back=%d %s: restart 0.3 px off agrees to %.2e sigma; condition %.1e' % (K, back, mode, worst, cond))
        assert worst <= 1e-6
        assert cond <= 1e4
        if pulls:
            rms = float(np.sqrt(np.mean(np.square(pulls))))
            print('    rms pull of the exact-model groups %.2f (%d values)' % (rms, len(pulls)))
            assert 0.5 < rms < 2.0


def test_a_single_star_fit_of_a_blend_is_wrong_by_many_sigma():
    data, var, psf, F, pos, b, given, fits = G.yardstick(2, True, 'free')
    off = []
    for g, f in enumerate(fits):
        k = int(np.argmax(F[g]))
        single = R.fit(data[g], var[g], psf[g], True, shift=given[g][k])
        off.append(abs(single['x'][0] - f['F'][k]) / f['err_F'][k])
    print('single-star flux of the brightest source, in sigma of the group fit: ' + ' '.join('%.1f' % o for o in off))
    assert sum(o > 5.0 for o in off) >= len(off) // 2


def test_header_constants_and_symbol():
    src = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    for name, val in (('MPSFR_MAX_GROUP', _lib.MAX_GROUP), ('MPSFR_NFIT_GROUP', _lib.NFIT_GROUP),
                      ('MPSFR_FIT_COMMON_SHIFT', _lib.FIT_COMMON_SHIFT)):
        assert int(re.search(r'#define %s\s+(\d+)' % name, src).group(1)) == val, name
    assert (_lib.MAX_GROUP, _lib.NFIT_GROUP, _lib.FIT_COMMON_SHIFT) == (4, 48, 8)
    body = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'int mpsfr_fit_groups_psf\(mpsfr_ctx\* ctx, int nstamp, int nsrc, const double\* stamps, '
                     r'const double\* var, int npsf,\s+const double\* psf, const int32_t\* psf_index, '
                     r'const double\* shift,\s+int flags,\s+double\* fit_out, int on_device\);', body)
    assert 'mpsfr_fit_groups_psf' in _lib.EXPORTS
    import muse_psfr_amd
    assert (muse_psfr_amd.NFIT_GROUP, muse_psfr_amd.MAX_GROUP, muse_psfr_amd.FIT_COMMON_SHIFT) == (48, 4, 8)
    assert callable(muse_psfr_amd.fit_star_groups_with_psf)


def test_argument_validation():
    assert _lib.group_fit_flags(True, 'free') == 1 and _lib.group_fit_flags(False, 'free') == 0
    assert _lib.group_fit_flags(True, 'common') == 9 and _lib.group_fit_flags(False, 'fixed') == 4
    for bad in ((1, 'free'), (True, 'both'), (True, None), (True, 12), (True, ('common', 'fixed'))):
        with pytest.raises(ValueError):
            _lib.group_fit_flags(*bad)
    psf = np.ones((3, 40, 40))
    ps, ix, sh, flags = _lib.group_fit_arguments(3, psf, None, np.zeros((3, 2, 2)), True, 'common')
    assert ps.shape == (3, 40, 40) and ix is None and sh.shape == (3, 2, 2) and flags == 9
    ps, ix, sh, flags = _lib.group_fit_arguments(5, psf, [0, 2, 1, 1, 0], np.full((5, 4, 2), 8.0), False, 'fixed')
    assert ix.dtype == np.int32 and ix.tolist() == [0, 2, 1, 1, 0] and sh.shape == (5, 4, 2) and flags == 4
    nan = np.zeros((3, 2, 2))
    nan[1, 1, 0] = np.nan
    far = np.zeros((3, 3, 2))
    far[2, 0, 1] = 8.5
    bad = (dict(shift=np.zeros((3, 1, 2))), dict(shift=np.zeros((3, 5, 2))),       # nsrc 1 and 5
           dict(mode='both'), dict(mode=('common', 'fixed')),                         # both shift flags
           dict(shift=nan), dict(shift=far), dict(shift=None),
           dict(psf_index=[0, 1, 3]), dict(psf_index=[0, -1, 1]), dict(psf_index=[0, 1]),
           dict(nstamp=2), dict(shift=np.zeros((2, 2, 2))), dict(shift=np.zeros((3, 2, 3))), dict(shift=np.zeros(12)),
           dict(background=1), dict(psf=np.ones((3, 40, 39))))
    for kw in bad:
        args = dict(nstamp=3, psf=psf, psf_index=None, shift=np.zeros((3, 2, 2)), background=True, mode='free')
        args.update(kw)
        with pytest.raises(ValueError):
            _lib.group_fit_arguments(**args)


# mpsfr_fit_groups_psf(ctx, nstamp, nsrc, stamps, var, npsf, psf, psf_index, shift, flags, fit_out, on_device): flags
# 1 background, 4 fixed, 8 common shift
def test_marshalling_of_the_four_call_shapes():
    ctx = make_ctx()
    rng = np.random.default_rng(3)
    model = rng.uniform(0.1, 1.0, (2, 40, 40))
    index = np.array([0, 1, 1, 0, 1])
    shift = rng.uniform(-2.0, 2.0, (5, 3, 2))
    out = ctx.fit_groups_psf(STAMPS, STAMPS, shift[:, :2])
    assert out.shape == (5, _lib.NFIT_GROUP) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_fit_groups_psf', [CTX, I(5), I(2), V(STAMPS), NULL, I(5), V(STAMPS), NULL,
                                                V(shift[:, :2]), I(1), OUT(out), I(0)])
    out = ctx.fit_groups_psf(STAMPS, model, shift, var=VAR, psf_index=index, background=False, mode='common')
    expect(ctx.lib, 1, 'mpsfr_fit_groups_psf', [CTX, I(5), I(3), V(STAMPS), V(VAR), I(2), V(model), V(index, np.int32),
                                                V(shift), I(8), OUT(out), I(0)])
    assert ctx.fit_groups_psf_device(5, 4, DEV['stamps'], 5, DEV['model'], DEV['shift'], DEV['fit']) is None
    expect(ctx.lib, 2, 'mpsfr_fit_groups_psf', [CTX, I(5), I(4), DEVP(DEV['stamps']), NULL, I(5), DEVP(DEV['model']),
                                                NULL, DEVP(DEV['shift']), I(1), DEVP(DEV['fit']), I(1)])
    ctx.fit_groups_psf_device(5, 2, DEV['stamps'], 2, DEV['model'], DEV['shift'], DEV['fit'], var_ptr=DEV['var'],
                              psf_index_ptr=DEV['index'], background=True, mode='fixed')
    expect(ctx.lib, 3, 'mpsfr_fit_groups_psf', [CTX, I(5), I(2), DEVP(DEV['stamps']), DEVP(DEV['var']), I(2),
                                                DEVP(DEV['model']), DEVP(DEV['index']), DEVP(DEV['shift']), I(5),
                                                DEVP(DEV['fit']), I(1)])
    for bad in (dict(nsrc=1), dict(nsrc=5), dict(nstamp=0), dict(shift_ptr=0), dict(fit_ptr=None), dict(npsf=2),
                dict(mode='both')):
        args = dict(nstamp=5, nsrc=2, stamps_ptr=1, npsf=5, psf_ptr=1, shift_ptr=1, fit_ptr=1)
        args.update(bad)
        with pytest.raises(ValueError):
            ctx.fit_groups_psf_device(**args)
    assert len(ctx.lib.calls) == 4
    ctx._h = None


class _FakeContext:
    """Records the library calls of fit_star_groups_with_psf and answers with rows that name their stamp: the stamp's
    number is its pixel [0, 0]; F of source k is 100 stamp + k, its position is the given one."""

    def __init__(self):
        self.calls = []

    def fit_stamps_psf(self, stamps, psf, var=None, psf_index=None, shift=None, background=True, fixed_shift=False):
        self.calls.append(('single', len(stamps), psf_index.tolist(), background, fixed_shift, var is not None))
        out = np.zeros((len(stamps), _lib.NFIT_PSF))
        out[:, 0] = 100 * stamps[:, 0, 0]
        out[:, 1:3] = shift
        out[:, 3], out[:, 4], out[:, 11] = stamps[:, 0, 0] + 0.5, 7.0, 1600
        return out

    def fit_groups_psf(self, stamps, psf, shift, var=None, psf_index=None, background=True, mode='free'):
        K = shift.shape[1]
        self.calls.append(('group', K, len(stamps), psf_index.tolist(), background, mode, var is not None))
        out = np.zeros((len(stamps), _lib.NFIT_GROUP))
        out[:, 0], out[:, 2], out[:, 5], out[:, 6] = stamps[:, 0, 0] + 0.5, 7.0, 1600, K
        for k in range(K):
            out[:, 8 + 8 * k] = 100 * stamps[:, 0, 0] + k
            out[:, 9 + 8 * k:11 + 8 * k] = shift[:, k]
        out[:, 40:46] = [0.1, -0.6, 0.3, 0.2, -0.25, 0.5]
        out[:, 40:46] *= np.array([j < K for _, j in G.PAIRS])
        return out


def test_fit_star_groups_buckets_by_size_and_keeps_the_input_order(monkeypatch):
    fake = _FakeContext()
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: fake)
    n = 6
    stars = np.ones((n, 40, 40)) * np.arange(n)[:, None, None]
    psf = np.ones((2, 40, 40))
    index = [0, 1, 1, 0, 1, 0]
    sizes = [2, 1, 3, 2, 1, 4]
    rng = np.random.default_rng(4)
    positions = [rng.uniform(-1.0, 1.0, (k, 2)) for k in sizes]
    t = psfrec.fit_star_groups_with_psf(stars, psf, positions, psf_index=index, mode='common', pixscale=0.2)
    assert fake.calls == [('single', 2, [1, 1], True, False, False), ('group', 2, 2, [0, 0], True, 'common', False),
                          ('group', 3, 1, [1], True, 'common', False), ('group', 4, 1, [0], True, 'common', False)]
    names = list(t.colnames if hasattr(t, 'colnames') else t.keys())
    assert names == ['group', 'source', 'scale', 'shift', 'flux', 'err_scale', 'err_shift', 'err_flux', 'back',
                     'err_back', 'chi2', 'npix', 'status', 'max_corr']
    group, source = np.asarray(t['group']), np.asarray(t['source'])
    assert group.tolist() == [0, 0, 1, 2, 2, 2, 3, 3, 4, 5, 5, 5, 5]
    assert source.tolist() == [0, 1, 0, 0, 1, 2, 0, 1, 0, 0, 1, 2, 3]
    np.testing.assert_array_equal(np.asarray(t['scale']), 100 * group + source)
    np.testing.assert_allclose(np.asarray(t['shift']), np.concatenate(positions), rtol=0, atol=1e-15)   # arcsec
    np.testing.assert_array_equal(np.asarray(t['back']), group + 0.5)
    np.testing.assert_array_equal(np.asarray(t['npix']), 1600)
    want = {1: [0.0], 2: [0.1, 0.1], 3: [0.6, 0.2, 0.6], 4: [0.6, 0.25, 0.6, 0.5]}
    np.testing.assert_array_equal(np.asarray(t['max_corr']), np.concatenate([want[k] for k in sizes]))
    # the (n, K, 2) form with NaN rows is the same request; 'fixed' holds the single stars' shifts too
    fake.calls.clear()
    arr = np.full((n, 4, 2), np.nan)
    for g, p in enumerate(positions):
        arr[g, :len(p)] = p
    var = np.ones_like(stars)
    t2 = psfrec.fit_star_groups_with_psf(stars, psf, arr, psf_index=index, var=var, fit_back=False, mode='fixed')
    assert fake.calls == [('single', 2, [1, 1], False, True, True), ('group', 2, 2, [0, 0], False, 'fixed', True),
                          ('group', 3, 1, [1], False, 'fixed', True), ('group', 4, 1, [0], False, 'fixed', True)]
    np.testing.assert_array_equal(np.asarray(t2['scale']), np.asarray(t['scale']))


def test_fit_star_groups_refuses_before_any_context(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('a GPU context was requested before the arguments were checked')
    monkeypatch.setattr(psfrec, 'get_context', refuse)
    stars, psf = np.ones((2, 40, 40)), np.ones((2, 40, 40))
    ok = [np.zeros((2, 2)), np.zeros((1, 2))]
    bad = (dict(positions=[np.zeros((2, 2))]), dict(positions=[np.zeros((5, 2)), np.zeros((1, 2))]),
           dict(positions=[np.zeros((0, 2)), np.zeros((1, 2))]), dict(positions=np.full((2, 2, 2), np.nan)),
           dict(positions=[np.array([[0.0, 1.7]]), np.zeros((1, 2))]),                 # 8.5 px at 0.2 arcsec
           dict(positions=[np.array([[0.0, np.inf]]), np.zeros((1, 2))]), dict(positions=np.zeros((2, 2, 3))),
           dict(mode='both'), dict(fit_back=1), dict(pixscale=0.0), dict(psf=np.ones((3, 40, 40))),
           dict(psf_index=[0, 2]), dict(stars=np.ones((2, 40, 39))), dict(var=np.ones((2, 40, 39))))
    for kw in bad:
        args = dict(stars=stars, psf=psf, positions=ok)
        args.update(kw)
        with pytest.raises(ValueError):
            psfrec.fit_star_groups_with_psf(args.pop('stars'), args.pop('psf'), args.pop('positions'), **args)
