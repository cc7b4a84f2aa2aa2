"""CPU: Cn2 profiles (compute_profile_psf, Context.reconstruct_profile, simul_psd_wfm(wind_dir=...)) refuse bad
profiles before any GPU context exists or the library is called, the header declares what the binding passes, and
the g9 fixture's two-layer case is the oracle's AO zone."""
import os
import re

import numpy as np
import pytest

import psfr_oracle as O
from conftest import ROOT, H, rel_err
from muse_psfr_amd import _lib, psfrec


@pytest.fixture
def no_context(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('a GPU context was requested before the arguments were checked')
    monkeypatch.setattr(psfrec, 'get_context', refuse)


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError('the library was called before the arguments were checked')


@pytest.fixture
def bare_context():
    """A Context whose library refuses every call: refusals must happen before it is reached."""
    ctx = object.__new__(_lib.Context)
    ctx.lib = _NoLib()
    ctx.dim, ctx.pixscale, ctx.dimpsf, ctx.precision = 512, 0.2, 40, 'mixed'
    ctx._pending = {}
    return ctx


GOOD = dict(cn2=[0.6, 0.25, 0.15], h=[0.0, 1000.0, 10000.0], wind_speed=[8.0, 15.0, 30.0], wind_dir=[0.3, -1.0, 2.0])

BAD_PROFILES = [
    dict(cn2=[], h=[], wind_speed=[], wind_dir=[]),                                  # no layer
    dict(cn2=[1.0] * 9, h=[100.0 * k for k in range(9)], wind_speed=[10.0] * 9, wind_dir=[0.0] * 9),   # 9 layers
    dict(h=[0.0, np.nan, 10000.0]),
    dict(h=[0.0, 1000.0, np.inf]),
    dict(h=[-1.0, 1000.0, 10000.0]),
    dict(h=[0.0, 1000.0, 50001.0]),
    dict(wind_speed=[8.0, np.nan, 30.0]),
    dict(wind_speed=[8.0, -0.5, 30.0]),
    dict(wind_speed=[8.0, 15.0, 100.5]),
    dict(wind_dir=[0.3, np.inf, 2.0]),
    dict(wind_dir=[0.3, -1.0]),                                                      # one direction short
    dict(wind_speed=[8.0, 15.0]),
    dict(cn2=[0.6, -0.25, 0.15]),
    dict(cn2=[0.6, np.nan, 0.15]),
    dict(cn2=[0.6, np.inf, 0.15]),
    dict(cn2=[0.0, 0.0, 0.0]),
    dict(cn2=[0.6, 0.4]),                                                            # one weight short
]


def _profile(kw):
    p = dict(GOOD)
    p.update(kw)
    return p


@pytest.mark.parametrize('kw', BAD_PROFILES)
def test_compute_profile_psf_refuses_bad_profiles_before_any_context(no_context, kw):
    p = _profile(kw)
    with pytest.raises(ValueError):
        psfrec.compute_profile_psf([600.0], 1.0, 25.0, p['cn2'], p['h'], p['wind_speed'], p['wind_dir'],
                                   verbose=False)


@pytest.mark.parametrize('kw', [dict(npsflin=0), dict(npsflin=6), dict(npsflin=2.5), dict(seeing=-1.0),
                                dict(L0=0.0), dict(lbda=[]), dict(lbda=[-600.0]), dict(GL=1.5),
                                dict(precision='f32'), dict(positions=[[0.0, 61.0]]),
                                dict(positions=np.zeros((0, 2))), dict(wind_dir=None),
                                dict(cn2=[[0.6, 0.25, 0.15]])])
def test_compute_profile_psf_refuses_bad_arguments_before_any_context(no_context, kw):
    args = dict(lbda=[600.0], seeing=1.0, L0=25.0, verbose=False, **GOOD)
    args.update(kw)
    with pytest.raises(ValueError):
        psfrec.compute_profile_psf(**args)


def test_simul_psd_wfm_profile_refusals_before_any_context(no_context):
    for kw in BAD_PROFILES:
        p = _profile(kw)
        with pytest.raises(ValueError):
            psfrec.simul_psd_wfm(p['cn2'], p['h'], 1.0, 25.0, wind_speed=p['wind_speed'], wind_dir=p['wind_dir'],
                                 verbose=False)
    # without wind_dir the two-layer rule of today stands
    with pytest.raises(ValueError):
        psfrec.simul_psd_wfm([0.5, 0.3, 0.2], (100, 1000, 10000), 1.0, 25.0, verbose=False)
    # and the two-layer call keeps the reference's winds: a wind speed needs wind_dir
    for ws in (10.0, [10.0, 20.0]):
        with pytest.raises(ValueError):
            psfrec.simul_psd_wfm([0.7, 0.3], (100, 10000), 1.0, 25.0, verbose=False, wind_speed=ws)


@pytest.mark.parametrize('kw', BAD_PROFILES)
def test_context_reconstruct_profile_refuses_before_the_library(bare_context, kw):
    p = _profile(kw)
    with pytest.raises(ValueError):
        bare_context.reconstruct_profile([600.0], [1.0], [0.6], [25.0], p['cn2'], p['h'], p['wind_speed'],
                                         p['wind_dir'])
    with pytest.raises(ValueError):
        bare_context.reconstruct_profile_device([600.0], [1.0], [0.6], [25.0], p['cn2'], p['h'], p['wind_speed'],
                                                p['wind_dir'], [0], 1, None, None, 0, 0, 0)


@pytest.mark.parametrize('kw', [dict(npsflin=0), dict(npsflin=6), dict(npsflin=1, positions=[[0.0, 0.0]]),
                                dict(positions=[[0.0, 0.0]] * 26), dict(positions=[[np.nan, 0.0]]),
                                dict(cn2=np.ones((3, 3)))])
def test_context_reconstruct_profile_refuses_bad_modes(bare_context, kw):
    args = dict(GOOD)
    args.update(kw)
    with pytest.raises(ValueError):
        bare_context.reconstruct_profile([600.0], [1.0, 0.8], [0.6, 0.5], [25.0, 20.0], **args)


def test_profile_columns_and_shapes_in_both_modes(monkeypatch):
    """compute_profile_psf assembles compute_psf's / compute_field_psf's tables from what the context returns."""
    calls = []

    class FakeCtx:
        def reconstruct_profile(self, lbda, seeing, gl, l0, cn2, h, ws, wd, three, npsflin=None, positions=None,
                                masks=None, want_sum=True):
            calls.append(dict(gl=gl, cn2=np.array(cn2), h=h, ws=ws, wd=wd, npsflin=npsflin, positions=positions))
            nl = len(lbda)
            lead = (1,) if positions is None else (1, len(positions))
            fit = np.ones(lead + (nl, _lib.NFIT)) * 2.0
            return dict(psf=np.zeros(lead + (nl, 40, 40)), fit=fit, psf_sum=None)

    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: FakeCtx())
    lb = [500.0, 700.0, 900.0]
    t, psf = psfrec.compute_profile_psf(lb, 1.0, 25.0, verbose=False, **GOOD)
    assert psf.shape == (3, 40, 40) and len(t) == 3
    assert list(t.colnames)[:len(psfrec._FIT_COLS)] == list(psfrec._FIT_COLS)
    assert {'SEEING', 'GL', 'L0'} <= set(t.colnames)
    assert calls[-1]['npsflin'] == 1 and calls[-1]['positions'] is None
    # GL defaults to the normalised weight of the lowest layer
    assert calls[-1]['gl'] == [0.6]
    np.testing.assert_array_equal(t['GL'], 0.6)
    pos = [[0.0, 0.0], [30.0, 0.0], [-30.0, 0.0], [0.0, 45.0], [-50.0, -50.0]]
    t, psf = psfrec.compute_profile_psf(lb, 1.0, 25.0, positions=pos, GL=0.3, verbose=False, **GOOD)
    assert psf.shape == (5, 3, 40, 40) and len(t) == 15
    assert list(t.colnames)[:3] == ['dir_idx', 'x', 'y']
    np.testing.assert_array_equal(t['dir_idx'], np.repeat(np.arange(5), 3))
    np.testing.assert_array_equal(t['x'], np.repeat(np.array(pos)[:, 0], 3))
    assert calls[-1]['npsflin'] == 0 and calls[-1]['gl'] == [0.3]
    # two layers without wind_dir: the reference's directions
    psfrec.compute_profile_psf(lb, 1.0, 25.0, [0.7, 0.3], (100, 10000), verbose=False)
    np.testing.assert_array_equal(calls[-1]['wd'], _lib.REF_WIND_DIR)
    np.testing.assert_array_equal(calls[-1]['ws'], [12.5, 12.5])
    assert calls[-1]['gl'] == [0.7]
    # more than 25 positions go in several calls
    psfrec.compute_profile_psf(lb, 1.0, 25.0, positions=np.zeros((30, 2)), verbose=False, **GOOD)
    assert [len(c['positions']) for c in calls[-2:]] == [25, 5]


def test_golden_two_layer_case_is_the_oracle(golden, ref_masks):
    g = golden('g9_profile')
    tabs = O.ao_tables(H, False, 1, masks=ref_masks)
    for ci, (see, gl, l0) in enumerate(g['e_cases']):
        d = O.ao_zone_psd(np.array([gl, 1 - gl]), H, l0, O.seeing_to_r0(see), False, 1, tables=tabs)
        assert rel_err(d, g['e_dsp_c%d' % ci]) < 1e-13


def test_golden_profiles_are_what_the_fixture_says(golden):
    g, gd, g1 = golden('g9_profile'), golden('g9_profile_field'), golden('g1_ao_zone')
    assert g['a_h'].size == 3 and g['b_h'].size == 7 and g['c_h'].size == 1
    assert np.count_nonzero(g['b_cn2'] == 0) == 1 and bool(g['b_three']) and int(g['b_npsflin']) == 3
    assert g['b_zone'].shape == (9, 80, 80) and gd['d_zone'].shape == (5, 80, 80)
    assert int(g['c_dim']) == 1280 and g['c_lbda'].size == 3 and int(g['a_dim']) == 512
    np.testing.assert_array_equal(gd['d_dirs'].T, [[0, 0], [30, 0], [-30, 0], [0, 45], [-50, -50]])
    # the masks the reference saw are the g1 fixture's (what the GPU tests pass as ref_masks)
    np.testing.assert_array_equal(g['mask_rec'], g1['mask_rec'])
    np.testing.assert_array_equal(g['mask_res'], g1['mask_res'])
    for k, src in (('a', g), ('b', g), ('c', g), ('d', gd)):
        assert np.all(np.isfinite(src[k + '_zone'])) and np.all(src[k + '_zone'] >= 0)
        nl = src[k + '_lbda'].size
        lead = (5, nl) if k == 'd' else (nl,)
        assert src[k + '_pre'].shape == lead + (40, 40) and src[k + '_fin'].shape == lead + (40, 40)
        assert src[k + '_fit'].shape == lead + (5,)
        np.testing.assert_allclose(src[k + '_pre'].sum(axis=(-2, -1)), 1.0, rtol=1e-10)


def _prototype(src, name):
    m = re.search(r'\b%s\s*\((.*?)\);' % name, src, re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(',')]


def _ctype(arg):
    t = re.sub(r'\s*\b\w+\s*(\[\d*\])?$', '', arg.replace('/*', '').strip())
    t = t.replace('const ', '').replace(' ', '')
    return t


def test_header_prototypes_match_the_binding():
    import ctypes as C
    src = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert int(re.search(r'#define MPSFR_MAX_LAYERS\s+(\d+)', src).group(1)) == _lib.MAX_LAYERS
    m = {'mpsfr_ctx*': C.c_void_p, 'int': C.c_int, 'double': C.c_double, 'double*': C.POINTER(C.c_double),
         'uint8_t*': C.POINTER(C.c_uint8)}
    lib = _lib.load()
    for name in ('mpsfr_reconstruct_profile', 'mpsfr_simul_psd_profile'):
        args = _prototype(src, name)
        want = [m[_ctype(a)] for a in args]
        got = getattr(lib, name).argtypes
        assert len(got) == len(want), name
        for k, (g_, w) in enumerate(zip(got, want)):
            if w is C.POINTER(C.c_double) and args[k].split()[-1].endswith('_out'):
                assert g_ in (C.c_void_p, C.POINTER(C.c_double)), (name, k)
            else:
                assert g_ is w, (name, k, args[k])
        assert getattr(lib, name).restype is C.c_int
