"""Host: the crowded-field fit of a cube with free positions (mpsfr_fit_cube_psf_free) without a GPU.

1. the yardstick (cube_free_ref) checked on itself: the delta column against central differences of the rendered cube;
   rho < 1/2 in every parity case (the condition the seed of cube_free_cases was picked for) with a pos_tol that leaves
   the loop three steps and more; at nl = 1 its minimiser is frame_free_ref's within the sum of the two bounds; L
   identical layers give the single layer's minimiser; on the noisy cube the joint positions beat the best single
   layer's; the rule on cases written out by hand -- carried in one layer only, nobody free, the dof rule, the
   across-layer +-8 bound.
2. what Context.fit_cube_psf_free and its device form hand to C, every refusal of the Python layer before any library
   call, against the recording stub.
3. psfrec.refine_crowded_spectra against an answering stub, with and without position_layers.
4. constants, exports, the source list.
"""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import cube_fit_cases as K
import cube_free_cases as Q
import cube_free_ref as R
import frame_fit_ref as F
import frame_free_ref as G
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec
from test_cube_fit_host import CubeLib
from test_frame_free_host import FREE_BAD
from test_group_host import _array
from test_render_host import DEV, HANDLE, make_ctx

NS = 40
TOL, MAX_ITER = 1e-12, 100            # of the parity runs of tests/test_gpu_cube_free.py
CASES = list(itertools.product((True, False), (True, False), (4.0, 8.0)))
# the places of the C arguments
(A_CTX, A_NL, A_NY, A_NX, A_CUBE, A_VAR, A_NSTAR, A_NPSF, A_PSF, A_INDEX, A_ORIGIN, A_SHIFT, A_LSHIFT, A_SCALE0, A_RADIUS,
 A_FLAGS, A_MAXIT, A_TOL, A_OUTER, A_POSTOL, A_STEP, A_MOVE, A_SNR, A_ROWS, A_HEAD, A_POS, A_SHOUT, A_CALL, A_RESID,
 A_ONDEV) = range(30)


# ---- 1. the yardstick
def test_delta_column_agrees_with_central_differences_of_the_rendered_cube():
    c = Q.cube(False)
    ls, psf = c['layer_shift'], c['psf']
    flux = np.array([[800.0, 40.0, 3200.0]]).T * np.ones(c['n'])             # F0 [nl][n]
    h = 1e-5
    for k in (0, 8, 17):
        for ax in range(2):
            for l in range(Q.NL):
                def frame(s):
                    return F.column(F.FRAME, psf[c['index'][k], l], c['origin'][k], s + ls[l]) * flux[l, k]
                e = np.zeros(2)
                e[ax] = h
                num = (frame(c['shift'][k] + e) - frame(c['shift'][k] - e)) / (2 * h)
                col = G.columns(F.FRAME, psf[c['index'][k], l], c['origin'][k], c['shift'][k] + ls[l])[1 + ax] * flux[l, k]
                # (frame_free_ref's tolerance: the third derivative of the Keys kernel and the rounding of the difference)
                pk = np.abs(psf[c['index'][k], l]).max() * flux[l, k]
                tol = 1.5 * h * h * pk * 16 + 4 * F.EPS * pk * 16 / h
                assert np.max(np.abs(col - num)) <= tol and np.abs(col).max() > 1e3 * tol


def test_cube_is_what_the_tests_need():
    c, s = Q.cube(False), G.displaced_scene(False, Q.AMPLITUDE, Q.SEED)
    d = c['shift'] - c['truth']
    assert c['cube'].shape == (Q.NL, 97, 150) and c['psf'].shape == (4, Q.NL, NS, NS) and c['n'] == 34
    assert np.array_equal(c['truth'], F.scene(False)['shift']) and np.array_equal(c['shift'], s['shift'])
    assert 0.25 < np.abs(d).max() <= 0.3 and np.array_equal(c['layer_shift'], K.layer_shifts(3))
    assert np.array_equal(Q.cube(True)['shift'], c['shift']) and np.array_equal(c['psf'][:, 1], K.models_of_layer(1))
    # the last layer's models are wider: their peak is lower
    assert c['psf'][0, 2].max() < 0.7 * K.models_of_layer(2)[0].max()
    conv = Q.cube_converged(True, True, 8.0, False, max_outer=10)
    st = [p.base['status'][Q.MASKED] for p in conv['problem'].layers]
    assert st == [0, 2, 0] and list(conv['carried'][:, Q.MASKED]) == [True, False, True]


def test_the_faint_star_is_carried_by_one_layer_under_min_snr_and_by_both_without():
    # (conditions on the yardstick that test_gpu_cube_free.py relies on to tell which layers carried the star)
    c = Q.two_layers('faint')
    ref, both = Q.run(c, max_outer=1), Q.run(c, max_outer=1, min_snr=0.0)
    assert list(ref['carried'][:, Q.FAINT]) == [True, False] and list(both['carried'][:, Q.FAINT]) == [True, True]
    _, by, bx = R.inner_bounds(ref['last'], TOL, MAX_ITER, 2)
    j = int(np.flatnonzero(ref['last']['free'] == Q.FAINT)[0])
    assert np.abs(ref['shift'][Q.FAINT] - both['shift'][Q.FAINT]).max() > 4.0 * max(by[j], bx[j])
    dead = Q.run(Q.two_layers('nan'), max_outer=1)
    assert dead['problem'].live == [0] and dead['closing'][1] is None and dead['nfree_last'] > 0


@pytest.mark.parametrize('with_var,background,radius', CASES)
def test_contraction_is_below_one_half_and_the_inner_solves_fit(with_var, background, radius):
    conv = Q.cube_converged(with_var, background, radius, False, max_outer=10)
    assert conv['rho'] < 0.5, conv['steps']
    assert conv['steps'][-1] <= conv['floor'] < 1e-7 and conv['problem'].live == [0, 1, 2]
    assert len(conv['last']['free']) == conv['problem'].seen.sum()
    # (whether max_iter = 100 is enough for tol = 1e-12 from the warm starts is asserted where it is run: the GPU
    # parity test asks for status 0)
    inner = R.position_bounds(conv, 1.0, TOL, MAX_ITER)[1]
    pos_tol = R.parity_pos_tol(conv, TOL, MAX_ITER)
    steps = np.array(conv['steps'])
    assert 10.0 * inner.max() <= pos_tol < 0.1 and not np.any(np.abs(steps - pos_tol) <= 0.1 * pos_tol)
    assert np.argmax(steps <= pos_tol) >= 2


def _as_cube(s, copies):
    return (np.stack([s['image']] * copies), np.stack([s['var']] * copies),
            np.ascontiguousarray(np.stack([s['psf']] * copies, axis=1)))


@pytest.mark.parametrize('copies', [1, 3])
def test_identical_layers_give_the_minimiser_of_the_frame(copies):
    s = G.displaced_scene(False)
    conv_f = G.scene_converged(True, True, 8.0, False, max_outer=10)
    cube, var, psf = _as_cube(s, copies)
    conv_c = R.converged(cube, var, psf, s['index'], s['origin'], s['shift'], None, 8.0, True, max_outer=10)
    acc = conv_f['problem'].acc
    free = acc[conv_f['last']['free_idx']]
    assert np.array_equal(free, conv_c['last']['free']) and conv_c['rho'] < 0.5
    # each run's own error: the reference and right-side terms of its inner bound (no iteration: tol = 0, k = 0)
    _, fy, fx = G.inner_bounds(conv_f['last'], 0.0, 0)
    _, cy, cx = R.inner_bounds(conv_c['last'], 0.0, 0, copies)
    diff = np.abs(conv_c['shift'][free] - conv_f['shift'][free])
    assert np.all(diff <= np.stack([fy + cy, fx + cx], axis=1)) and diff.max() < 1e-8
    for l in range(copies):
        np.testing.assert_allclose(conv_c['closing'][l]['F'], conv_f['closing']['F'], rtol=1e-7)


def test_joint_positions_beat_the_best_single_layer_on_the_noisy_cube():
    # (seed: the cube's own, default_rng(200 + l) per layer on the draw of SEED)
    c = Q.cube(True)
    joint = Q.run(c)
    quiet = joint['problem'].seen.copy()
    for l in range(Q.NL):
        pr, cl = joint['problem'].layers[l], joint['closing'][l]
        quiet[pr.acc[cl['overlap'] >= 0.5]] = False
        quiet[np.setdiff1d(np.arange(c['n']), pr.acc)] = False
    assert quiet.sum() >= 15

    def rms(shift):
        return float(np.sqrt(np.mean((shift[quiet] - c['truth'][quiet]) ** 2)))
    single = []
    for l in range(Q.NL):
        r = G.refine(c['cube'][l], c['var'][l], np.ascontiguousarray(c['psf'][:, l]), c['index'], c['origin'],
                     c['shift'] + c['layer_shift'][l], 8.0, True)
        single.append(rms(r['shift'] - c['layer_shift'][l]))
    print('rms position error: joint %.4f px, single layers %s px, start %.4f px' %
          (rms(joint['shift']), ', '.join('%.4f' % v for v in single), rms(c['shift'])))
    assert rms(joint['shift']) < min(single) < rms(c['shift'])


def _two_stars(ls, scale=(1.0, 1.0), start_off=((0.3, 0.0), (0.0, 0.0)), noise=0.0):
    base = F.Y.models()
    nl = len(ls)
    psf = np.ascontiguousarray(np.stack([np.roll(base, l, axis=0) for l in range(nl)], axis=1))
    origin, index = np.array([[0, 0], [14, 16]], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    truth = np.array([[0.2, -0.1], [0.0, 0.3]])
    rng = np.random.default_rng(3)
    cube = np.stack([F.Y.render(None, np.ascontiguousarray(psf[:, l]), index, origin, truth + ls[l],
                                np.array([1000.0, 500.0]) * np.asarray(scale[l]), shape=(64, 64))[0]
                     + noise * rng.normal(size=(64, 64)) for l in range(nl)])
    return cube, psf, index, origin, truth, truth + np.array(start_off)


def test_the_rule_on_cases_written_out_by_hand():
    ls = np.array([[0.0, 0.0], [0.11, -0.07]])
    cube, psf, index, origin, truth, start = _two_stars(ls)
    kw = dict(radius=6.0, background=False)
    r = R.refine(cube, None, psf, index, origin, start, ls, max_outer=0, **kw)
    assert r['nouter'] == 0 and r['posok'] and np.array_equal(r['shift'], start) and not r['flags'].any()
    r = R.refine(cube, None, psf, index, origin, start, ls, max_outer=12, pos_tol=1e-9, **kw)
    assert r['posok'] and np.abs(r['shift'] - truth).max() < 1e-9 and r['carried'].all() and r['status'] == 0
    r = R.refine(cube, None, psf, index, origin, start, ls, max_outer=1, max_step=0.05, **kw)
    assert r['shift'][0, 0] == start[0, 0] - 0.05 and r['flags'][0] == R.CLIPPED and r['status'] == 1
    # nobody free
    r = R.refine(cube, None, psf, index, origin, start, ls, min_snr=1e12, **kw)
    assert r['nouter'] == 0 and r['posok'] and list(r['flags']) == [R.HELD, R.HELD] and not r['err_shift'].any()
    # carried in one layer only: star 1 at 1 / 1000 of its flux in layer 1, under the noise there
    cube, psf, index, origin, truth, start = _two_stars(ls, scale=((1.0, 1.0), (1.0, 1e-3)), noise=1.0)
    r = R.refine(cube, None, psf, index, origin, start, ls, max_outer=1, **kw)
    assert r['carried'].tolist() == [[True, True], [True, False]] and list(r['nfree']) == [1, 1]
    assert np.all(r['err_shift'] > 0) and not r['flags'].any()
    # ... and with layer 0 all NaN the star is free in no layer: held, while star 0 moves
    dead = cube.copy()
    dead[0] = np.nan
    r = R.refine(dead, None, psf, index, origin, start, ls, max_outer=1, **kw)
    assert r['problem'].live == [1] and list(r['nfree']) == [1, 0] and list(r['flags']) == [0, R.HELD]
    assert np.array_equal(r['shift'][1], start[1]) and r['closing'][0] is None
    # the dof rule: one star on a 1 x 2 frame is free with three layers and held with one
    psf1 = np.ascontiguousarray(np.stack([F.Y.models()[:1]] * 3, axis=1))
    tiny = np.array([[[3.5, 2.5]], [[7.2, 4.9]], [[1.7, 1.3]]])
    og, ix = np.array([[-20, -20]], dtype=np.int32), np.zeros(1, dtype=np.int32)
    off = np.array([[0.3, 0.4]])                 # (at a zero shift the y column of the symmetric model vanishes on row 0)
    r = R.refine(tiny, None, psf1, ix, og, off, None, 1.0, False, max_outer=1, min_snr=0.0)
    assert r['nfree_last'] == 1 and r['nouter'] == 1
    r = R.refine(tiny[:1], None, np.ascontiguousarray(psf1[:, :1]), ix, og, off, None, 1.0, False, max_outer=1, min_snr=0.0)
    assert r['nfree_last'] == 0 and r['nouter'] == 0 and r['posok'] and list(r['flags']) == [R.HELD]
    # the across-layer +-8 bound
    lo, hi = R.shift_interval(np.array([[0.0, 0.0], [0.5, -0.25]]))
    assert list(hi) == [7.5, 8.0] and list(lo) == [-8.0, -7.75] and R.shift_interval(None)[1].tolist() == [8.0, 8.0]
    odd = np.array([[0.0, 0.0], [0.1 + 0.2, -1.0 / 3.0], [1e-17, 3.0]])
    lo, hi = R.shift_interval(odd)
    assert np.all(np.abs(hi + odd) <= 8.0) and np.all(np.abs(lo + odd) <= 8.0)
    assert hi[1] == 5.0 and abs(hi[0] - 7.7) < 1e-14 and list(lo) == [-8.0, -8.0 + 1.0 / 3.0]


# ---- 2. what reaches C
@pytest.fixture
def ctx():
    c = make_ctx()
    yield c
    c._h = None


def test_fit_cube_psf_free_host_form(ctx):
    c = Q.cube(True)
    n, nl = c['n'], Q.NL
    rows, pos, shifts, head, call = ctx.fit_cube_psf_free(c['cube'], c['psf'], c['origin'], var=c['var'], shift=c['shift'],
                                                          layer_shift=c['layer_shift'], psf_index=c['index'])
    assert rows.shape == (nl, n, _lib.NFRAMEFIT) and head.shape == (nl, _lib.NFRAMEFIT) and shifts.shape == (n, 2)
    assert pos.shape == (n, _lib.NCUBEFREE_POS) and call.shape == (_lib.NCUBEFREE_CALL,)
    name, a = ctx.lib.calls[0]
    assert name == 'mpsfr_fit_cube_psf_free' and len(a) == 30 and len(ctx.lib.calls) == 1 and a[A_CTX].value == HANDLE
    assert (a[A_NL], a[A_NY], a[A_NX], a[A_NSTAR], a[A_NPSF], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL]) == \
        (nl, 97, 150, n, 4, 8.0, _lib.FIT_BACKGROUND, 100, 1e-10)
    assert (a[A_OUTER], a[A_POSTOL], a[A_STEP], a[A_MOVE], a[A_SNR], a[A_ONDEV]) == (8, 1e-3, 0.5, 2.0, 3.0, 0)
    assert all(isinstance(a[i], int) and not isinstance(a[i], bool)
               for i in (A_NL, A_NY, A_NX, A_NSTAR, A_NPSF, A_FLAGS, A_MAXIT, A_OUTER, A_ONDEV))
    assert all(isinstance(a[i], float) for i in (A_RADIUS, A_TOL, A_POSTOL, A_STEP, A_MOVE, A_SNR))
    assert a[A_SCALE0] is None and a[A_RESID] is None
    assert (a[A_ROWS].value, a[A_HEAD].value, a[A_POS].value, a[A_SHOUT].value, a[A_CALL].value) == \
        (rows.ctypes.data, head.ctypes.data, pos.ctypes.data, shifts.ctypes.data, call.ctypes.data)
    np.testing.assert_array_equal(_array(a[A_ORIGIN], 2 * n, C.c_int32, np.int32).reshape(n, 2), c['origin'])
    np.testing.assert_array_equal(_array(a[A_INDEX], n, C.c_int32, np.int32), c['index'])
    np.testing.assert_array_equal(_array(a[A_SHIFT], 2 * n, C.c_double, np.float64).reshape(n, 2), c['shift'])
    np.testing.assert_array_equal(_array(a[A_LSHIFT], 2 * nl, C.c_double, np.float64).reshape(nl, 2), c['layer_shift'])
    np.testing.assert_array_equal(_array(a[A_VAR], nl * 97 * 150, C.c_double, np.float64).reshape(nl, 97, 150), c['var'])
    np.testing.assert_array_equal(_array(a[A_PSF], 4 * nl * NS * NS, C.c_double, np.float64).reshape(c['psf'].shape),
                                  c['psf'])
    got = _array(a[A_CUBE], nl * 97 * 150, C.c_double, np.float64).reshape(nl, 97, 150)
    assert np.array_equal(got, c['cube'], equal_nan=True)
    # lists, one model per star, the optional arrays and parameters
    ctx.lib.calls.clear()
    one = np.ascontiguousarray(np.broadcast_to(c['psf'][:1], (n, nl, NS, NS)))
    out = ctx.fit_cube_psf_free(c['cube'].tolist(), one, c['origin'].tolist(), scale0=np.arange(nl * n).reshape(nl, n),
                                radius=4, background=False, max_iter=1000, tol=np.float32(0.5), max_outer=16,
                                pos_tol=np.float32(0.25), max_step=1, max_move=4, min_snr=0, return_residual=True)
    a = ctx.lib.calls[0][1]
    assert len(out) == 6 and out[5].shape == (nl, 97, 150) and a[A_RESID].value == out[5].ctypes.data
    assert (a[A_NPSF], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL]) == (n, 4.0, 0, 1000, 0.5)
    assert (a[A_OUTER], a[A_POSTOL], a[A_STEP], a[A_MOVE], a[A_SNR]) == (16, 0.25, 1.0, 4.0, 0.0)
    assert all(a[i] is None for i in (A_VAR, A_INDEX, A_SHIFT, A_LSHIFT))
    np.testing.assert_array_equal(_array(a[A_SCALE0], nl * n, C.c_double, np.float64), np.arange(nl * n))


def test_fit_cube_psf_free_device_form(ctx):
    assert ctx.fit_cube_psf_free_device(7, 97, 150, DEV['image'], 4096, 4096, DEV['psf'], DEV['origin'], DEV['rows'],
                                        DEV['out'], DEV['scale'], DEV['shift'], DEV['vstamps']) is None
    name, a = ctx.lib.calls[0]
    assert name == 'mpsfr_fit_cube_psf_free' and len(a) == 30 and a[A_ONDEV] == 1
    assert (a[A_NL], a[A_NY], a[A_NX], a[A_NSTAR], a[A_NPSF], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL]) == \
        (7, 97, 150, 4096, 4096, 8.0, 1, 100, 1e-10)
    assert (a[A_OUTER], a[A_POSTOL], a[A_STEP], a[A_MOVE], a[A_SNR]) == (8, 1e-3, 0.5, 2.0, 3.0)
    assert (a[A_CUBE].value, a[A_PSF].value, a[A_ORIGIN].value, a[A_ROWS].value, a[A_HEAD].value, a[A_POS].value,
            a[A_SHOUT].value, a[A_CALL].value) == (DEV['image'], DEV['psf'], DEV['origin'], DEV['rows'], DEV['out'],
                                                   DEV['scale'], DEV['shift'], DEV['vstamps'])
    assert all(a[i] is None for i in (A_VAR, A_INDEX, A_SHIFT, A_LSHIFT, A_SCALE0, A_RESID))
    ctx.lib.calls.clear()
    ctx.fit_cube_psf_free_device(_lib.CUBE_FIT_MAX_LAYERS, 1, 1, DEV['image'], 1000, 1000, DEV['psf'], DEV['origin'],
                                 DEV['rows'], DEV['out'], DEV['scale'], DEV['shift'], DEV['vstamps'], var_ptr=DEV['var'],
                                 shift_ptr=DEV['shift'], layer_shift_ptr=DEV['vstamps'], psf_index_ptr=DEV['index'],
                                 scale0_ptr=DEV['scale'], resid_ptr=DEV['stamps'], radius=20, background=False, max_iter=1,
                                 tol=0.999, max_outer=0, pos_tol=1e-300, max_step=1e-300, max_move=1e-300, min_snr=1e300)
    a = ctx.lib.calls[0][1]
    assert (a[A_VAR].value, a[A_INDEX].value, a[A_SHIFT].value, a[A_LSHIFT].value, a[A_SCALE0].value,
            a[A_RESID].value) == (DEV['var'], DEV['index'], DEV['shift'], DEV['vstamps'], DEV['scale'], DEV['stamps'])
    assert (a[A_NL], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL], a[A_OUTER], a[A_POSTOL], a[A_STEP], a[A_MOVE],
            a[A_SNR]) == (4096, 20.0, 0, 1, 0.999, 0, 1e-300, 1e-300, 1e-300, 1e300)


def test_fit_cube_psf_free_refuses(ctx):
    c = Q.cube(True)
    n, nl = c['n'], Q.NL
    base = dict(cube=c['cube'], psf=c['psf'], origin=c['origin'], var=None, shift=None, layer_shift=None,
                psf_index=c['index'], scale0=None, radius=8.0, background=True, max_iter=100, tol=1e-10,
                return_residual=False)
    shift = np.zeros((n, 2))
    far, nan, edge = shift.copy(), shift.copy(), shift.copy()
    far[3, 1], nan[0, 0], edge[5, 0] = 8.5, np.nan, 7.9          # edge: legal alone, beyond 8 with the offset of a layer
    ls = c['layer_shift']
    ls_nan, ls_far = ls.copy(), ls.copy()
    ls_nan[2, 0], ls_far[1, 1] = np.nan, -8.01
    bad = [dict(cube=c['cube'][0]), dict(cube='x'), dict(cube=np.zeros((0, 3, 3))), dict(var=c['var'][:2]), dict(var='v'),
           dict(psf=c['psf'][:, :2]), dict(psf=c['psf'][:, :, :39]), dict(psf=c['psf'][0]), dict(psf='p'),
           dict(psf_index=None), dict(psf_index=np.full(n, 4)), dict(psf_index=np.zeros(n - 1, dtype=int)),
           dict(origin=c['origin'][:, :1]), dict(origin=np.full((n, 2), 2 ** 30 + 1)),
           dict(shift=far), dict(shift=nan), dict(shift=shift[:-1]),
           dict(layer_shift=ls_nan), dict(layer_shift=ls_far), dict(layer_shift=ls[:2]), dict(layer_shift='l'),
           dict(shift=edge, layer_shift=ls),
           dict(scale0=np.zeros(n)), dict(scale0=np.full((nl, n), np.inf)), dict(scale0=np.zeros((n, nl))),
           dict(radius=0.99), dict(radius=20.01), dict(radius=np.nan), dict(tol=0.0), dict(tol=1.0), dict(max_iter=0),
           dict(max_iter=1001), dict(background=1), dict(return_residual=1), dict(layer_batch=0)] + FREE_BAD
    for kw in bad:
        args = dict(base)
        args.update(kw)
        cu, ps, og = args.pop('cube'), args.pop('psf'), args.pop('origin')
        with pytest.raises((ValueError, TypeError) if 'layer_batch' in kw else ValueError):
            ctx.fit_cube_psf_free(cu, ps, og, **args)
    # all layers are resident: a call above the budget of work memory is refused, as C refuses it
    big = np.broadcast_to(np.zeros((1, 1, 1)), (40, 4096, 4096))               # (no memory behind it)
    with pytest.raises(ValueError, match='work memory'):
        ctx.fit_cube_psf_free(big, np.zeros((1, 40, NS, NS)), [[0, 0]])
    with pytest.raises(ValueError, match='work memory'):
        ctx.fit_cube_psf_free_device(64, 4096, 4096, 1, 10, 1, 1, 1, 1, 1, 1, 1, 1, psf_index_ptr=1)
    assert _lib.cube_free_work(64, 320, 320, 2000) < _lib.CUBE_FREE_WORK_BYTES // 30
    ok = (3, 97, 150, 1, 10, 1, 1, 1, 1, 1, 1, 1, 1)
    for k, v in [(0, 0), (0, _lib.CUBE_FIT_MAX_LAYERS + 1), (0, 3.0), (0, True), (1, 0), (2, 16385), (1, 97.0), (3, 0),
                 (4, 0), (4, 2 ** 20 + 1), (4, True), (5, 0), (6, 0), (7, 0), (8, 0), (9, None), (10, 0), (11, None),
                 (12, 0), (3, None)]:
        a = list(ok)
        a[k] = v
        with pytest.raises(ValueError):
            ctx.fit_cube_psf_free_device(*a, psf_index_ptr=1)
    with pytest.raises(ValueError):
        ctx.fit_cube_psf_free_device(*ok)                            # npsf != nstar without psf_index_ptr
    for kw in [dict(radius=0.5), dict(tol=0), dict(max_iter=0), dict(background=0)] + FREE_BAD:
        with pytest.raises(ValueError):
            ctx.fit_cube_psf_free_device(*ok, psf_index_ptr=1, **kw)
    assert ctx.lib.calls == []
    # the edges themselves are legal: a summed shift of exactly 8, the most layers
    ctx.fit_cube_psf_free(c['cube'], c['psf'], c['origin'], psf_index=c['index'], shift=np.full((n, 2), 7.5),
                          layer_shift=np.full((nl, 2), 0.5))
    ctx.fit_cube_psf_free_device(4096, 64, 64, 1, 2 ** 10, 1, 1, 1, 1, 1, 1, 1, 1, psf_index_ptr=1, radius=1, tol=1e-300,
                                 max_iter=1000, max_outer=16, max_step=1.0, max_move=4.0, min_snr=0)
    assert len(ctx.lib.calls) == 2


# ---- 3. psfrec against an answering stub
CALL = (321.0, 4000.0, 5.0, 2e-4, 3.0, 40.0, 0.0, 1e-11)


class CubeFreeLib(CubeLib):
    """CubeLib whose mpsfr_fit_cube_psf_free answers in the rows and heads as its mpsfr_fit_cube_psf does, moves every
    star by (+0.125, -0.25) px (errors 0.5 and 0.25 px, flags 4, free in 3 steps; star 1 of three or more held: it keeps
    its shift, flags 1) and returns CALL."""

    def mpsfr_fit_cube_psf_free(self, *a):
        cube_args = a[:A_OUTER] + (0,) + a[A_ROWS:A_POS] + (a[A_RESID], a[A_ONDEV])
        CubeLib.mpsfr_fit_cube_psf(self, *cube_args)
        self.calls[-1] = ('mpsfr_fit_cube_psf_free', a)
        n = a[A_NSTAR]
        sh = _array(a[A_SHIFT], 2 * n, C.c_double, np.float64).reshape(n, 2)
        pos = _array(a[A_POS], 8 * n, C.c_double, np.float64).reshape(n, 8)
        pos[:, :2] = sh + (0.125, -0.25)
        pos[:, 2:] = (0.5, 0.25, 0.125, -0.25, 4.0, 3.0)
        if n >= 3:
            pos[1] = (sh[1, 0], sh[1, 1], 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        _array(a[A_SHOUT], 2 * n, C.c_double, np.float64).reshape(n, 2)[:] = pos[:, :2]
        _array(a[A_CALL], 8, C.c_double, np.float64)[:] = CALL
        return 0


def _free_ctx(monkeypatch):
    ctx = make_ctx()
    ctx.lib = CubeFreeLib()
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: ctx)
    return ctx


def test_refine_crowded_spectra_table(monkeypatch):
    ctx = _free_ctx(monkeypatch)
    pos = np.array([[10.4, 20.5], [30.5, 7.25], [-3.0, 12.75], [50.0, 60.0]])
    nl, n = 3, 4
    cube = np.arange(nl * 70.0 * 80).reshape(nl, 70, 80)
    psf = np.stack([F.Y.models()[l] for l in range(nl)])
    found = {'position': pos, 'scale': np.array([5.0, 6.0, 7.0, 8.0])}
    lbda = [500.0, 600.0, 700.0]
    dar = np.array([[0.0, 0.0], [0.05, -0.025], [0.1, -0.05]])               # arcsec
    fit, origin, resid = psfrec.refine_crowded_spectra(
        cube, psf, found, lbda=lbda, layer_shift=dar, start='found', radius=6, fit_back=False, max_iter=50, tol=1e-8,
        max_outer=5, pos_tol=1e-2, max_step=0.25, max_move=1.5, min_snr=4, return_residual=True, pixscale=0.25)
    assert tuple(fit.colnames) == psfrec._FIT_COLS_REFINED_SPECTRA
    assert set(psfrec._FIT_COLS_CROWDED_SPECTRA) | {'position', 'err_shift', 'moved', 'free', 'flags'} == set(fit.colnames)
    want = (np.rint(pos) - 20).astype(np.int32)
    assert origin.dtype == np.int32 and np.array_equal(origin, want)
    sh = pos - (want + 20)
    assert [c[0] for c in ctx.lib.calls] == ['mpsfr_fit_cube_psf_free']
    a = ctx.lib.calls[0][1]
    assert (a[A_NL], a[A_NY], a[A_NX], a[A_NSTAR], a[A_NPSF], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL], a[A_ONDEV]) \
        == (nl, 70, 80, n, 1, 6.0, 0, 50, 1e-8, 0)
    assert (a[A_OUTER], a[A_POSTOL], a[A_STEP], a[A_MOVE], a[A_SNR]) == (5, 1e-2, 0.25, 1.5, 4.0)
    np.testing.assert_array_equal(_array(a[A_SCALE0], nl * n, C.c_double, np.float64).reshape(nl, n),
                                  np.tile([5.0, 6.0, 7.0, 8.0], (nl, 1)))
    np.testing.assert_array_equal(_array(a[A_SHIFT], 2 * n, C.c_double, np.float64).reshape(n, 2), sh)
    np.testing.assert_array_equal(_array(a[A_LSHIFT], 2 * nl, C.c_double, np.float64).reshape(nl, 2), dar / 0.25)
    keep = np.array([True, False, True, True])
    moved = sh + np.where(keep[:, None], (0.125, -0.25), 0.0)
    np.testing.assert_array_equal(fit['shift'], moved * 0.25)
    np.testing.assert_array_equal(fit['position'], (want + 20) + moved)
    np.testing.assert_array_equal(np.asarray(fit['err_shift']), np.where(keep[:, None], (0.5 * 0.25, 0.25 * 0.25), 0.0))
    np.testing.assert_array_equal(np.asarray(fit['moved']), np.where(keep[:, None], (0.125 * 0.25, -0.25 * 0.25), 0.0))
    np.testing.assert_array_equal(fit['flags'], [4, 1, 4, 4])
    np.testing.assert_array_equal(fit['free'], [3, 0, 3, 3])
    F0 = (1000.0 * sh[:, 0] + sh[:, 1])[:, None] + 1e6 * np.arange(nl)[None, :]
    fitted = np.ones((n, nl), dtype=bool)
    fitted[1, 1] = False
    for name in ('scale', 'flux', 'err_scale', 'err_flux', 'overlap', 'npix', 'status'):
        assert np.asarray(fit[name]).shape == (n, nl), name
    np.testing.assert_array_equal(np.asarray(fit['scale'])[fitted], F0[fitted])
    np.testing.assert_array_equal(np.asarray(fit['status']), np.where(fitted, 0, 2))
    assert all(np.asarray(fit[k]).dtype == np.int64 for k in ('npix', 'free', 'flags', 'status'))
    meta = dict(fit.meta)
    assert sorted(meta) == sorted(psfrec._META_CROWDED_SPECTRA + psfrec._META_REFINED_SPECTRA + ('position_layers', 'lbda'))
    np.testing.assert_array_equal(meta['iterations'], [9, 10, 11])
    np.testing.assert_array_equal(meta['status'], [0, 0, 1])
    np.testing.assert_array_equal(meta['position_layers'], [0, 1, 2])
    assert tuple(meta[k] for k in psfrec._META_REFINED_SPECTRA) == CALL
    assert all(isinstance(meta[k], int) for k in ('outer', 'nfree', 'inner', 'call_status'))
    assert np.array_equal(resid, cube)
    # the defaults; a slice that names every layer is the whole cube
    ctx.lib.calls.clear()
    four = np.ascontiguousarray(np.broadcast_to(F.Y.models()[:, None], (4, nl, NS, NS)))
    fit, origin = psfrec.refine_crowded_spectra(cube, four, pos, var=np.ones((nl, 70, 80)), position_layers=slice(None))
    a = ctx.lib.calls[0][1]
    assert len(ctx.lib.calls) == 1 and (a[A_NPSF], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL]) == (4, 8.0, 1, 100, 1e-10)
    assert (a[A_OUTER], a[A_POSTOL], a[A_STEP], a[A_MOVE], a[A_SNR]) == (8, 1e-3, 0.5, 2.0, 3.0)
    assert all(a[i] is None for i in (A_INDEX, A_SCALE0, A_LSHIFT, A_RESID)) and a[A_VAR] is not None
    assert 'lbda' not in fit.meta
    ctx._h = None


def test_refine_crowded_spectra_with_position_layers(monkeypatch):
    ctx = _free_ctx(monkeypatch)
    pos = np.array([[10.4, 20.5], [30.5, 7.25], [-3.0, 12.75], [50.0, 60.0]])
    nl, n = 5, 4
    cube = np.arange(nl * 70.0 * 80).reshape(nl, 70, 80)
    var = cube + 1.0
    psf = np.stack([np.roll(F.Y.models(), l, axis=0) for l in range(nl)], axis=1)         # (4, nl, 40, 40)
    dar = np.stack([0.01 * np.arange(nl), -0.02 * np.arange(nl)], axis=1)
    start = np.arange(nl * n, dtype=float).reshape(nl, n)
    sel = [3, 1]
    fit, origin, resid = psfrec.refine_crowded_spectra(
        cube, psf, pos, var=var, psf_index=[0, 1, 2, 3], layer_shift=dar, start=start, position_layers=sel,
        return_residual=True, pixscale=0.25, max_outer=3)
    assert [c[0] for c in ctx.lib.calls] == ['mpsfr_fit_cube_psf_free', 'mpsfr_fit_cube_psf']
    want = (np.rint(pos) - 20).astype(np.int32)
    sh = pos - (want + 20)
    a = ctx.lib.calls[0][1]
    # the position call sees the chosen layers alone, in the order given, and asks for no residual
    assert (a[A_NL], a[A_NY], a[A_NX], a[A_NSTAR], a[A_NPSF], a[A_OUTER]) == (2, 70, 80, n, 4, 3) and a[A_RESID] is None
    np.testing.assert_array_equal(_array(a[A_CUBE], 2 * 70 * 80, C.c_double, np.float64).reshape(2, 70, 80), cube[sel])
    np.testing.assert_array_equal(_array(a[A_VAR], 2 * 70 * 80, C.c_double, np.float64).reshape(2, 70, 80), var[sel])
    np.testing.assert_array_equal(_array(a[A_PSF], 4 * 2 * NS * NS, C.c_double, np.float64).reshape(4, 2, NS, NS),
                                  psf[:, sel])
    np.testing.assert_array_equal(_array(a[A_LSHIFT], 4, C.c_double, np.float64).reshape(2, 2), dar[sel] / 0.25)
    np.testing.assert_array_equal(_array(a[A_SCALE0], 2 * n, C.c_double, np.float64).reshape(2, n), start[sel])
    np.testing.assert_array_equal(_array(a[A_SHIFT], 2 * n, C.c_double, np.float64).reshape(n, 2), sh)
    # the refined shifts go straight into the flux-only solve of the whole cube
    b = ctx.lib.calls[1][1]
    keep = np.array([True, False, True, True])
    moved = sh + np.where(keep[:, None], (0.125, -0.25), 0.0)
    assert (b[1], b[2], b[3], b[6], b[7]) == (nl, 70, 80, n, 4)
    np.testing.assert_array_equal(_array(b[11], 2 * n, C.c_double, np.float64).reshape(n, 2), moved)
    np.testing.assert_array_equal(_array(b[12], 2 * nl, C.c_double, np.float64).reshape(nl, 2), dar / 0.25)
    np.testing.assert_array_equal(_array(b[13], nl * n, C.c_double, np.float64).reshape(nl, n), start)
    np.testing.assert_array_equal(fit['shift'], moved * 0.25)
    F0 = (1000.0 * moved[:, 0] + moved[:, 1])[:, None] + 1e6 * np.arange(nl)[None, :]
    fitted = np.ones((n, nl), dtype=bool)
    fitted[1, 1] = False
    np.testing.assert_array_equal(np.asarray(fit['scale'])[fitted], F0[fitted])
    assert np.asarray(fit['scale']).shape == (n, nl) and np.array_equal(resid, cube)
    np.testing.assert_array_equal(fit.meta['position_layers'], sel)
    np.testing.assert_array_equal(fit.meta['iterations'], 9 + np.arange(nl))
    assert fit.meta['outer'] == 5 and fit.meta['chi2_all'] == CALL[0]
    # a slice, a masked cube
    ctx.lib.calls.clear()
    psfrec.refine_crowded_spectra(np.ma.masked_less(cube, 2.0), psf, pos, psf_index=[0, 1, 2, 3],
                                  position_layers=slice(0, nl, 2))
    a = ctx.lib.calls[0][1]
    assert a[A_NL] == 3 and np.isnan(_array(a[A_CUBE], 2, C.c_double, np.float64)).all()
    # refusals, before any call
    ctx.lib.calls.clear()
    for kw in [dict(position_layers=[5]), dict(position_layers=[]), dict(position_layers=[1, 1]),
               dict(position_layers='a'), dict(position_layers=[[0, 1]]), dict(position_layers=[0], start=np.zeros((2, n))),
               dict(position_layers=[0], layer_shift=np.zeros((2, 2))), dict(radius=0.5), dict(fit_back=1),
               dict(start='find'), dict(max_iter=0), dict(tol=1.0), dict(pixscale=0.0), dict(return_residual=None),
               dict(lbda=[1.0, 2.0])] + FREE_BAD:
        with pytest.raises(ValueError):
            psfrec.refine_crowded_spectra(cube, psf, pos, psf_index=[0, 1, 2, 3], **kw)
    with pytest.raises(ValueError):
        psfrec.refine_crowded_spectra(cube[:4], psf, pos, psf_index=[0, 1, 2, 3], position_layers=[0])
    assert ctx.lib.calls == []
    ctx._h = None


# ---- 4. constants and exports
def test_exports_and_header_constants():
    assert 'mpsfr_fit_cube_psf_free' in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    for name, val in (('NCUBEFREE_POS', _lib.NCUBEFREE_POS), ('NCUBEFREE_CALL', _lib.NCUBEFREE_CALL)):
        assert int(re.search(r'#define MPSFR_%s\s+(\d+)' % name, hdr).group(1)) == val == 8, name
    assert re.search(r'#define MPSFR_CUBE_FREE_WORK_BYTES\s+\(\(size_t\)4 << 30\)', hdr)
    assert _lib.CUBE_FREE_WORK_BYTES == 4 << 30
    assert re.search(r'int mpsfr_fit_cube_psf_free\(mpsfr_ctx\* ctx, int nl, int ny, int nx, const double\* cube', hdr)
    assert 'is the follow-up' not in hdr
    # the work memory the header states is what the Python layer counts
    m = re.search(r'per layer two frames of\s+\* doubles, (\d+) nstar \+ (\d+) ceil\(ny nx / 4096\) \+ (\d+) doubles and '
                  r'(\d+) nstar \+ (\d+) int32; once (\d+) nstar \+ (\d+) doubles and\s+\* (\d+) nstar \+ (\d+) int32', hdr)
    assert m and [int(v) for v in m.groups()] == [25, 8, 17, 4, 5, 14, 10, 5, 11]
    nl, ny, nx, n = 3, 97, 150, 34
    nt, nchunk = 4 * 5, 4
    lists = 4 * (3 * nt + 1 + 10 * n)
    assert _lib.cube_free_work(nl, ny, nx, n) == (lists + 7) // 8 * 8 + 8 * (nl * (2 * ny * nx + 25 * n + 8 * nchunk + 17)
                                                                            + 14 * n + 10) + 4 * (nl * (4 * n + 5) + 5 * n + 11)
    import muse_psfr_amd
    for name in ('refine_crowded_spectra', 'NCUBEFREE_POS', 'NCUBEFREE_CALL', 'CUBE_FREE_WORK_BYTES'):
        assert hasattr(muse_psfr_amd, name), name
    assert 'refine_crowded_spectra' in muse_psfr_amd.__doc__
    build = __import__('muse_psfr_amd._build', fromlist=['SOURCES'])
    assert 'cube_free.hip' in build.SOURCES and 'frame_free_impl.h' in build.HEADERS
    for f in ('cube_free.hip', 'frame_free_impl.h'):
        src = open(os.path.join(ROOT, 'muse_psfr_amd', 'csrc', f)).read()
        assert 'atomicAdd' not in src                          # no floating-point atomics: every sum has a fixed order
    free = open(os.path.join(ROOT, 'muse_psfr_amd', 'csrc', 'frame_free.hip')).read()
    assert 'k_fr_walk<false>' in free and 'k_fr_project<true, false>' in free
