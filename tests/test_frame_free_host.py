"""Host: the crowded-field fit with free positions (mpsfr_fit_frame_psf_free) without a GPU.

1. the yardstick (frame_free_ref) checked on itself: the analytic derivative columns against central differences of
   render_ref.window; the noiseless displaced scene is recovered to the bound where every lit star is fitted (radius 8);
   the contraction rho of the noiseless scene is below 1/2 in the eight cases of the GPU parity test -- the condition
   the choice of the draw has to meet --, and the steps the parity tolerance asks of the inner solves stay below its
   max_iter; with noise every position pull is at most 4 conditional sigma for the stars with overlap < 0.5.
2. what Context.fit_frame_psf_free and its device form hand to C, every refusal of the Python layer before any library
   call (the recording stub of test_render_host.py).
3. psfrec.refine_crowded_stars and fit_found_stars(crowded='free') against an answering stub.
4. the constants against the header, the exports, the build list.
"""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import frame_fit_ref as F
import frame_free_ref as G
import group_ref as GR
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec
from test_frame_fit_host import FrameLib
from test_group_host import _array, crowd
from test_render_host import DEV, HANDLE, make_ctx

NS = 40
TOL, MAX_ITER = 1e-12, 100            # of the parity runs of tests/test_gpu_frame_free.py
CASES = list(itertools.product((True, False), (True, False), (4.0, 8.0)))


# ---- 1. the yardstick
def test_derivative_columns_agree_with_central_differences():
    rng = np.random.default_rng(2)
    h = 1e-5
    for P in F.Y.models():
        for _ in range(4):
            dp, dq = rng.uniform(-7.9, 7.9, 2)
            if min(abs(v - round(v)) for v in (dp, dq)) < 0.01:          # away from integer shifts: c' has a kink there
                continue
            w, wy, wx = G.windows(P, dp, dq)
            assert np.array_equal(w, F.Y.window(P, dp, dq))
            ny = (F.Y.window(P, dp + h, dq) - F.Y.window(P, dp - h, dq)) / (2 * h)
            nx = (F.Y.window(P, dp, dq + h) - F.Y.window(P, dp, dq - h)) / (2 * h)
            # the Keys kernel is a cubic between the knots: the central difference is off by h^2 / 6 times its third
            # derivative, at most 9 in modulus, times sum |P| = 1 along the axis; and by the rounding eps max|P| / h
            tol = 1.5 * h * h * np.abs(P).max() * 16 + 4 * F.EPS * np.abs(P).max() * 16 / h
            assert np.max(np.abs(wy - ny)) <= tol and np.max(np.abs(wx - nx)) <= tol
            assert np.abs(wy).max() > 1e3 * tol and np.abs(wx).max() > 1e3 * tol
    # on the 40 stamp rows the columns are those of psf_fit_ref.model's Jacobian
    P = F.Y.models()[1]
    m, jac = G.F.Y.R.model(P, (1.0, 0.3, -0.45, 0.0), jac=True)
    w, wy, wx = G.windows(P, 0.3, -0.45)
    a = slice(G.APRON, G.APRON + NS)
    assert np.allclose(w[a, a], m, atol=1e-17) and np.allclose(wy[a, a], jac[..., 1], atol=1e-16)
    assert np.allclose(wx[a, a], jac[..., 2], atol=1e-16)


def test_displaced_scene_is_what_the_tests_need():
    s, t = G.displaced_scene(False), F.scene(False)
    d = s['shift'] - s['truth']
    assert np.array_equal(s['truth'], t['shift']) and np.array_equal(s['origin'], t['origin'])
    assert 0.25 < np.abs(d).max() <= 0.3 and np.abs(s['shift']).max() <= 8.0 and abs(d.mean()) < 0.1
    assert np.array_equal(G.displaced_scene(True)['shift'], s['shift'])


@pytest.mark.parametrize('with_var,background,radius', CASES)
def test_contraction_is_below_one_half_and_the_inner_solves_fit(with_var, background, radius):
    conv = G.scene_converged(with_var, background, radius, False, max_outer=10)
    assert conv['rho'] < 0.5, conv['steps']
    assert conv['steps'][-1] < 1e-10 and len(conv['last']['free_idx']) == conv['problem'].nacc
    assert G.pcg_steps(conv['last'], TOL, MAX_ITER) <= MAX_ITER
    # pos_tol of the parity run: at least ten times the inner term, no step of the yardstick within a tenth of it, and
    # small enough to leave the loop three steps and more
    inner = G.position_bounds(conv, 1.0, TOL, MAX_ITER)[1]
    pos_tol = G.parity_pos_tol(conv, TOL, MAX_ITER)
    steps = np.array(conv['steps'])
    assert 10.0 * inner.max() <= pos_tol < 0.1 and not np.any(np.abs(steps - pos_tol) <= 0.1 * pos_tol)
    assert np.argmax(steps <= pos_tol) >= 2


@pytest.mark.parametrize('with_var,background', [(True, True), (True, False), (False, True), (False, False)])
def test_noiseless_scene_is_recovered_to_the_bound(with_var, background):
    # (radius 8: every lit star is accepted, so the truth has a zero residual and is the minimiser; at radius 4 the
    # two stars at the frame's edge are left out and their light stays in the frame)
    s = G.displaced_scene(False)
    conv = G.scene_converged(with_var, background, 8.0, False, max_outer=10)
    acc, fi = conv['problem'].acc, conv['last']['free_idx']
    assert conv['problem'].nacc == s['n'] - 2
    # the yardstick's own error: the reference and right-side terms of the inner bound (no iteration: tol = 0, k = 0)
    _, by, bx = G.inner_bounds(conv['last'], 0.0, 0)
    err = np.abs(conv['shift'][acc][fi] - s['truth'][acc][fi])
    assert np.all(err <= np.stack([by, bx], axis=1)) and err.max() < 1e-9
    assert np.allclose(conv['closing']['F'], s['flux'][acc], rtol=1e-9)


@pytest.mark.parametrize('radius,background', [(8.0, True), (4.0, False)])
def test_noisy_pulls_stay_within_four_conditional_sigma(radius, background):
    s = G.displaced_scene(True)
    r = G.refine(s['image'], s['var'], s['psf'], s['index'], s['origin'], s['shift'], radius, background)
    acc = r['problem'].acc
    quiet = (r['closing']['overlap'] < 0.5) & (r['nfree'][acc] > 0)
    assert quiet.sum() >= 15
    pull = (r['shift'][acc] - s['truth'][acc])[quiet] / r['err_shift'][acc][quiet]
    assert np.all(np.isfinite(pull)) and np.abs(pull).max() <= 4.0
    # and the fit has moved them towards the truth
    before = np.abs(s['shift'][acc] - s['truth'][acc])[quiet]
    assert np.abs(r['shift'][acc] - s['truth'][acc])[quiet].mean() < before.mean()


def test_the_rule_on_cases_written_out_by_hand():
    psf = F.Y.models()
    origin, index = np.array([[0, 0], [14, 16]], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    truth = np.array([[0.2, -0.1], [0.0, 0.3]])
    image, _, _ = F.Y.render(None, psf, index, origin, truth, [1000.0, 500.0], shape=(64, 64))
    start = truth + np.array([[0.3, 0.0], [0.0, 0.0]])
    kw = dict(radius=6.0, background=False)
    r = G.refine(image, None, psf, index, origin, start, max_outer=0, **kw)
    assert r['nouter'] == 0 and r['posok'] and np.array_equal(r['shift'], start) and not r['flags'].any()
    r = G.refine(image, None, psf, index, origin, start, max_outer=1, max_step=0.05, **kw)
    assert r['shift'][0, 0] == start[0, 0] - 0.05 and r['flags'][0] == G.CLIPPED and r['head_status'] == 1
    r = G.refine(image, None, psf, index, origin, start, max_outer=12, max_move=0.2, pos_tol=1e-9, **kw)
    assert r['shift'][0, 0] == start[0, 0] - 0.2 and r['flags'][0] & G.BOUND and not r['posok'] and r['nouter'] == 12
    r = G.refine(image, None, psf, index, origin, start, min_snr=1e12, **kw)
    assert r['nouter'] == 0 and r['posok'] and list(r['flags']) == [G.HELD, G.HELD] and not r['err_shift'].any()
    r = G.refine(image, None, psf, index, origin, start, max_outer=12, pos_tol=1e-9, **kw)
    assert r['posok'] and np.abs(r['shift'] - truth).max() < 1e-9 and np.all(r['err_shift'] >= 0)
    # Omega stays where the start put it
    assert np.array_equal(r['problem'].omega, F.solve(image, None, psf, index, origin, start, 6.0, False)['omega'])


# ---- 2. what reaches C
@pytest.fixture
def ctx():
    c = make_ctx()
    yield c
    c._h = None


def test_fit_frame_psf_free_host_form(ctx):
    s = F.scene()
    n = s['n']
    rows, shifts, head = ctx.fit_frame_psf_free(s['image'], s['psf'], s['origin'], var=s['var'], shift=s['shift'],
                                                psf_index=s['index'])
    assert rows.shape == (n, _lib.NFRAMEFREE) and shifts.shape == (n, 2) and head.shape == (_lib.NFRAMEFREE_HEAD,)
    name, a = ctx.lib.calls[0]
    assert name == 'mpsfr_fit_frame_psf_free' and len(a) == 26 and len(ctx.lib.calls) == 1 and a[0].value == HANDLE
    assert (a[1], a[2], a[5], a[6], a[12], a[13], a[14], a[15]) == (97, 150, n, 4, 8.0, _lib.FIT_BACKGROUND, 100, 1e-10)
    assert (a[16], a[17], a[18], a[19], a[20], a[25]) == (8, 1e-3, 0.5, 2.0, 3.0, 0)
    assert all(isinstance(a[i], int) and not isinstance(a[i], bool) for i in (1, 2, 5, 6, 13, 14, 16, 25))
    assert all(isinstance(a[i], float) for i in (12, 15, 17, 18, 19, 20))
    assert a[11] is None and a[24] is None
    assert (a[21].value, a[22].value, a[23].value) == (rows.ctypes.data, shifts.ctypes.data, head.ctypes.data)
    np.testing.assert_array_equal(_array(a[9], 2 * n, C.c_int32, np.int32).reshape(n, 2), s['origin'])
    np.testing.assert_array_equal(_array(a[8], n, C.c_int32, np.int32), s['index'])
    np.testing.assert_array_equal(_array(a[10], 2 * n, C.c_double, np.float64).reshape(n, 2), s['shift'])
    np.testing.assert_array_equal(_array(a[4], 97 * 150, C.c_double, np.float64).reshape(97, 150), s['var'])
    ctx.lib.calls.clear()
    out = ctx.fit_frame_psf_free(s['image'].tolist(), s['psf'][0], s['origin'].tolist(), psf_index=[0] * n,
                                 scale0=list(range(n)), radius=4, background=False, max_iter=1000, tol=np.float32(0.5),
                                 max_outer=16, pos_tol=np.float32(0.25), max_step=1, max_move=4, min_snr=0,
                                 return_residual=True)
    a = ctx.lib.calls[0][1]
    assert len(out) == 4 and out[3].shape == F.FRAME and a[24].value == out[3].ctypes.data
    assert (a[6], a[12], a[13], a[14], a[15]) == (1, 4.0, 0, 1000, 0.5) and a[4] is None and a[10] is None
    assert (a[16], a[17], a[18], a[19], a[20]) == (16, 0.25, 1.0, 4.0, 0.0)
    np.testing.assert_array_equal(_array(a[11], n, C.c_double, np.float64), np.arange(n))


def test_fit_frame_psf_free_device_form(ctx):
    assert ctx.fit_frame_psf_free_device(97, 150, DEV['image'], 4096, 4096, DEV['psf'], DEV['origin'], DEV['rows'],
                                         DEV['shift'], DEV['out']) is None
    name, a = ctx.lib.calls[0]
    assert name == 'mpsfr_fit_frame_psf_free' and len(a) == 26 and a[25] == 1
    assert (a[1], a[2], a[5], a[6], a[12], a[13], a[14], a[15]) == (97, 150, 4096, 4096, 8.0, 1, 100, 1e-10)
    assert (a[16], a[17], a[18], a[19], a[20]) == (8, 1e-3, 0.5, 2.0, 3.0)
    assert (a[3].value, a[7].value, a[9].value, a[21].value, a[22].value, a[23].value) == \
        (DEV['image'], DEV['psf'], DEV['origin'], DEV['rows'], DEV['shift'], DEV['out'])
    assert all(a[i] is None for i in (4, 8, 10, 11, 24))
    ctx.lib.calls.clear()
    ctx.fit_frame_psf_free_device(1, 1, DEV['image'], 2 ** 20, 2 ** 20, DEV['psf'], DEV['origin'], DEV['rows'],
                                  DEV['scale'], DEV['out'], var_ptr=DEV['var'], shift_ptr=DEV['shift'],
                                  psf_index_ptr=DEV['index'], scale0_ptr=DEV['scale'], resid_ptr=DEV['stamps'], radius=20,
                                  background=False, max_iter=1, tol=0.999, max_outer=0, pos_tol=1e-300, max_step=1e-300,
                                  max_move=1e-300, min_snr=1e300)
    a = ctx.lib.calls[0][1]
    assert (a[4].value, a[8].value, a[10].value, a[11].value, a[24].value) == \
        (DEV['var'], DEV['index'], DEV['shift'], DEV['scale'], DEV['stamps'])
    assert (a[12], a[13], a[14], a[15], a[16], a[17], a[18], a[19], a[20]) == \
        (20.0, 0, 1, 0.999, 0, 1e-300, 1e-300, 1e-300, 1e300)


FREE_BAD = [dict(max_outer=-1), dict(max_outer=17), dict(max_outer=2.0), dict(max_outer=True), dict(max_outer=None),
            dict(pos_tol=0.0), dict(pos_tol=-1.0), dict(pos_tol=np.nan), dict(pos_tol=np.inf), dict(pos_tol='1'),
            dict(pos_tol=True), dict(max_step=0.0), dict(max_step=1.001), dict(max_step=np.nan), dict(max_step=None),
            dict(max_move=0.0), dict(max_move=4.001), dict(max_move=np.inf), dict(max_move=True),
            dict(min_snr=-0.1), dict(min_snr=np.nan), dict(min_snr=np.inf), dict(min_snr='3')]


def test_fit_frame_psf_free_refuses(ctx):
    s = F.scene()
    image, psf, origin = s['image'], s['psf'], s['origin']
    n = len(origin)
    base = dict(var=None, shift=None, psf_index=np.zeros(n, dtype=int), scale0=None, return_residual=False)
    far = np.zeros((n, 2))
    far[3, 1] = 8.5
    bad = [dict(var=np.ones((3, 3))), dict(psf_index=None), dict(psf_index=np.full(n, 4)), dict(shift=far),
           dict(shift=np.zeros((n - 1, 2))), dict(scale0=np.full(n, np.inf)), dict(scale0=np.zeros(n - 1)),
           dict(radius=0.99), dict(radius=20.01), dict(radius=np.nan), dict(tol=0.0), dict(tol=1.0), dict(max_iter=0),
           dict(max_iter=1001), dict(background=1), dict(return_residual=1)] + FREE_BAD
    for kw in bad:
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError):
            ctx.fit_frame_psf_free(image, psf, origin, **args)
    for im, ps, og in ((image[0], psf, origin), (image, psf[:, :39], origin), (image, psf, origin[:, :1]),
                       (image, psf, np.full((n, 2), 2 ** 30 + 1))):
        with pytest.raises(ValueError):
            ctx.fit_frame_psf_free(im, ps, og, **base)
    ok = (97, 150, 1, 10, 1, 1, 1, 1, 1, 1)
    for k, v in [(0, 0), (1, 16385), (0, 97.0), (2, 0), (3, 0), (3, 2 ** 20 + 1), (3, True), (4, 0), (5, 0), (6, 0),
                 (7, 0), (8, 0), (9, None), (8, None), (2, None)]:
        a = list(ok)
        a[k] = v
        with pytest.raises(ValueError):
            ctx.fit_frame_psf_free_device(*a, psf_index_ptr=1)
    with pytest.raises(ValueError):
        ctx.fit_frame_psf_free_device(*ok)                           # npsf != nstar without psf_index_ptr
    for kw in [dict(radius=0.5), dict(tol=0), dict(max_iter=0), dict(background=0)] + FREE_BAD:
        with pytest.raises(ValueError):
            ctx.fit_frame_psf_free_device(*ok, psf_index_ptr=1, **kw)
    assert ctx.lib.calls == []
    ctx.fit_frame_psf_free_device(16384, 4096, 1, 2 ** 20, 1, 1, 1, 1, 1, 1, psf_index_ptr=1, radius=1, tol=1e-300,
                                  max_iter=1000, max_outer=16, max_step=1.0, max_move=4.0, min_snr=0)
    assert len(ctx.lib.calls) == 1                                   # the bounds themselves are legal


# ---- 3. psfrec against an answering stub
class FreeLib(FrameLib):
    """FrameLib whose mpsfr_fit_frame_psf_free answers as its mpsfr_fit_frame_psf does in columns 0 - 7, moves every
    star by (+0.125, -0.25) px (errors 0.5 and 0.25 px, flags 4, free in 3 steps; star 1 of three or more left out: it
    keeps its shift) and the head (3, 0.5, 77, 1234, 9, 1e-11, n, 0, 5, 2e-4, n, 40)."""

    def mpsfr_fit_frame_psf_free(self, *a):
        self.calls.append(('mpsfr_fit_frame_psf_free', a))
        ny, nx, n = a[1], a[2], a[5]
        sh = _array(a[10], 2 * n, C.c_double, np.float64).reshape(n, 2)
        out = _array(a[21], n * 16, C.c_double, np.float64).reshape(n, 16)
        out[:] = 0.0
        out[:, 0] = 1000.0 * sh[:, 0] + sh[:, 1]
        out[:, 1:7] = (1.0, 0.0, 2.0, 0.25, 50.0, 4.0)
        out[:, 2] = 2.0 * out[:, 0]
        out[:, 8:10] = sh + (0.125, -0.25)
        out[:, 10:16] = (0.5, 0.25, 0.125, -0.25, 4.0, 3.0)
        if n >= 3:
            out[1] = 0.0
            out[1, 7], out[1, 8:10] = 2.0, sh[1]
        _array(a[22], 2 * n, C.c_double, np.float64).reshape(n, 2)[:] = out[:, 8:10]
        _array(a[23], 12, C.c_double, np.float64)[:] = (3.0, 0.5, 77.0, 1234.0, 9.0, 1e-11, n, 0.0, 5.0, 2e-4, n, 40.0)
        if a[24] is not None:
            _array(a[24], ny * nx, C.c_double, np.float64)[:] = _array(a[3], ny * nx, C.c_double, np.float64)
        return 0


def _free_ctx(monkeypatch):
    ctx = make_ctx()
    ctx.lib = FreeLib()
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: ctx)
    return ctx


def test_refine_crowded_stars_table(monkeypatch):
    ctx = _free_ctx(monkeypatch)
    pos = np.array([[10.4, 20.5], [30.5, 7.25], [-3.0, 12.75], [50.0, 60.0]])
    image, psf = np.arange(70.0 * 80).reshape(70, 80), F.Y.models()[0]
    found = {'position': pos, 'scale': np.array([5.0, 6.0, 7.0, 8.0])}
    fit, origin, resid = psfrec.refine_crowded_stars(image, psf, found, start='found', radius=6, fit_back=False,
                                                     max_iter=50, tol=1e-8, max_outer=5, pos_tol=1e-2, max_step=0.25,
                                                     max_move=1.5, min_snr=4, return_residual=True, pixscale=0.25)
    assert tuple(fit.colnames) == psfrec._FIT_COLS_REFINED
    want = (np.rint(pos) - 20).astype(np.int32)
    assert origin.dtype == np.int32 and np.array_equal(origin, want)
    sh = pos - (want + 20)
    a = ctx.lib.calls[0][1]
    assert [c[0] for c in ctx.lib.calls] == ['mpsfr_fit_frame_psf_free']
    assert (a[1], a[2], a[5], a[6], a[12], a[13], a[14], a[15]) == (70, 80, 4, 1, 6.0, 0, 50, 1e-8)
    assert (a[16], a[17], a[18], a[19], a[20]) == (5, 1e-2, 0.25, 1.5, 4.0)
    np.testing.assert_array_equal(_array(a[11], 4, C.c_double, np.float64), [5.0, 6.0, 7.0, 8.0])
    np.testing.assert_array_equal(_array(a[10], 8, C.c_double, np.float64).reshape(4, 2), sh)
    keep = np.array([True, False, True, True])
    moved = sh + np.where(keep[:, None], (0.125, -0.25), 0.0)
    np.testing.assert_array_equal(fit['shift'], moved * 0.25)
    np.testing.assert_array_equal(fit['position'], (want + 20) + moved)
    np.testing.assert_array_equal(np.asarray(fit['err_shift'])[keep], np.tile((0.5 * 0.25, 0.25 * 0.25), (3, 1)))
    np.testing.assert_array_equal(np.asarray(fit['moved'])[keep], np.tile((0.125 * 0.25, -0.25 * 0.25), (3, 1)))
    np.testing.assert_array_equal(np.asarray(fit['scale'])[keep], (1000.0 * sh[:, 0] + sh[:, 1])[keep])
    np.testing.assert_array_equal(fit['status'], [0, 2, 0, 0])
    np.testing.assert_array_equal(fit['flags'], [4, 0, 4, 4])
    np.testing.assert_array_equal(fit['free'], [3, 0, 3, 3])
    np.testing.assert_array_equal(fit['npix'], [50, 0, 50, 50])
    assert all(np.asarray(fit[k]).dtype == np.int64 for k in ('npix', 'free', 'flags', 'status'))
    assert not np.asarray(fit['moved'])[1].any() and not np.asarray(fit['err_shift'])[1].any()
    assert dict(fit.meta) == dict(back=3.0, err_back=0.5, chi2=77.0, npix=1234, iterations=9, residual=1e-11, status=0,
                                  outer=5, step=2e-4, nfree=4, inner=40)
    assert np.array_equal(resid, image)
    # the defaults, one model stamp per star, a plain array of positions
    ctx.lib.calls.clear()
    fit, origin = psfrec.refine_crowded_stars(image, F.Y.models(), pos, var=np.ones((70, 80)))
    a = ctx.lib.calls[0][1]
    assert (a[6], a[12], a[13], a[14], a[15]) == (4, 8.0, 1, 100, 1e-10) and a[8] is None and a[11] is None
    assert (a[16], a[17], a[18], a[19], a[20]) == (8, 1e-3, 0.5, 2.0, 3.0) and a[4] is not None and a[24] is None
    # the table is what subtract_stars takes: the refined shifts at the origins of the start
    ctx.lib.calls.clear()
    res, status = psfrec.subtract_stars(image, F.Y.models(), origin, fit, pixscale=0.2)
    a = ctx.lib.calls[0][1]
    assert ctx.lib.calls[0][0] == 'mpsfr_render_stars' and a[4] == 3 and list(status) == [0, -1, 0, 0]
    np.testing.assert_allclose(_array(a[9], 6, C.c_double, np.float64).reshape(3, 2), moved[keep], rtol=1e-15)
    np.testing.assert_array_equal(_array(a[8], 6, C.c_int32, np.int32).reshape(3, 2), origin[keep])
    # refusals, before any call
    ctx.lib.calls.clear()
    for kw in [dict(radius=0.5), dict(fit_back=1), dict(start='find'), dict(start=np.zeros(3)), dict(max_iter=0),
               dict(tol=1.0), dict(pixscale=0.0), dict(return_residual=None)] + FREE_BAD:
        with pytest.raises(ValueError):
            psfrec.refine_crowded_stars(image, psf, pos, **kw)
    for p in (np.zeros(2), np.array([[np.nan, 1.0]]), np.zeros((0, 2))):
        with pytest.raises(ValueError):
            psfrec.refine_crowded_stars(image, psf, p)
    assert ctx.lib.calls == []
    ctx._h = None


def test_fit_found_stars_crowded_free(monkeypatch):
    ctx = _free_ctx(monkeypatch)
    pos, crit, shape = crowd()
    ref = GR.group(pos, crit, shape)
    row = {int(r[2]): k for k, r in enumerate(ref['groups'])}
    grp = np.array([row[int(v)] for v in ref['label']])
    crowded = ref['groups'][grp, 1] != 0
    assert crowded.sum() == 9
    image = np.random.default_rng(1).normal(size=shape)
    psf = np.zeros((NS, NS))
    psf[20, 20] = 1.0
    found = {'position': pos, 'scale': np.arange(len(pos)) + 100.0}
    held, origin_held = psfrec.fit_found_stars(image, psf, found, crit=crit, pixscale=0.25, crowded='frame', radius=5.0,
                                               fit_back=False)
    names_held = [c[0] for c in ctx.lib.calls]
    ctx.lib.calls.clear()
    fit, origin = psfrec.fit_found_stars(image, psf, found, crit=crit, pixscale=0.25, crowded='free', radius=5.0,
                                         fit_back=False)
    names = [c[0] for c in ctx.lib.calls]
    assert names[:-1] == names_held[:-1] and (names_held[-1], names[-1]) == ('mpsfr_fit_frame_psf',
                                                                              'mpsfr_fit_frame_psf_free')
    assert tuple(fit.colnames) == tuple(held.colnames) and np.array_equal(origin, origin_held)
    a = ctx.lib.calls[-1][1]
    idx = np.flatnonzero(crowded)
    own = (np.rint(pos[idx]) - 20).astype(np.int32)
    sh = pos[idx] - (own + 20)
    assert (a[1], a[2], a[5], a[6], a[12], a[13]) == (shape[0], shape[1], 9, 1, 5.0, 0)
    assert (a[14], a[15], a[16], a[17], a[18], a[19], a[20]) == (100, 1e-10, 8, 1e-3, 0.5, 2.0, 3.0)
    np.testing.assert_array_equal(_array(a[9], 18, C.c_int32, np.int32).reshape(9, 2), own)
    np.testing.assert_array_equal(_array(a[10], 18, C.c_double, np.float64).reshape(9, 2), sh)
    np.testing.assert_array_equal(_array(a[11], 9, C.c_double, np.float64), idx + 100.0)
    # every row but the crowded stars' shift and err_shift is what crowded='frame' gives
    for name in fit.colnames:
        if name not in ('shift', 'err_shift'):
            np.testing.assert_array_equal(np.asarray(fit[name]), np.asarray(held[name]), err_msg=name)
        np.testing.assert_array_equal(np.asarray(fit[name])[~crowded], np.asarray(held[name])[~crowded])
    ok = np.ones(9, dtype=bool)
    ok[1] = False                                                # the stub leaves star 1 out
    np.testing.assert_array_equal(np.asarray(fit['shift'])[idx[ok]], (sh[ok] + (0.125, -0.25)) * 0.25)
    np.testing.assert_array_equal(np.asarray(fit['err_shift'])[idx[ok]], np.tile((0.125, 0.0625), (8, 1)))
    assert fit['status'][idx[1]] == 2 and np.isnan(fit['scale'][idx[1]])
    ctx._h = None


# ---- 4. constants and exports
def test_exports_and_header_constants():
    assert 'mpsfr_fit_frame_psf_free' in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    for name, val in (('NFRAMEFREE', _lib.NFRAMEFREE), ('NFRAMEFREE_HEAD', _lib.NFRAMEFREE_HEAD),
                      ('FRAME_FREE_MAX_OUTER', _lib.FRAME_FREE_MAX_OUTER), ('FRAME_FREE_HELD', _lib.FRAME_FREE_HELD),
                      ('FRAME_FREE_BOUND', _lib.FRAME_FREE_BOUND), ('FRAME_FREE_CLIPPED', _lib.FRAME_FREE_CLIPPED)):
        assert int(re.search(r'#define MPSFR_%s\s+(\d+)' % name, hdr).group(1)) == val, name
    assert (_lib.NFRAMEFREE, _lib.NFRAMEFREE_HEAD, _lib.FRAME_FREE_MAX_OUTER) == (16, 12, 16)
    assert float(re.search(r'#define MPSFR_FRAME_FREE_MAX_STEP\s+([\d.]+)', hdr).group(1)) == _lib.FRAME_FREE_MAX_STEP == 1.0
    assert float(re.search(r'#define MPSFR_FRAME_FREE_MAX_MOVE\s+([\d.]+)', hdr).group(1)) == _lib.FRAME_FREE_MAX_MOVE == 4.0
    assert (G.HELD, G.BOUND, G.CLIPPED) == (_lib.FRAME_FREE_HELD, _lib.FRAME_FREE_BOUND, _lib.FRAME_FREE_CLIPPED)
    assert re.search(r'int mpsfr_fit_frame_psf_free\(mpsfr_ctx\* ctx, int ny, int nx, const double\* image', hdr)
    import muse_psfr_amd
    for name in ('refine_crowded_stars', 'NFRAMEFREE', 'NFRAMEFREE_HEAD', 'FRAME_FREE_MAX_OUTER', 'FRAME_FREE_MAX_STEP',
                 'FRAME_FREE_MAX_MOVE', 'FRAME_FREE_HELD', 'FRAME_FREE_BOUND', 'FRAME_FREE_CLIPPED'):
        assert hasattr(muse_psfr_amd, name), name
    build = __import__('muse_psfr_amd._build', fromlist=['SOURCES'])
    assert 'frame_free.hip' in build.SOURCES
    src = open(os.path.join(ROOT, 'muse_psfr_amd', 'csrc', 'frame_free.hip')).read()
    assert 'atomicAdd' not in src                              # no floating-point atomics: every sum has a fixed order
