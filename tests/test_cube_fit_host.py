"""CPU: the shared cube of cube_fit_cases.py and the Python layer of mpsfr_fit_cube_psf.

1. the cube: the statuses the GPU tests rely on hold in the yardsticks of the layers, and the yardstick's iteration
   counts over the fitted layers are not all equal (so the per-layer stop of a batch is exercised).
2. what Context.fit_cube_psf and fit_cube_psf_device hand to C (a recording stub), and every refusal of
   cube_fit_arguments, before any library call.
3. psfrec.fit_crowded_spectra against an answering stub: the call it makes and the table it builds.
4. constants and exports.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cube_fit_cases as K
import frame_fit_ref as F
from conftest import ROOT
from muse_psfr_amd import _lib, psfrec
from test_group_host import TableLib, _array
from test_render_host import DEV, HANDLE, make_ctx

NS = 40
TOL, MAX_ITER = 1e-10, 100
# the places of mpsfr_fit_cube_psf's arguments
(A_CTX, A_NL, A_NY, A_NX, A_CUBE, A_VAR, A_NSTAR, A_NPSF, A_PSF, A_INDEX, A_ORIGIN, A_SHIFT, A_LSHIFT, A_SCALE0, A_RADIUS,
 A_FLAGS, A_MAXIT, A_TOL, A_BATCH, A_ROWS, A_HEAD, A_RESID, A_ONDEV) = range(23)


# ---- 1. the cube
def test_cube_statuses_hold_in_the_references():
    c = K.cube()
    assert c['cube'].shape == (K.NL, 97, 150) and c['psf'].shape == (4, K.NL, NS, NS) and K.NL % 2 == 1
    assert np.array_equal(c['layer_shift'][2], [0.22, -0.14])
    for l in range(K.NL):
        ref = K.reference(l)
        if l == K.NAN_LAYER:
            assert ref['head_status'] == 2 and ref['nacc'] == 0
            assert set(ref['status']) == {1, 2} and ref['status'][c['off']] == 1
            assert np.array_equal(np.isnan(ref['resid']), np.ones(F.FRAME, dtype=bool))
            continue
        assert ref['head_status'] == 0
        want = np.zeros(c['n'], dtype=int)
        want[c['off']], want[c['dark']] = 1, 2
        if l == K.MASK_LAYER:
            want[K.MASKED] = 2
        np.testing.assert_array_equal(ref['status'], want)
    # every layer has other models per star, and another truth
    assert not np.array_equal(c['psf'][:, 0], c['psf'][:, 1]) and not np.array_equal(c['flux'][0], c['flux'][2])


def test_iteration_counts_of_the_yardstick_differ_between_layers():
    counts = [F.pcg(K.reference(l), TOL, MAX_ITER)[1] for l in K.FITTED]
    assert len(counts) == 4 and all(1 < n < MAX_ITER for n in counts)
    assert len(set(counts)) > 1, counts


def test_lattice_has_a_tile_list_longer_than_the_sort_chunk():
    s = K.lattice()
    assert s['n'] == 289 and s['cube'].shape == (2, 80, 80)
    assert K.longest_tile_list(s['origin'], (80, 80)) > _lib.RENDER_SORT_CHUNK == 256


# ---- 2. what reaches C
@pytest.fixture
def ctx():
    c = make_ctx()
    yield c
    c._h = None


def test_fit_cube_psf_host_form(ctx):
    c = K.cube()
    n, nl = c['n'], K.NL
    rows, head = ctx.fit_cube_psf(c['cube'], c['psf'], c['origin'], var=c['var'], shift=c['shift'],
                                  layer_shift=c['layer_shift'], psf_index=c['index'])
    assert rows.shape == (nl, n, _lib.NFRAMEFIT) and head.shape == (nl, _lib.NFRAMEFIT)
    name, a = ctx.lib.calls[0]
    assert name == 'mpsfr_fit_cube_psf' and len(a) == 23 and len(ctx.lib.calls) == 1 and a[A_CTX].value == HANDLE
    assert (a[A_NL], a[A_NY], a[A_NX], a[A_NSTAR], a[A_NPSF], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL], a[A_BATCH],
            a[A_ONDEV]) == (nl, 97, 150, n, 4, 8.0, _lib.FIT_BACKGROUND, 100, 1e-10, 0, 0)
    assert all(isinstance(a[i], int) and not isinstance(a[i], bool)
               for i in (A_NL, A_NY, A_NX, A_NSTAR, A_NPSF, A_FLAGS, A_MAXIT, A_BATCH, A_ONDEV))
    assert isinstance(a[A_RADIUS], float) and isinstance(a[A_TOL], float)
    assert a[A_SCALE0] is None and a[A_RESID] is None
    assert a[A_ROWS].value == rows.ctypes.data and a[A_HEAD].value == head.ctypes.data
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
    out = ctx.fit_cube_psf(c['cube'].tolist(), one, c['origin'].tolist(), scale0=np.arange(nl * n).reshape(nl, n),
                           radius=4, background=False, max_iter=1000, tol=np.float32(0.5), layer_batch=np.int64(7),
                           return_residual=True)
    a = ctx.lib.calls[0][1]
    assert len(out) == 3 and out[2].shape == (nl, 97, 150) and a[A_RESID].value == out[2].ctypes.data
    assert (a[A_NPSF], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL], a[A_BATCH]) == (n, 4.0, 0, 1000, 0.5, 7)
    assert all(a[i] is None for i in (A_VAR, A_INDEX, A_SHIFT, A_LSHIFT))
    np.testing.assert_array_equal(_array(a[A_SCALE0], nl * n, C.c_double, np.float64), np.arange(nl * n))
    # a masked cube: masked pixels are NaN; layer_shift without shift
    ctx.lib.calls.clear()
    ctx.fit_cube_psf(np.ma.masked_less(np.arange(12.0).reshape(2, 2, 3), 2.0), c['psf'][:1, :2], [[0, 0]],
                     layer_shift=[[8.0, -8.0], [0.0, 0.5]])
    a = ctx.lib.calls[0][1]
    assert np.isnan(_array(a[A_CUBE], 12, C.c_double, np.float64)[:2]).all()
    assert (a[A_NL], a[A_NY], a[A_NX], a[A_NSTAR], a[A_NPSF]) == (2, 2, 3, 1, 1) and a[A_SHIFT] is None


def test_fit_cube_psf_device_form(ctx):
    assert ctx.fit_cube_psf_device(7, 97, 150, DEV['image'], 4096, 4096, DEV['psf'], DEV['origin'], DEV['rows'],
                                   DEV['out']) is None
    name, a = ctx.lib.calls[0]
    assert name == 'mpsfr_fit_cube_psf' and len(a) == 23 and a[A_ONDEV] == 1
    assert (a[A_NL], a[A_NY], a[A_NX], a[A_NSTAR], a[A_NPSF], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL],
            a[A_BATCH]) == (7, 97, 150, 4096, 4096, 8.0, 1, 100, 1e-10, 0)
    assert (a[A_CUBE].value, a[A_PSF].value, a[A_ORIGIN].value, a[A_ROWS].value, a[A_HEAD].value) == \
        (DEV['image'], DEV['psf'], DEV['origin'], DEV['rows'], DEV['out'])
    assert all(a[i] is None for i in (A_VAR, A_INDEX, A_SHIFT, A_LSHIFT, A_SCALE0, A_RESID))
    ctx.lib.calls.clear()
    ctx.fit_cube_psf_device(_lib.CUBE_FIT_MAX_LAYERS, 1, 1, DEV['image'], 2 ** 20, 2 ** 20, DEV['psf'], DEV['origin'],
                            DEV['rows'], DEV['out'], var_ptr=DEV['var'], shift_ptr=DEV['shift'],
                            layer_shift_ptr=DEV['vstamps'], psf_index_ptr=DEV['index'], scale0_ptr=DEV['scale'],
                            resid_ptr=DEV['stamps'], radius=20, background=False, max_iter=1, tol=0.999,
                            layer_batch=5000)
    a = ctx.lib.calls[0][1]
    assert (a[A_VAR].value, a[A_INDEX].value, a[A_SHIFT].value, a[A_LSHIFT].value, a[A_SCALE0].value,
            a[A_RESID].value) == (DEV['var'], DEV['index'], DEV['shift'], DEV['vstamps'], DEV['scale'], DEV['stamps'])
    assert (a[A_NL], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL], a[A_BATCH]) == (4096, 20.0, 0, 1, 0.999, 5000)


def test_fit_cube_psf_refuses(ctx):
    c = K.cube()
    n, nl = c['n'], K.NL
    base = dict(cube=c['cube'], psf=c['psf'], origin=c['origin'], var=None, shift=None, layer_shift=None,
                psf_index=c['index'], scale0=None, radius=8.0, background=True, max_iter=100, tol=1e-10, layer_batch=0,
                return_residual=False)
    shift = np.zeros((n, 2))
    far, nan = shift.copy(), shift.copy()
    far[3, 1], nan[0, 0] = 8.5, np.nan
    edge = shift.copy()
    edge[5, 0] = 7.9                                             # legal alone, beyond 8 with the offset of a layer
    ls = c['layer_shift']
    ls_nan, ls_inf, ls_far = ls.copy(), ls.copy(), ls.copy()
    ls_nan[2, 0], ls_inf[4, 1], ls_far[1, 1] = np.nan, np.inf, -8.01
    bad = [dict(cube=c['cube'][0]), dict(cube='x'), dict(cube=np.zeros((0, 3, 3))), dict(cube=np.zeros((2, 0, 3))),
           dict(cube=c['cube'][None]), dict(var=c['var'][:4]), dict(var=c['var'][0]), dict(var='v'),
           dict(psf=c['psf'][:, :4]), dict(psf=c['psf'][:, :, :39]), dict(psf=c['psf'][0]), dict(psf='p'),
           dict(psf_index=None), dict(psf_index=np.full(n, 4)), dict(psf_index=np.zeros(n)),
           dict(psf_index=np.zeros(n - 1, dtype=int)),
           dict(origin=c['origin'][:, :1]), dict(origin=c['origin'].astype(float)),
           dict(origin=np.zeros((0, 2), dtype=int)), dict(origin=np.full((n, 2), 2 ** 30 + 1)),
           dict(shift=far), dict(shift=nan), dict(shift=shift[:-1]), dict(shift='s'),
           dict(layer_shift=ls_nan), dict(layer_shift=ls_inf), dict(layer_shift=ls_far), dict(layer_shift=ls[:4]),
           dict(layer_shift=ls.T), dict(layer_shift='l'), dict(layer_shift=np.zeros(nl)),
           dict(shift=edge, layer_shift=ls),
           dict(scale0=np.zeros(n)), dict(scale0=np.zeros((nl, n - 1))), dict(scale0=np.full((nl, n), np.inf)),
           dict(scale0=np.full((nl, n), np.nan)), dict(scale0='s'), dict(scale0=np.zeros((n, nl))),
           dict(radius=0.99), dict(radius=20.01), dict(radius=np.nan), dict(radius=np.inf), dict(radius='8'),
           dict(radius=None), dict(radius=True),
           dict(tol=0.0), dict(tol=1.0), dict(tol=-1e-3), dict(tol=np.nan), dict(tol=None), dict(tol=True),
           dict(max_iter=0), dict(max_iter=1001), dict(max_iter=10.0), dict(max_iter=True), dict(max_iter=None),
           dict(layer_batch=-1), dict(layer_batch=2.0), dict(layer_batch=True), dict(layer_batch=None),
           dict(layer_batch=2 ** 31),
           dict(background=1), dict(background=None), dict(return_residual=1)]
    for kw in bad:
        args = dict(base)
        args.update(kw)
        cu, ps, og = args.pop('cube'), args.pop('psf'), args.pop('origin')
        with pytest.raises(ValueError):
            ctx.fit_cube_psf(cu, ps, og, **args)
    with pytest.raises(ValueError):                              # more layers than one call takes
        ctx.fit_cube_psf(np.zeros((_lib.CUBE_FIT_MAX_LAYERS + 1, 1, 2)),
                         np.zeros((1, _lib.CUBE_FIT_MAX_LAYERS + 1, NS, NS)), [[0, 0]])
    ok = (3, 97, 150, 1, 10, 1, 1, 1, 1, 1)
    for k, v in [(0, 0), (0, _lib.CUBE_FIT_MAX_LAYERS + 1), (0, 3.0), (0, True), (1, 0), (2, 16385), (1, 97.0), (3, 0),
                 (4, 0), (4, 2 ** 20 + 1), (4, 1.0), (4, True), (5, 0), (6, 0), (7, 0), (8, 0), (9, None), (3, None)]:
        a = list(ok)
        a[k] = v
        with pytest.raises(ValueError):
            ctx.fit_cube_psf_device(*a, psf_index_ptr=1)
    with pytest.raises(ValueError):
        ctx.fit_cube_psf_device(*ok)                                 # npsf != nstar without psf_index_ptr
    for kw in (dict(radius=0.5), dict(radius=21), dict(tol=0), dict(tol=1), dict(max_iter=0), dict(max_iter=1001),
               dict(background=0), dict(tol=np.nan), dict(radius=np.nan), dict(layer_batch=-1), dict(layer_batch=1.0)):
        with pytest.raises(ValueError):
            ctx.fit_cube_psf_device(*ok, psf_index_ptr=1, **kw)
    assert ctx.lib.calls == []
    # the edges themselves are legal: a summed shift of exactly 8, the most layers, a batch above nl
    ctx.fit_cube_psf(c['cube'], c['psf'], c['origin'], psf_index=c['index'], shift=np.full((n, 2), 7.5),
                     layer_shift=np.full((nl, 2), 0.5), layer_batch=99)
    ctx.fit_cube_psf_device(4096, 16384, 4096, 1, 2 ** 20, 1, 1, 1, 1, 1, psf_index_ptr=1, radius=1, tol=1e-300,
                            max_iter=1000, layer_batch=2 ** 31 - 1)
    assert len(ctx.lib.calls) == 2


# ---- 3. psfrec against an answering stub
class CubeLib(TableLib):
    """TableLib whose mpsfr_fit_cube_psf answers, for star k of layer l, F = 1000 dp + dq of its shift plus 10^6 l (err 1
    + l, flux 2 F, err_flux 2, overlap 0.25, 50 + l pixels, N_kk 4, status 0; star 1 of layer 1 status 2) and the heads
    (3 + l, 0.5, 77, 1234, 9 + l, 1e-11, n, 0; layer 2: status 1), the residual the cube itself."""

    def mpsfr_fit_cube_psf(self, *a):
        self.calls.append(('mpsfr_fit_cube_psf', a))
        nl, ny, nx, n = a[A_NL], a[A_NY], a[A_NX], a[A_NSTAR]
        sh = _array(a[A_SHIFT], 2 * n, C.c_double, np.float64).reshape(n, 2)
        out = _array(a[A_ROWS], nl * n * 8, C.c_double, np.float64).reshape(nl, n, 8)
        head = _array(a[A_HEAD], nl * 8, C.c_double, np.float64).reshape(nl, 8)
        out[:] = 0.0
        for l in range(nl):
            out[l, :, 0] = 1000.0 * sh[:, 0] + sh[:, 1] + 1e6 * l
            out[l, :, 1:7] = (1.0 + l, 0.0, 2.0, 0.25, 50.0 + l, 4.0)
            out[l, :, 2] = 2.0 * out[l, :, 0]
            head[l] = (3.0 + l, 0.5, 77.0, 1234.0, 9.0 + l, 1e-11, n, 1.0 if l == 2 else 0.0)
        if nl > 1 and n > 1:
            out[1, 1] = (0, 0, 0, 0, 0, 0, 0, 2)
        if a[A_RESID] is not None:
            m = nl * ny * nx
            _array(a[A_RESID], m, C.c_double, np.float64)[:] = _array(a[A_CUBE], m, C.c_double, np.float64)
        return 0


def _cube_ctx(monkeypatch):
    ctx = make_ctx()
    ctx.lib = CubeLib()
    monkeypatch.setattr(psfrec, 'get_context', lambda *a, **k: ctx)
    return ctx


def test_fit_crowded_spectra_table(monkeypatch):
    ctx = _cube_ctx(monkeypatch)
    pos = np.array([[10.4, 20.5], [30.5, 7.25], [-3.0, 12.75], [50.0, 60.0]])
    nl, n = 3, 4
    cube = np.arange(nl * 70.0 * 80).reshape(nl, 70, 80)
    psf = np.stack([F.Y.models()[l] for l in range(nl)])                       # (nl, 40, 40): one model cube
    found = {'position': pos, 'scale': np.array([5.0, 6.0, 7.0, 8.0])}
    lbda = [500.0, 600.0, 700.0]
    dar = np.array([[0.0, 0.0], [0.05, -0.025], [0.1, -0.05]])               # arcsec
    fit, origin, resid = psfrec.fit_crowded_spectra(cube, psf, found, lbda=lbda, layer_shift=dar, start='found',
                                                    radius=6, fit_back=False, max_iter=50, tol=1e-8, layer_batch=2,
                                                    return_residual=True, pixscale=0.25)
    assert tuple(fit.colnames) == psfrec._FIT_COLS_CROWDED_SPECTRA == ('shift', 'scale', 'flux', 'err_scale',
                                                                       'err_flux', 'overlap', 'npix', 'status')
    want = (np.rint(pos) - 20).astype(np.int32)
    assert origin.dtype == np.int32 and np.array_equal(origin, want)
    sh = pos - (want + 20)
    assert [c[0] for c in ctx.lib.calls] == ['mpsfr_fit_cube_psf']
    a = ctx.lib.calls[0][1]
    assert (a[A_NL], a[A_NY], a[A_NX], a[A_NSTAR], a[A_NPSF], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL], a[A_BATCH],
            a[A_ONDEV]) == (nl, 70, 80, n, 1, 6.0, 0, 50, 1e-8, 2, 0)
    np.testing.assert_array_equal(_array(a[A_SCALE0], nl * n, C.c_double, np.float64).reshape(nl, n),
                                  np.tile([5.0, 6.0, 7.0, 8.0], (nl, 1)))
    np.testing.assert_array_equal(_array(a[A_INDEX], n, C.c_int32, np.int32), 0)
    np.testing.assert_array_equal(_array(a[A_SHIFT], 2 * n, C.c_double, np.float64).reshape(n, 2), sh)
    np.testing.assert_array_equal(_array(a[A_LSHIFT], 2 * nl, C.c_double, np.float64).reshape(nl, 2), dar / 0.25)
    np.testing.assert_array_equal(_array(a[A_PSF], nl * NS * NS, C.c_double, np.float64).reshape(nl, NS, NS), psf)
    F0 = (1000.0 * sh[:, 0] + sh[:, 1])[:, None] + 1e6 * np.arange(nl)[None, :]
    keep = np.ones((n, nl), dtype=bool)
    keep[1, 1] = False
    for name in ('scale', 'flux', 'err_scale', 'err_flux', 'overlap', 'npix', 'status'):
        assert np.asarray(fit[name]).shape == (n, nl), name
    np.testing.assert_array_equal(np.asarray(fit['scale'])[keep], F0[keep])
    np.testing.assert_array_equal(np.asarray(fit['flux'])[keep], 2.0 * F0[keep])
    np.testing.assert_array_equal(fit['shift'], sh * 0.25)
    st = np.zeros((n, nl), dtype=int)
    st[1, 1] = 2
    np.testing.assert_array_equal(fit['status'], st)
    np.testing.assert_array_equal(fit['npix'], np.where(keep, 50 + np.arange(nl)[None, :], 0))
    assert np.asarray(fit['npix']).dtype == np.int64 and np.asarray(fit['status']).dtype == np.int64
    np.testing.assert_array_equal(np.asarray(fit['overlap'])[keep], 0.25)
    np.testing.assert_array_equal(np.asarray(fit['err_scale']), np.where(keep, 1.0 + np.arange(nl)[None, :], 0.0))
    np.testing.assert_array_equal(np.asarray(fit['err_flux'])[keep], 2.0)
    assert np.asarray(fit['scale'])[1, 1] == 0.0
    meta = dict(fit.meta)
    assert sorted(meta) == sorted(psfrec._META_CROWDED_SPECTRA + ('lbda',))
    np.testing.assert_array_equal(meta['back'], [3.0, 4.0, 5.0])
    np.testing.assert_array_equal(meta['err_back'], [0.5] * 3)
    np.testing.assert_array_equal(meta['chi2'], [77.0] * 3)
    np.testing.assert_array_equal(meta['npix'], [1234] * 3)
    np.testing.assert_array_equal(meta['iterations'], [9, 10, 11])
    np.testing.assert_array_equal(meta['residual'], [1e-11] * 3)
    np.testing.assert_array_equal(meta['status'], [0, 0, 1])
    np.testing.assert_array_equal(meta['lbda'], lbda)
    assert all(meta[k].dtype == np.int64 for k in ('npix', 'iterations', 'status'))
    assert np.array_equal(resid, cube)
    # model cubes per star, a plain array of positions, no start, no offsets, no wavelengths
    ctx.lib.calls.clear()
    four = np.ascontiguousarray(np.broadcast_to(F.Y.models()[:, None], (4, nl, NS, NS)))
    fit, origin = psfrec.fit_crowded_spectra(cube, four, pos, var=np.ones((nl, 70, 80)))
    a = ctx.lib.calls[0][1]
    assert (a[A_NPSF], a[A_RADIUS], a[A_FLAGS], a[A_MAXIT], a[A_TOL], a[A_BATCH]) == (4, 8.0, 1, 100, 1e-10, 0)
    assert all(a[i] is None for i in (A_INDEX, A_SCALE0, A_LSHIFT, A_RESID)) and a[A_VAR] is not None
    assert 'lbda' not in fit.meta
    # an index into several model cubes
    ctx.lib.calls.clear()
    psfrec.fit_crowded_spectra(cube, four[:2], pos, psf_index=[1, 0, 1, 1], start=np.ones((nl, n)))
    a = ctx.lib.calls[0][1]
    np.testing.assert_array_equal(_array(a[A_INDEX], n, C.c_int32, np.int32), [1, 0, 1, 1])
    assert a[A_NPSF] == 2
    ctx._h = None


def test_fit_crowded_spectra_refuses(monkeypatch):
    ctx = _cube_ctx(monkeypatch)
    nl = 3
    cube, psf, pos = np.zeros((nl, 30, 30)), np.stack([F.Y.models()[0]] * nl), np.array([[3.0, 4.0], [5.0, 6.0]])
    for p in (np.zeros(2), 'p', np.zeros((2, 3)), np.array([[np.nan, 1.0]]), np.array([[2.0 ** 31, 1.0]]),
              np.zeros((0, 2))):
        with pytest.raises(ValueError):
            psfrec.fit_crowded_spectra(cube, psf, p)
    for kw in (dict(radius=0.5), dict(radius=25), dict(fit_back=1), dict(start='find'), dict(start='found'),
               dict(start=np.zeros(2)), dict(start=np.full((nl, 2), np.nan)), dict(max_iter=0), dict(tol=1.0), dict(tol=0),
               dict(pixscale=0.0), dict(var=np.ones((nl, 3, 3))), dict(psf_index=[0, 0]), dict(return_residual=None),
               dict(layer_batch=-1), dict(layer_batch=1.5), dict(lbda=[1.0, 2.0]), dict(lbda='w'),
               dict(layer_shift=np.zeros((2, 2))), dict(layer_shift=np.full((nl, 2), np.nan)), dict(layer_shift='s'),
               dict(layer_shift=np.full((nl, 2), 1.7))):                      # 8.5 px at 0.2 arcsec per pixel
        with pytest.raises(ValueError):
            psfrec.fit_crowded_spectra(cube, psf, pos, **kw)
    for bad_psf in (np.zeros((40, 39)), 'p', np.zeros(40), np.zeros((40, 40)), np.zeros((2, 40, 40)),
                    np.zeros((3, nl, 40, 40)), np.zeros((2, 2, 40, 40))):
        with pytest.raises(ValueError):
            psfrec.fit_crowded_spectra(cube, bad_psf, pos)
    with pytest.raises(ValueError):
        psfrec.fit_crowded_spectra(cube[0], psf, pos)
    assert ctx.lib.calls == []
    ctx._h = None


# ---- 4. constants and exports
def test_exports_and_header_constants():
    assert 'mpsfr_fit_cube_psf' in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'mpsfr.h')).read()
    assert int(re.search(r'#define MPSFR_CUBE_FIT_MAX_LAYERS\s+(\d+)', hdr).group(1)) == _lib.CUBE_FIT_MAX_LAYERS >= 4096
    assert re.search(r'#define MPSFR_CUBE_FIT_WORK_BYTES\s+\(\(size_t\)256 << 20\)', hdr)
    assert re.search(r'int mpsfr_fit_cube_psf\(mpsfr_ctx\* ctx, int nl, int ny, int nx, const double\* cube', hdr)
    assert 'THE CONTRACT' in hdr
    import muse_psfr_amd
    for name in ('fit_crowded_spectra', 'CUBE_FIT_MAX_LAYERS'):
        assert hasattr(muse_psfr_amd, name), name
    assert 'fit_crowded_spectra' in muse_psfr_amd.__doc__
    build = __import__('muse_psfr_amd._build', fromlist=['SOURCES'])
    assert 'cube_fit.hip' in build.SOURCES and 'frame_fit_impl.h' in build.HEADERS
