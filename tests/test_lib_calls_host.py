"""Host: what every public Context method hands to the C library, argument by argument.

A Context is built without the library and given a stub `lib` that records each call (name, arguments) and returns 0;
mpsfr_last_ticket returns the number of mpsfr_reconstruct* calls made so far minus one, as the library's ticket
counter does.  Every test calls one public method on small fixed inputs (2 rows, 3 wavelengths, 2 positions, 2 bands,
3 layers, 5 stamps) and compares the recorded call with the prototype of include/mpsfr.h, written out here by hand:
the function name, the number of arguments, every scalar by value, every array by element type, shape and content,
every output buffer by identity with the returned array (whose shape is asserted), NULL where an optional argument is
absent, and the value of on_device.  The asynchronous forms also check the `_pending` / PendingResult bookkeeping.
"""
import ctypes as C

import numpy as np
import pytest

from muse_psfr_amd import _lib
from muse_psfr_amd._lib import NFIT, NFIT_ELL, NFIT_PSF, NMET_HEAD, Context, PendingMulti, PendingResult

DIM, NS = 8, 40
LB = np.array([500.0, 700.0, 900.0])
SEE = np.array([0.9, 1.1])
GL = np.array([0.6, 0.45])
L0 = np.array([22.0, 13.0])
THREE = np.array([0, 1], np.uint8)
HH = np.array([100.0, 10000.0])
POS = np.array([[0.0, 0.0], [25.0, -15.0]])
BW = np.array([[1.0, 2.0, 1.0], [0.0, 1.0, 3.0]])
LAY_H = np.array([0.0, 3000.0, 12000.0])
LAY_WS = np.array([8.0, 15.0, 25.0])
LAY_WD = np.array([0.3, 1.2, 2.5])
CN2 = np.array([[0.5, 0.3, 0.2], [0.2, 0.2, 0.6]])
_rng = np.random.default_rng(11)
MREC = _rng.uniform(size=(80, 80)) < 0.5
MRES = ~MREC
STAMPS = _rng.uniform(0.1, 1.0, (5, NS, NS))
VAR = _rng.uniform(0.5, 1.5, (5, NS, NS))
HANDLE = 0xABC0
DEV = dict(psf=0x10000, sum=0x20000, fit=0x30000, stamps=0x40000, var=0x50000, model=0x60000, index=0x70000,
           shift=0x80000, centers=0x90000)


class StubLib:
    """Every attribute is a C function that records (name, args) and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            if name == 'mpsfr_last_ticket':
                return sum(1 for n, _ in self.calls if n.startswith('mpsfr_reconstruct')) - 1
            self.calls.append((name, args))
            return 0
        return fn


def make_ctx(handle=HANDLE):
    ctx = Context.__new__(Context)
    ctx.lib = StubLib()
    ctx.dim, ctx.pixscale, ctx.dimpsf, ctx.precision = DIM, 0.2, NS, 'mixed'
    ctx._h = C.c_void_p(handle)
    ctx._pending, ctx._abandoned = {}, set()
    return ctx


@pytest.fixture
def ctx():
    c = make_ctx()
    yield c
    c._h = None            # (nothing to destroy)


# ---- the expected arguments: one item per C parameter
def I(v):
    return ('int', v)


def F(v):
    return ('float', v)


def D(a):
    """const double*: a typed pointer to these values."""
    return ('double*', np.asarray(a, dtype=np.float64))


def U8(a):
    """const uint8_t*: a typed pointer to these values."""
    return ('uint8*', np.asarray(a, dtype=np.uint8))


def V(a, dtype=np.float64):
    """A pointer of any type (the stamp family's arguments are void* in the binding) to these values."""
    return ('void*', np.asarray(a, dtype=dtype))


def OUT(a):
    """An output buffer: the pointer is the data of the returned array `a`."""
    return ('out', a)


def DEVP(addr):
    return ('dev', addr)


NULL = ('null',)
CTX = ('ctx',)

_CT = {np.dtype(np.float64): C.c_double, np.dtype(np.uint8): C.c_uint8, np.dtype(np.int32): C.c_int32}


def _addr(arg):
    return C.cast(arg, C.c_void_p).value


def _values(arg, like):
    n = int(like.size)
    buf = (_CT[like.dtype] * n).from_address(_addr(arg))
    return np.frombuffer(buf, dtype=like.dtype).reshape(like.shape)


def _is_null(arg):
    return arg is None or (isinstance(arg, C.c_void_p) and arg.value is None)


def expect(lib, index, name, items):
    got_name, args = lib.calls[index]
    assert got_name == name
    assert len(args) == len(items), (name, len(args), len(items))
    for k, (arg, item) in enumerate(zip(args, items)):
        kind, where = item[0], (name, k, item[0])
        if kind == 'ctx':
            assert isinstance(arg, C.c_void_p) and arg.value == HANDLE, where
        elif kind == 'int':
            assert isinstance(arg, (int, np.integer)) and not isinstance(arg, bool) and arg == item[1], where + (arg,)
        elif kind == 'float':
            assert isinstance(arg, float) and arg == item[1], where + (arg,)
        elif kind == 'null':
            assert _is_null(arg), where + (arg,)
        elif kind == 'dev':
            assert isinstance(arg, C.c_void_p) and arg.value == item[1], where + (arg,)
        elif kind == 'out':
            assert not _is_null(arg) and _addr(arg) == item[1].ctypes.data, where
            assert item[1].dtype == np.float64 and item[1].flags.c_contiguous, where
        else:
            want = item[1]
            if kind == 'double*':
                assert isinstance(arg, C.POINTER(C.c_double)), where + (type(arg),)
            elif kind == 'uint8*':
                assert isinstance(arg, C.POINTER(C.c_uint8)), where + (type(arg),)
            assert not _is_null(arg), where
            held = getattr(arg, '_arr', None)       # (numpy's data_as keeps the array: its own dtype and size)
            if held is not None:
                assert held.dtype == want.dtype and held.size == want.size and held.flags.c_contiguous, where
            np.testing.assert_array_equal(_values(arg, want), want, err_msg=str(where))


def shapes(r, psf, psum, fit):
    for key, shape in (('psf', psf), ('psf_sum', psum), ('fit', fit)):
        if shape is None:
            assert r[key] is None, key
        else:
            assert r[key].shape == shape and r[key].dtype == np.float64, (key, r[key].shape)
    assert set(r) == {'psf', 'psf_sum', 'fit'}


def out_or_null(a):
    return NULL if a is None else OUT(a)


ROWS = [I(2), D(SEE), D(GL), D(L0), U8(THREE)]                 # ntask, seeing, gl, l0, three_lgs
DEV_OUT = [DEVP(DEV['psf']), DEVP(DEV['sum']), DEVP(DEV['fit'])]


# ---- mpsfr_reconstruct(ctx, ntask, seeing, gl, l0, three_lgs, h, wind_speed, npsflin, nl, lbda_nm, mask_rec, mask_res,
#                        psf_out, psf_sum_out, fit_out, on_device)
def test_reconstruct_host(ctx):
    r = ctx.reconstruct(LB, SEE, GL, L0, THREE, HH, wind_speed=9.5, npsflin=2)
    shapes(r, (2, 3, NS, NS), (3, NS, NS), (2, 3, NFIT))
    assert len(ctx.lib.calls) == 1 and ctx._pending == {}
    expect(ctx.lib, 0, 'mpsfr_reconstruct', [CTX] + ROWS + [D(HH), F(9.5), I(2), I(3), D(LB), NULL, NULL,
                                                            OUT(r['psf']), OUT(r['psf_sum']), OUT(r['fit']), I(0)])


def test_reconstruct_defaults_masks_and_absent_outputs(ctx):
    """three_lgs None: zeros; wind_speed None: full_like(h, 12.5)[0], which is 12 for the integer default of h
    (psfrec.py:61); scalars become one-row arrays; an output that is not wanted is NULL."""
    r = ctx.reconstruct(700.0, 0.9, 0.6, 22.0, masks=(MREC, MRES), want_psf=False, want_fit=False)
    shapes(r, None, (1, NS, NS), None)
    expect(ctx.lib, 0, 'mpsfr_reconstruct',
           [CTX, I(1), D([0.9]), D([0.6]), D([22.0]), U8([0]), D([100.0, 10000.0]), F(12.0), I(1), I(1), D([700.0]),
            U8(MREC.ravel()), U8(MRES.ravel()), NULL, OUT(r['psf_sum']), NULL, I(0)])


def test_reconstruct_async_bookkeeping(ctx):
    pend = [ctx.reconstruct_async(LB, SEE, GL, L0, THREE, HH, wind_speed=9.5, want_sum=False) for _ in range(6)]
    for t, p in enumerate(pend):
        assert isinstance(p, PendingResult) and p.ticket == t and p.ctx is ctx
        shapes(p._arrays, (2, 3, NS, NS), None, (2, 3, NFIT))
        expect(ctx.lib, t, 'mpsfr_reconstruct', [CTX] + ROWS + [D(HH), F(9.5), I(1), I(3), D(LB), NULL, NULL,
                                                                OUT(p._arrays['psf']), NULL, OUT(p._arrays['fit']), I(2)])
    # the call with ticket t handed over ticket t - 4: four stay registered, each with the arrays of its result
    assert sorted(ctx._pending) == [2, 3, 4, 5]
    assert all(ctx._pending[t] is pend[t]._arrays for t in ctx._pending)
    assert len(ctx.lib.calls) == 6
    assert pend[3].wait() is pend[3]._arrays
    assert ctx.lib.calls[6][0] == 'mpsfr_wait' and ctx.lib.calls[6][1][1] == 3
    assert sorted(ctx._pending) == [4, 5]
    assert pend[0].wait() is pend[0]._arrays and len(ctx.lib.calls) == 7      # (handed over: no library call)
    ctx.sync()
    assert ctx.lib.calls[7][0] == 'mpsfr_sync' and ctx._pending == {}


def test_reconstruct_device(ctx):
    assert ctx.reconstruct_device(LB, SEE, GL, L0, THREE, HH, 12.0, 1, None, DEV['psf'], None, DEV['fit']) is None
    expect(ctx.lib, 0, 'mpsfr_reconstruct', [CTX] + ROWS + [D(HH), F(12.0), I(1), I(3), D(LB), NULL, NULL,
                                                            DEVP(DEV['psf']), NULL, DEVP(DEV['fit']), I(1)])
    ctx.reconstruct_device(LB, SEE, GL, L0, THREE, HH, 12.0, 2, (MREC, MRES), *[a[1] for a in DEV_OUT])
    expect(ctx.lib, 1, 'mpsfr_reconstruct', [CTX] + ROWS + [D(HH), F(12.0), I(2), I(3), D(LB), U8(MREC.ravel()),
                                                            U8(MRES.ravel())] + DEV_OUT + [I(1)])
    assert ctx._pending == {}


# ---- mpsfr_reconstruct_field(ctx, ntask, seeing, gl, l0, three_lgs, h, wind_speed, npos, pos_arcsec, nl, lbda_nm,
#                              mask_rec, mask_res, psf_out, psf_sum_out, fit_out, on_device)
def _field_args(outs, on_device, masks=False):
    m = [U8(MREC.ravel()), U8(MRES.ravel())] if masks else [NULL, NULL]
    return [CTX] + ROWS + [D(HH), F(9.5), I(2), D(POS), I(3), D(LB)] + m + outs + [I(on_device)]


def test_reconstruct_field_host_async_device(ctx):
    r = ctx.reconstruct_field(LB, SEE, GL, L0, THREE, HH, POS, wind_speed=9.5)
    shapes(r, (2, 2, 3, NS, NS), (2, 3, NS, NS), (2, 2, 3, NFIT))
    expect(ctx.lib, 0, 'mpsfr_reconstruct_field', _field_args([OUT(r['psf']), OUT(r['psf_sum']), OUT(r['fit'])], 0))
    p = ctx.reconstruct_field_async(LB, SEE, GL, L0, THREE, HH, POS, wind_speed=9.5, masks=(MREC, MRES),
                                    want_psf=False)
    assert isinstance(p, PendingResult) and p.ticket == 1 and ctx._pending == {1: p._arrays}
    shapes(p._arrays, None, (2, 3, NS, NS), (2, 2, 3, NFIT))
    expect(ctx.lib, 1, 'mpsfr_reconstruct_field',
           _field_args([NULL, OUT(p._arrays['psf_sum']), OUT(p._arrays['fit'])], 2, masks=True))
    assert ctx.reconstruct_field_device(LB, SEE, GL, L0, THREE, HH, 9.5, POS, None, *[a[1] for a in DEV_OUT]) is None
    expect(ctx.lib, 2, 'mpsfr_reconstruct_field', _field_args(DEV_OUT, 1))
    assert len(ctx.lib.calls) == 3 and ctx._pending == {1: p._arrays}


# ---- mpsfr_reconstruct_band(ctx, ntask, seeing, gl, l0, three_lgs, h, wind_speed, npsflin, npos, pos_arcsec, nl,
#                             lbda_nm, nband, weights, mask_rec, mask_res, band_out, band_sum_out, band_fit_out, on_device)
def _band_args(npsflin, pos, outs, on_device, masks=False):
    m = [U8(MREC.ravel()), U8(MRES.ravel())] if masks else [NULL, NULL]
    p = [I(0), NULL] if pos is None else [I(2), D(pos)]
    return [CTX] + ROWS + [D(HH), F(9.5), I(npsflin)] + p + [I(3), D(LB), I(2), D(BW)] + m + outs + [I(on_device)]


def test_reconstruct_band_grid(ctx):
    r = ctx.reconstruct_band(LB, BW, SEE, GL, L0, THREE, HH, wind_speed=9.5, npsflin=2)
    shapes(r, (2, 2, NS, NS), (2, NS, NS), (2, 2, NFIT))
    expect(ctx.lib, 0, 'mpsfr_reconstruct_band', _band_args(2, None, [OUT(r['psf']), OUT(r['psf_sum']), OUT(r['fit'])], 0))
    r = ctx.reconstruct_band(LB, BW, SEE, GL, L0, THREE, HH, wind_speed=9.5, want_fit=False)     # (npsflin None: 1)
    shapes(r, (2, 2, NS, NS), (2, NS, NS), None)
    expect(ctx.lib, 1, 'mpsfr_reconstruct_band', _band_args(1, None, [OUT(r['psf']), OUT(r['psf_sum']), NULL], 0))
    ctx.reconstruct_band_device(LB, BW, SEE, GL, L0, THREE, HH, 9.5, 3, None, (MREC, MRES), *[a[1] for a in DEV_OUT])
    expect(ctx.lib, 2, 'mpsfr_reconstruct_band', _band_args(3, None, DEV_OUT, 1, masks=True))
    ctx.reconstruct_band_device(LB, BW, SEE, GL, L0, THREE, HH, 9.5, None, None, None, *[a[1] for a in DEV_OUT])
    expect(ctx.lib, 3, 'mpsfr_reconstruct_band', _band_args(1, None, DEV_OUT, 1))
    assert ctx._pending == {}


def test_reconstruct_band_positions(ctx):
    """With positions the C call takes npsflin = 0, whether the caller leaves it at None or passes 0."""
    r = ctx.reconstruct_band(LB, BW, SEE, GL, L0, THREE, HH, wind_speed=9.5, positions=POS)
    shapes(r, (2, 2, 2, NS, NS), (2, 2, NS, NS), (2, 2, 2, NFIT))
    expect(ctx.lib, 0, 'mpsfr_reconstruct_band', _band_args(0, POS, [OUT(r['psf']), OUT(r['psf_sum']), OUT(r['fit'])], 0))
    p = ctx.reconstruct_band_async(LB, BW, SEE, GL, L0, THREE, HH, wind_speed=9.5, npsflin=0, positions=POS,
                                   want_sum=False)
    assert isinstance(p, PendingResult) and p.ticket == 1 and ctx._pending == {1: p._arrays}
    shapes(p._arrays, (2, 2, 2, NS, NS), None, (2, 2, 2, NFIT))
    expect(ctx.lib, 1, 'mpsfr_reconstruct_band',
           _band_args(0, POS, [OUT(p._arrays['psf']), NULL, OUT(p._arrays['fit'])], 2))
    ctx.reconstruct_band_device(LB, BW, SEE, GL, L0, THREE, HH, 9.5, None, POS, None, *[a[1] for a in DEV_OUT])
    expect(ctx.lib, 2, 'mpsfr_reconstruct_band', _band_args(0, POS, DEV_OUT, 1))


# ---- mpsfr_reconstruct_profile(ctx, ntask, seeing, gl, l0, three_lgs, nlayer, h, wind_speed, wind_dir, cn2, npsflin,
#                                npos, pos_arcsec, nl, lbda_nm, mask_rec, mask_res, psf_out, psf_sum_out, fit_out, on_device)
def _profile_args(npsflin, pos, outs, on_device, masks=False, cn2=CN2):
    m = [U8(MREC.ravel()), U8(MRES.ravel())] if masks else [NULL, NULL]
    p = [I(0), NULL] if pos is None else [I(2), D(pos)]
    return ([CTX] + ROWS + [I(3), D(LAY_H), D(LAY_WS), D(LAY_WD), D(cn2), I(npsflin)] + p + [I(3), D(LB)] + m + outs
            + [I(on_device)])


def test_reconstruct_profile_grid(ctx):
    r = ctx.reconstruct_profile(LB, SEE, GL, L0, CN2, LAY_H, LAY_WS, LAY_WD, THREE, npsflin=2)
    shapes(r, (2, 3, NS, NS), (3, NS, NS), (2, 3, NFIT))
    expect(ctx.lib, 0, 'mpsfr_reconstruct_profile',
           _profile_args(2, None, [OUT(r['psf']), OUT(r['psf_sum']), OUT(r['fit'])], 0))
    # npsflin None: 1; one row of weights serves every row; a scalar wind speed serves every layer
    p = ctx.reconstruct_profile_async(LB, SEE, GL, L0, CN2[0], LAY_H, 15.0, LAY_WD, THREE, masks=(MREC, MRES),
                                      want_psf=False)
    assert isinstance(p, PendingResult) and p.ticket == 1 and ctx._pending == {1: p._arrays}
    shapes(p._arrays, None, (3, NS, NS), (2, 3, NFIT))
    want = _profile_args(1, None, [NULL, OUT(p._arrays['psf_sum']), OUT(p._arrays['fit'])], 2, masks=True,
                         cn2=np.array([CN2[0], CN2[0]]))
    want[8] = D([15.0, 15.0, 15.0])
    expect(ctx.lib, 1, 'mpsfr_reconstruct_profile', want)
    ctx.reconstruct_profile_device(LB, SEE, GL, L0, CN2, LAY_H, LAY_WS, LAY_WD, THREE, 3, None, None,
                                   *[a[1] for a in DEV_OUT])
    expect(ctx.lib, 2, 'mpsfr_reconstruct_profile', _profile_args(3, None, DEV_OUT, 1))
    ctx.reconstruct_profile_device(LB, SEE, GL, L0, CN2, LAY_H, LAY_WS, LAY_WD, THREE, None, None, None,
                                   *[a[1] for a in DEV_OUT])
    expect(ctx.lib, 3, 'mpsfr_reconstruct_profile', _profile_args(1, None, DEV_OUT, 1))


def test_reconstruct_profile_positions(ctx):
    r = ctx.reconstruct_profile(LB, SEE, GL, L0, CN2, LAY_H, LAY_WS, LAY_WD, THREE, positions=POS)
    shapes(r, (2, 2, 3, NS, NS), (2, 3, NS, NS), (2, 2, 3, NFIT))
    expect(ctx.lib, 0, 'mpsfr_reconstruct_profile',
           _profile_args(0, POS, [OUT(r['psf']), OUT(r['psf_sum']), OUT(r['fit'])], 0))
    ctx.reconstruct_profile_device(LB, SEE, GL, L0, CN2, LAY_H, LAY_WS, LAY_WD, THREE, 0, POS, (MREC, MRES),
                                   DEV['psf'], None, DEV['fit'])
    expect(ctx.lib, 1, 'mpsfr_reconstruct_profile',
           _profile_args(0, POS, [DEVP(DEV['psf']), NULL, DEVP(DEV['fit'])], 1, masks=True))
    assert ctx._pending == {}


# ---- mpsfr_simul_psd_profile(ctx, seeing, l0, three_lgs, nlayer, h, wind_speed, wind_dir, cn2, npsflin, npos,
#                              pos_arcsec, mask_rec, mask_res, psd_out)
def test_simul_psd_profile(ctx):
    out = ctx.simul_psd_profile(0.9, 22.0, CN2[0], LAY_H, LAY_WS, LAY_WD, three_lgs=True, npsflin=2)
    assert out.shape == (4, DIM, DIM) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_simul_psd_profile',
           [CTX, F(0.9), F(22.0), I(1), I(3), D(LAY_H), D(LAY_WS), D(LAY_WD), D(CN2[:1]), I(2), I(0), NULL, NULL, NULL,
            OUT(out)])
    out = ctx.simul_psd_profile(0.9, 22.0, CN2[0], LAY_H, LAY_WS, LAY_WD, positions=POS, masks=(MREC, MRES))
    assert out.shape == (2, DIM, DIM)
    expect(ctx.lib, 1, 'mpsfr_simul_psd_profile',
           [CTX, F(0.9), F(22.0), I(0), I(3), D(LAY_H), D(LAY_WS), D(LAY_WD), D(CN2[:1]), I(0), I(2), D(POS),
            U8(MREC.ravel()), U8(MRES.ravel()), OUT(out)])


# ---- mpsfr_simul_psd(ctx, seeing, gl, l0, three_lgs, h, wind_speed, npsflin, mask_rec, mask_res, psd_out)
def test_simul_psd(ctx):
    out = ctx.simul_psd(0.9, 0.6, 22.0, three_lgs=True, h=HH, wind_speed=9.5, npsflin=2)
    assert out.shape == (4, DIM, DIM) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_simul_psd', [CTX, F(0.9), F(0.6), F(22.0), I(1), D(HH), F(9.5), I(2), NULL, NULL, OUT(out)])
    out = ctx.simul_psd(0.9, 0.6, 22.0, masks=(MREC, MRES))       # (wind speed: see the reconstruct defaults)
    assert out.shape == (1, DIM, DIM)
    expect(ctx.lib, 1, 'mpsfr_simul_psd', [CTX, F(0.9), F(0.6), F(22.0), I(0), D(HH), F(12.0), I(1), U8(MREC.ravel()),
                                           U8(MRES.ravel()), OUT(out)])


# ---- mpsfr_psf_from_psd(ctx, ndir, psd, nl, lbda_nm, psf_out)
def test_psf_from_psd(ctx):
    psd = _rng.uniform(size=(4, DIM, DIM))
    out = ctx.psf_from_psd(psd, LB)
    assert out.shape == (3, NS, NS) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_psf_from_psd', [CTX, I(4), D(psd), I(3), D(LB), OUT(out)])
    out = ctx.psf_from_psd(psd[0], 700.0)
    assert out.shape == (1, NS, NS)
    expect(ctx.lib, 1, 'mpsfr_psf_from_psd', [CTX, I(1), D(psd[:1]), I(1), D([700.0]), OUT(out)])


# ---- mpsfr_psd_to_psf(ctx, npsd, psd, npup, pup, phase_static, D, nl, lbda_m, dimnum, psf_out, on_device)
def test_psd_to_psf(ctx):
    psd = _rng.uniform(size=(2, DIM, DIM))
    pup = _rng.uniform(size=(4, 4))
    ph = _rng.uniform(size=(4, 4))
    lm = LB * 1e-9
    out = ctx.psd_to_psf(psd, pup, 8.0, lm)
    assert out.shape == (2, 3, DIM, DIM) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_psd_to_psf', [CTX, I(2), D(psd), I(4), D(pup), NULL, F(8.0), I(3), D(lm), I(DIM), OUT(out),
                                            I(0)])
    assert ctx.psd_to_psf(psd[0], pup, 8.0, lm[0], phase_static=ph, dimnum=4, out=DEV['psf']) is None
    expect(ctx.lib, 1, 'mpsfr_psd_to_psf', [CTX, I(1), D(psd[:1]), I(4), D(pup), D(ph), F(8.0), I(1), D(lm[:1]), I(4),
                                            DEVP(DEV['psf']), I(1)])


# ---- mpsfr_convolve_stamps(ctx, ntask, seeing, gl, l0, nl, lbda_nm, psf_in, psf_out)
def test_convolve_stamps(ctx):
    st = _rng.uniform(size=(2, 3, NS, NS))
    out = ctx.convolve_stamps(LB, SEE, GL, L0, st)
    assert out.shape == (2, 3, NS, NS) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_convolve_stamps', [CTX, I(2), D(SEE), D(GL), D(L0), I(3), D(LB), D(st), OUT(out)])
    one = ctx.convolve_stamps(LB, 0.9, 0.6, 22.0, st[0])
    assert one.shape == (3, NS, NS)
    expect(ctx.lib, 1, 'mpsfr_convolve_stamps', [CTX, I(1), D([0.9]), D([0.6]), D([22.0]), I(3), D(LB), D(st[:1]),
                                                 OUT(one)])


# ---- the stamp family: mpsfr_fit_stamps(ctx, nstamp, stamps, fit_out, on_device) and its siblings
def test_fit_stamps(ctx):
    out = ctx.fit_stamps(STAMPS)
    assert out.shape == (5, NFIT) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_fit_stamps', [CTX, I(5), V(STAMPS), OUT(out), I(0)])


def test_fit_stamps_device(ctx):
    assert ctx.fit_stamps_device(5, DEV['stamps'], DEV['fit']) is None
    expect(ctx.lib, 0, 'mpsfr_fit_stamps', [CTX, I(5), DEVP(DEV['stamps']), DEVP(DEV['fit']), I(1)])
    for bad in (dict(nstamp=0), dict(nstamp=True), dict(nstamp=2.0), dict(stamps_ptr=0), dict(fit_ptr=None)):
        with pytest.raises(ValueError):
            ctx.fit_stamps_device(**dict(dict(nstamp=5, stamps_ptr=DEV['stamps'], fit_ptr=DEV['fit']), **bad))
    assert len(ctx.lib.calls) == 1


def test_fit_stamps_elliptical(ctx):
    out = ctx.fit_stamps_elliptical(STAMPS)
    assert out.shape == (5, NFIT_ELL) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_fit_stamps_elliptical', [CTX, I(5), V(STAMPS), OUT(out), I(0)])
    assert ctx.fit_stamps_elliptical_device(5, DEV['stamps'], DEV['fit']) is None
    expect(ctx.lib, 1, 'mpsfr_fit_stamps_elliptical', [CTX, I(5), DEVP(DEV['stamps']), DEVP(DEV['fit']), I(1)])


# mpsfr_fit_stamps_observed(ctx, nstamp, stamps, var, flags, fit_out, on_device): flags 1 background, 2 elliptical
def test_fit_stamps_observed(ctx):
    out = ctx.fit_stamps_observed(STAMPS)
    assert out.shape == (5, NFIT_ELL) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_fit_stamps_observed', [CTX, I(5), V(STAMPS), NULL, I(1), OUT(out), I(0)])
    out = ctx.fit_stamps_observed(STAMPS, VAR, background=False, circular=False)
    expect(ctx.lib, 1, 'mpsfr_fit_stamps_observed', [CTX, I(5), V(STAMPS), V(VAR), I(2), OUT(out), I(0)])
    assert ctx.fit_stamps_observed_device(5, DEV['stamps'], DEV['fit']) is None
    expect(ctx.lib, 2, 'mpsfr_fit_stamps_observed', [CTX, I(5), DEVP(DEV['stamps']), NULL, I(1), DEVP(DEV['fit']), I(1)])
    ctx.fit_stamps_observed_device(5, DEV['stamps'], DEV['fit'], DEV['var'], background=True, circular=False)
    expect(ctx.lib, 3, 'mpsfr_fit_stamps_observed', [CTX, I(5), DEVP(DEV['stamps']), DEVP(DEV['var']), I(3),
                                                     DEVP(DEV['fit']), I(1)])


# mpsfr_fit_stamps_psf(ctx, nstamp, stamps, var, npsf, psf, psf_index, shift, flags, fit_out, on_device): flags
# 1 background, 4 fixed shift
def test_fit_stamps_psf(ctx):
    model = _rng.uniform(0.1, 1.0, (2, NS, NS))
    index = np.array([0, 1, 1, 0, 1])
    shift = _rng.uniform(-2.0, 2.0, (5, 2))
    out = ctx.fit_stamps_psf(STAMPS, STAMPS)
    assert out.shape == (5, NFIT_PSF) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_fit_stamps_psf', [CTX, I(5), V(STAMPS), NULL, I(5), V(STAMPS), NULL, NULL, I(1), OUT(out),
                                                I(0)])
    out = ctx.fit_stamps_psf(STAMPS, model, var=VAR, psf_index=index, shift=shift, background=False, fixed_shift=True)
    expect(ctx.lib, 1, 'mpsfr_fit_stamps_psf', [CTX, I(5), V(STAMPS), V(VAR), I(2), V(model), V(index, np.int32),
                                                V(shift), I(4), OUT(out), I(0)])
    assert ctx.fit_stamps_psf_device(5, DEV['stamps'], 5, DEV['model'], DEV['fit']) is None
    expect(ctx.lib, 2, 'mpsfr_fit_stamps_psf', [CTX, I(5), DEVP(DEV['stamps']), NULL, I(5), DEVP(DEV['model']), NULL,
                                                NULL, I(1), DEVP(DEV['fit']), I(1)])
    ctx.fit_stamps_psf_device(5, DEV['stamps'], 2, DEV['model'], DEV['fit'], var_ptr=DEV['var'],
                              psf_index_ptr=DEV['index'], shift_ptr=DEV['shift'], background=True, fixed_shift=True)
    expect(ctx.lib, 3, 'mpsfr_fit_stamps_psf', [CTX, I(5), DEVP(DEV['stamps']), DEVP(DEV['var']), I(2),
                                                DEVP(DEV['model']), DEVP(DEV['index']), DEVP(DEV['shift']), I(5),
                                                DEVP(DEV['fit']), I(1)])


# mpsfr_stamp_metrics(ctx, nstamp, stamps, centers, nrad, radii_px, nbox, boxes_px, nfrac, fractions, out, on_device)
def test_stamp_metrics(ctx):
    rad, box, frac = [2.0, 5.0, 9.5], [4.0], [0.5, 0.8]
    cen = _rng.uniform(15.0, 25.0, (5, 2))
    out = ctx.stamp_metrics(STAMPS, rad, box, frac)
    assert out.shape == (5, NMET_HEAD + 6) and out.dtype == np.float64
    expect(ctx.lib, 0, 'mpsfr_stamp_metrics', [CTX, I(5), V(STAMPS), NULL, I(3), D(rad), I(1), D(box), I(2), D(frac),
                                               OUT(out), I(0)])
    out = ctx.stamp_metrics(STAMPS, rad, None, None, centers=cen)
    assert out.shape == (5, NMET_HEAD + 3)
    expect(ctx.lib, 1, 'mpsfr_stamp_metrics', [CTX, I(5), V(STAMPS), V(cen), I(3), D(rad), I(0), D([]), I(0), D([]),
                                               OUT(out), I(0)])
    assert ctx.stamp_metrics_device(5, DEV['stamps'], DEV['fit'], rad, box, frac) is None
    expect(ctx.lib, 2, 'mpsfr_stamp_metrics', [CTX, I(5), DEVP(DEV['stamps']), NULL, I(3), D(rad), I(1), D(box), I(2),
                                               D(frac), DEVP(DEV['fit']), I(1)])
    ctx.stamp_metrics_device(5, DEV['stamps'], DEV['fit'], rad, box, frac, centers_ptr=DEV['centers'])
    expect(ctx.lib, 3, 'mpsfr_stamp_metrics', [CTX, I(5), DEVP(DEV['stamps']), DEVP(DEV['centers']), I(3), D(rad), I(1),
                                               D(box), I(2), D(frac), DEVP(DEV['fit']), I(1)])


# ---- mpsfr_reconstruct_multi(ctxs, nctx, ntask, seeing, gl, l0, three_lgs, h, wind_speed, npsflin, nl, lbda_nm,
#                              mask_rec, mask_res, psf_out, psf_sum_out, fit_out) and its _async form
def _expect_multi(lib, index, name, arrays, masks=False):
    got_name, args = lib.calls[index]
    assert got_name == name and len(args) == 17
    assert [args[0][k] for k in range(2)] == [HANDLE, HANDLE + 0x10]           # (the array of context handles)
    m = [U8(MREC.ravel()), U8(MRES.ravel())] if masks else [NULL, NULL]
    rest = StubLib()
    rest.calls.append((got_name, args[1:]))
    expect(rest, 0, name, [I(2)] + ROWS + [D(HH), F(9.5), I(2), I(3), D(LB)] + m
           + [out_or_null(arrays[k]) for k in ('psf', 'psf_sum', 'fit')])


def test_reconstruct_multi():
    ctxs = [make_ctx(HANDLE), make_ctx(HANDLE + 0x10)]
    try:
        r = Context.reconstruct_multi(ctxs, LB, SEE, GL, L0, THREE, HH, wind_speed=9.5, npsflin=2, want_sum=False)
        shapes(r, (2, 3, NS, NS), None, (2, 3, NFIT))
        assert len(ctxs[0].lib.calls) == 1 and ctxs[1].lib.calls == []
        _expect_multi(ctxs[0].lib, 0, 'mpsfr_reconstruct_multi', r)
        assert ctxs[0]._pending == {} and ctxs[1]._pending == {}

        p = Context.reconstruct_multi_async(ctxs, LB, SEE, GL, L0, THREE, HH, wind_speed=9.5, npsflin=2,
                                            masks=(MREC, MRES))
        assert isinstance(p, PendingMulti)
        shapes(p._arrays, (2, 3, NS, NS), (3, NS, NS), (2, 3, NFIT))
        _expect_multi(ctxs[0].lib, 1, 'mpsfr_reconstruct_multi_async', p._arrays, masks=True)
        # every context keeps the arrays alive under the ticket of its shard: the stub of context 0 has seen two
        # mpsfr_reconstruct* calls (ticket 1), that of context 1 none (ticket -1: no shard, nothing registered)
        assert ctxs[0]._pending == {('multi', 1): p._arrays} and ctxs[1]._pending == {}
        assert p.wait() is p._arrays
        name, args = ctxs[0].lib.calls[2]
        assert name == 'mpsfr_wait_multi' and len(args) == 2 and args[1] == 2
        assert [args[0][k] for k in range(2)] == [HANDLE, HANDLE + 0x10]
        assert ctxs[0]._pending == {} and ctxs[1]._pending == {}
    finally:
        for c in ctxs:
            c._h = None


def test_h_needs_two_layers(ctx):
    for call in (lambda: ctx.reconstruct(LB, SEE, GL, L0, THREE, (100.0, 5000.0, 10000.0)),
                 lambda: Context.reconstruct_multi([ctx], LB, SEE, GL, L0, THREE, (100.0,)),
                 lambda: ctx.reconstruct_field(LB, SEE, GL, L0, THREE, (100.0,), POS)):
        with pytest.raises(ValueError):
            call()
    assert ctx.lib.calls == []
