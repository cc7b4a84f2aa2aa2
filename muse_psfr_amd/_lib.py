"""ctypes binding of libmpsfr.so (include/mpsfr.h).  No CPU fallback: if the HIP library is
missing or cannot be loaded this module raises.  Here: the binding and the Context that calls it.  What the header
says about arguments -- its limits and flag values and the validators of every call -- is _args.py."""
import ctypes as C
import os

import numpy as np

# every limit, validator and helper of _args stays reachable as _lib.NAME (its __all__ says which names these are)
from ._args import *        # noqa: F401,F403
from ._args import flag

HERE = os.path.dirname(os.path.abspath(__file__))
# MPSFR_LIB_PATH: load another build of the library (kernel experiments, scripts/variants.py)
LIB_PATH = os.environ.get('MPSFR_LIB_PATH') or os.path.join(HERE, 'libmpsfr.so')

_lib = None


class MpsfrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('libmpsfr error %d: %s' % (code, msg))
        self.code = code


def _preload_hip_runtime():
    """One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (same SONAME as
    /opt/rocm's).  If libmpsfr.so pulled in the system runtime first and torch were imported
    later, the process would hold two runtimes and the second finds no GPU.  So when torch is
    installed, its runtime is loaded first (without importing torch) and libmpsfr binds to it."""
    import importlib.util
    try:
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], 'lib', 'libamdhip64.so')
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load():
    """Load libmpsfr.so (built by muse_psfr_amd._build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError('%s not found: build it with `python -m muse_psfr_amd._build` '
                          '(hipcc, gfx950); there is no CPU fallback' % LIB_PATH)
    _preload_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    p = C.c_void_p
    dp = C.POINTER(C.c_double)
    u8p = C.POINTER(C.c_uint8)
    lib.mpsfr_create.argtypes = [C.POINTER(p), C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]
    lib.mpsfr_create.restype = C.c_int
    lib.mpsfr_destroy.argtypes = [p]
    lib.mpsfr_destroy.restype = None
    lib.mpsfr_last_error.argtypes = []
    lib.mpsfr_last_error.restype = C.c_char_p
    lib.mpsfr_set_option.argtypes = [p, C.c_char_p, C.c_double]
    lib.mpsfr_set_option.restype = C.c_int
    lib.mpsfr_reconstruct.argtypes = [p, C.c_int, dp, dp, dp, u8p, dp, C.c_double, C.c_int,
                                      C.c_int, dp, u8p, u8p, p, p, p, C.c_int]
    lib.mpsfr_reconstruct.restype = C.c_int
    lib.mpsfr_reconstruct_field.argtypes = [p, C.c_int, dp, dp, dp, u8p, dp, C.c_double, C.c_int, dp,
                                            C.c_int, dp, u8p, u8p, p, p, p, C.c_int]
    lib.mpsfr_reconstruct_field.restype = C.c_int
    lib.mpsfr_reconstruct_profile.argtypes = [p, C.c_int, dp, dp, dp, u8p, C.c_int, dp, dp, dp, dp, C.c_int, C.c_int,
                                              dp, C.c_int, dp, u8p, u8p, p, p, p, C.c_int]
    lib.mpsfr_reconstruct_profile.restype = C.c_int
    lib.mpsfr_simul_psd_profile.argtypes = [p, C.c_double, C.c_double, C.c_int, C.c_int, dp, dp, dp, dp, C.c_int,
                                            C.c_int, dp, u8p, u8p, dp]
    lib.mpsfr_simul_psd_profile.restype = C.c_int
    lib.mpsfr_reconstruct_band.argtypes = [p, C.c_int, dp, dp, dp, u8p, dp, C.c_double, C.c_int, C.c_int, dp,
                                           C.c_int, dp, C.c_int, dp, u8p, u8p, p, p, p, C.c_int]
    lib.mpsfr_reconstruct_band.restype = C.c_int
    lib.mpsfr_reconstruct_multi.argtypes = [C.POINTER(p), C.c_int, C.c_int, dp, dp, dp, u8p, dp, C.c_double,
                                            C.c_int, C.c_int, dp, u8p, u8p, p, p, p]
    lib.mpsfr_reconstruct_multi.restype = C.c_int
    lib.mpsfr_reconstruct_multi_async.argtypes = lib.mpsfr_reconstruct_multi.argtypes
    lib.mpsfr_reconstruct_multi_async.restype = C.c_int
    lib.mpsfr_wait_multi.argtypes = [C.POINTER(p), C.c_int]
    lib.mpsfr_wait_multi.restype = C.c_int
    lib.mpsfr_fit_stamps.argtypes = [p, C.c_int, p, p, C.c_int]
    lib.mpsfr_fit_stamps.restype = C.c_int
    lib.mpsfr_fit_stamps_elliptical.argtypes = [p, C.c_int, p, p, C.c_int]
    lib.mpsfr_fit_stamps_elliptical.restype = C.c_int
    lib.mpsfr_fit_stamps_observed.argtypes = [p, C.c_int, p, p, C.c_int, p, C.c_int]
    lib.mpsfr_fit_stamps_observed.restype = C.c_int
    lib.mpsfr_fit_stamps_psf.argtypes = [p, C.c_int, p, p, C.c_int, p, p, p, C.c_int, p, C.c_int]
    lib.mpsfr_fit_stamps_psf.restype = C.c_int
    lib.mpsfr_fit_groups_psf.argtypes = [p, C.c_int, C.c_int, p, p, C.c_int, p, p, p, C.c_int, p, C.c_int]
    lib.mpsfr_fit_groups_psf.restype = C.c_int
    lib.mpsfr_fit_spectra_psf.argtypes = [p, C.c_int, C.c_int, p, p, C.c_int, p, p, p, p, C.c_int, p, C.c_int]
    lib.mpsfr_fit_spectra_psf.restype = C.c_int
    lib.mpsfr_stamp_metrics.argtypes = [p, C.c_int, p, p, C.c_int, dp, C.c_int, dp, C.c_int, dp, p, C.c_int]
    lib.mpsfr_stamp_metrics.restype = C.c_int
    lib.mpsfr_cut_stamps.argtypes = [p, C.c_int, C.c_int, p, p, C.c_int, p, p, p, C.c_int]
    lib.mpsfr_cut_stamps.restype = C.c_int
    lib.mpsfr_render_stars.argtypes = [p, C.c_int, C.c_int, p, C.c_int, C.c_int, p, p, p, p, p, C.c_int, p, p, C.c_int]
    lib.mpsfr_render_stars.restype = C.c_int
    lib.mpsfr_find_stars.argtypes = [p, C.c_int, C.c_int, p, p, p, C.c_int, C.c_int, C.c_double, C.c_int, p, p, p, p,
                                     C.c_int]
    lib.mpsfr_find_stars.restype = C.c_int
    lib.mpsfr_frame_background.argtypes = [p, C.c_int, C.c_int, C.c_int, p, p, C.c_int, C.c_int, C.c_double, C.c_int,
                                           C.c_double, p, p, p, p, p, p, C.c_int]
    lib.mpsfr_frame_background.restype = C.c_int
    lib.mpsfr_group_stars.argtypes = [p, C.c_int, C.c_int, C.c_int, p, C.c_int, C.c_double, C.c_int, p, p, p, p, p,
                                      C.c_int]
    lib.mpsfr_group_stars.restype = C.c_int
    lib.mpsfr_fit_frame_psf.argtypes = [p, C.c_int, C.c_int, p, p, C.c_int, C.c_int, p, p, p, p, p, C.c_double, C.c_int,
                                        C.c_int, C.c_double, p, p, p, C.c_int]
    lib.mpsfr_fit_frame_psf.restype = C.c_int
    lib.mpsfr_fit_frame_psf_free.argtypes = [p, C.c_int, C.c_int, p, p, C.c_int, C.c_int, p, p, p, p, p, C.c_double,
                                             C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double,
                                             C.c_double, p, p, p, p, C.c_int]
    lib.mpsfr_fit_frame_psf_free.restype = C.c_int
    lib.mpsfr_fit_cube_psf.argtypes = [p, C.c_int, C.c_int, C.c_int, p, p, C.c_int, C.c_int, p, p, p, p, p, p, C.c_double,
                                       C.c_int, C.c_int, C.c_double, C.c_int, p, p, p, C.c_int]
    lib.mpsfr_fit_cube_psf.restype = C.c_int
    lib.mpsfr_fit_cube_psf_free.argtypes = [p, C.c_int, C.c_int, C.c_int, p, p, C.c_int, C.c_int, p, p, p, p, p, p,
                                            C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double,
                                            C.c_double, C.c_double, p, p, p, p, p, p, C.c_int]
    lib.mpsfr_fit_cube_psf_free.restype = C.c_int
    lib.mpsfr_simul_psd.argtypes = [p, C.c_double, C.c_double, C.c_double, C.c_int, dp, C.c_double, C.c_int, u8p, u8p, dp]
    lib.mpsfr_simul_psd.restype = C.c_int
    lib.mpsfr_psf_from_psd.argtypes = [p, C.c_int, dp, C.c_int, dp, dp]
    lib.mpsfr_psf_from_psd.restype = C.c_int
    lib.mpsfr_psd_to_psf.argtypes = [p, C.c_int, dp, C.c_int, dp, dp, C.c_double, C.c_int, dp, C.c_int, p, C.c_int]
    lib.mpsfr_psd_to_psf.restype = C.c_int
    lib.mpsfr_convolve_stamps.argtypes = [p, C.c_int, dp, dp, dp, C.c_int, dp, dp, dp]
    lib.mpsfr_convolve_stamps.restype = C.c_int
    lib.mpsfr_fit_rows.argtypes = [dp, C.c_long, C.c_double, dp, C.c_long]
    lib.mpsfr_fit_rows.restype = C.c_int
    lib.mpsfr_sync.argtypes = [p]
    lib.mpsfr_sync.restype = C.c_int
    lib.mpsfr_last_ticket.argtypes = [p]
    lib.mpsfr_last_ticket.restype = C.c_long
    lib.mpsfr_wait.argtypes = [p, C.c_long]
    lib.mpsfr_wait.restype = C.c_int
    lib.mpsfr_abandon.argtypes = [p]
    lib.mpsfr_abandon.restype = C.c_int
    lib.mpsfr_stream.argtypes = [p]
    lib.mpsfr_stream.restype = C.c_void_p
    lib.mpsfr_stream_wait.argtypes = [p, C.c_void_p]
    lib.mpsfr_stream_wait.restype = C.c_int
    lib.mpsfr_wait_event.argtypes = [p, C.c_void_p]
    lib.mpsfr_wait_event.restype = C.c_int
    lib.mpsfr_host_time.argtypes = [p, dp, C.POINTER(C.c_long)]
    lib.mpsfr_host_time.restype = C.c_int
    lib.mpsfr_debug_fetch.argtypes = [p, C.c_char_p, dp, C.c_size_t]
    lib.mpsfr_debug_fetch.restype = C.c_long
    lib.mpsfr_profile_count.argtypes = []
    lib.mpsfr_profile_count.restype = C.c_int
    lib.mpsfr_profile_name.argtypes = [C.c_int]
    lib.mpsfr_profile_name.restype = C.c_char_p
    lib.mpsfr_profile_get.argtypes = [p, C.c_int, dp, C.POINTER(C.c_long)]
    lib.mpsfr_profile_get.restype = C.c_int
    lib.mpsfr_profile_reset.argtypes = [p]
    lib.mpsfr_profile_reset.restype = C.c_int
    lib.mpsfr_version.argtypes = []
    lib.mpsfr_version.restype = C.c_int
    lib.mpsfr_device_count.argtypes = []
    lib.mpsfr_device_count.restype = C.c_int
    lib.mpsfr_build_id.argtypes = []
    lib.mpsfr_build_id.restype = C.c_char_p
    _lib = lib
    return lib


EXPORTS = ['mpsfr_create', 'mpsfr_destroy', 'mpsfr_last_error', 'mpsfr_set_option',
           'mpsfr_reconstruct', 'mpsfr_reconstruct_field', 'mpsfr_reconstruct_profile', 'mpsfr_simul_psd_profile', 'mpsfr_reconstruct_band', 'mpsfr_reconstruct_multi', 'mpsfr_reconstruct_multi_async', 'mpsfr_wait_multi', 'mpsfr_fit_stamps', 'mpsfr_fit_stamps_elliptical', 'mpsfr_fit_stamps_observed', 'mpsfr_fit_stamps_psf', 'mpsfr_fit_groups_psf', 'mpsfr_fit_spectra_psf', 'mpsfr_stamp_metrics', 'mpsfr_cut_stamps', 'mpsfr_render_stars', 'mpsfr_find_stars', 'mpsfr_group_stars', 'mpsfr_fit_frame_psf', 'mpsfr_fit_frame_psf_free', 'mpsfr_fit_cube_psf', 'mpsfr_fit_cube_psf_free', 'mpsfr_frame_background', 'mpsfr_simul_psd', 'mpsfr_psf_from_psd',
           'mpsfr_psd_to_psf',
           'mpsfr_convolve_stamps', 'mpsfr_fit_rows', 'mpsfr_sync', 'mpsfr_last_ticket', 'mpsfr_wait', 'mpsfr_abandon',
           'mpsfr_stream', 'mpsfr_stream_wait', 'mpsfr_wait_event',
           'mpsfr_host_time', 'mpsfr_debug_fetch',
           'mpsfr_profile_count', 'mpsfr_profile_name', 'mpsfr_profile_get',
           'mpsfr_profile_reset', 'mpsfr_version', 'mpsfr_build_id', 'mpsfr_device_count']


def fit_rows(fit, pixscale, out):
    """mpsfr_fit_rows: the 14 fit columns of FIT_ROWS from library fit rows `fit` (n, NFIT) into `out`, a C-contiguous
    float64 (n, stride >= 14) block whose first 14 columns receive them."""
    f = np.ascontiguousarray(fit, dtype=np.float64).reshape(-1, NFIT)
    assert out.dtype == np.float64 and out.ndim == 2 and out.shape[0] == f.shape[0] and out.strides[1] == 8
    _check(load().mpsfr_fit_rows(_dptr(f), f.shape[0], float(pixscale), out.ctypes.data_as(C.POINTER(C.c_double)),
                                 out.strides[0] // 8))


def device_count():
    """HIP devices visible to this process (0 without a GPU)."""
    return int(load().mpsfr_device_count())


def _check(rc):
    if rc < 0:
        raise MpsfrError(rc, load().mpsfr_last_error().decode())
    return rc


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _u8ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))


def _vptr(a):
    """void* of a host array (None: NULL)."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _devptr(v):
    """void* of a raw device pointer (an int; None or 0: NULL)."""
    return C.c_void_p(int(v)) if v else None


def _host_outs(arrays):
    return [_vptr(arrays[k]) for k in ('psf', 'psf_sum', 'fit')]


def _device_outs(psf_ptr, sum_ptr, fit_ptr):
    return [_devptr(psf_ptr), _devptr(sum_ptr), _devptr(fit_ptr)]


def _masks(masks):
    """(mask_rec, mask_res) of a call as flat uint8 arrays, or (None, None)."""
    if masks is None:
        return None, None
    mrec = np.ascontiguousarray(masks[0]).astype(np.uint8).reshape(-1)
    mres = np.ascontiguousarray(masks[1]).astype(np.uint8).reshape(-1)
    assert mrec.size == DIM_AO * DIM_AO and mres.size == DIM_AO * DIM_AO
    return mrec, mres


class Context:
    """One GPU context: grid size, precision, HIP stream, workspaces."""

    def __init__(self, dim=1280, pixscale=0.2, dimpsf=40, precision='mixed', device=0):
        self.lib = load()
        self.dim, self.pixscale, self.dimpsf = int(dim), float(pixscale), int(dimpsf)
        self.precision = precision
        prec = {'mixed': PREC_MIXED, 'f64': PREC_F64}[precision]
        h = C.c_void_p()
        _check(self.lib.mpsfr_create(C.byref(h), int(device), self.dim, self.dimpsf,
                                     self.pixscale, prec))
        self._h = h
        # Output arrays of asynchronous host-output calls not yet handed over, by ticket: the library holds
        # raw pointers to them (it writes them in mpsfr_wait, in mpsfr_sync, or when the ring of four comes
        # round again), so the context keeps them alive until then -- a PendingResult that is dropped
        # without wait() leaves no dangling pointer behind.
        self._pending = {}
        self._abandoned = set()

    def close(self):
        if getattr(self, '_h', None):
            self.lib.mpsfr_destroy(self._h)        # (destroys the ring without writing to any caller array)
            self._h = None
            self._pending = {}

    __del__ = close

    def set_option(self, key, value):
        _check(self.lib.mpsfr_set_option(self._h, key.encode(), float(value)))

    def sync(self):
        _check(self.lib.mpsfr_sync(self._h))
        self._pending.clear()

    def abandon(self):
        """Drop every asynchronous host-output call not yet waited for (mpsfr_abandon): the GPU drains, the
        library forgets the output arrays without writing to them, the context stays usable.  For error paths."""
        try:
            _check(self.lib.mpsfr_abandon(self._h))
        finally:
            self._abandoned.update(t for t in self._pending if not isinstance(t, tuple))
            self._pending.clear()

    def _handed_over(self, upto):
        for t in [t for t in self._pending if (t[1] if isinstance(t, tuple) else t) <= upto]:
            del self._pending[t]

    def wait_event(self, hip_event):
        """The next reconstruct call waits on the GPU for this recorded hipEvent_t (an integer
        handle, e.g. torch.cuda.Event.cuda_event)."""
        _check(self.lib.mpsfr_wait_event(self._h, C.c_void_p(int(hip_event))))

    def stream_wait(self, hip_stream):
        """Make the caller's stream (an integer hipStream_t, e.g. torch.cuda.current_stream().cuda_stream) wait on the
        GPU for every call made so far (mpsfr_stream_wait): the cheap form of waiting on stream_handle()."""
        _check(self.lib.mpsfr_stream_wait(self._h, C.c_void_p(int(hip_stream))))

    def host_time(self):
        """(seconds spent inside mpsfr_reconstruct, calls) since the last profile_reset()."""
        sec, n = C.c_double(), C.c_long()
        _check(self.lib.mpsfr_host_time(self._h, C.byref(sec), C.byref(n)))
        return sec.value, n.value

    def stream_handle(self):
        """hipStream_t of the context as an integer (for torch.cuda.ExternalStream)."""
        return int(self.lib.mpsfr_stream(self._h) or 0)

    def _finish(self, arrays, _async):
        """What a host-output call returns: the arrays, or for an asynchronous call a PendingResult, the arrays kept
        alive under the call's ticket until the library has written them."""
        if not _async:
            return arrays
        ticket = int(self.lib.mpsfr_last_ticket(self._h))
        self._pending[ticket] = arrays
        self._handed_over(ticket - 4)        # the call itself handed over the ticket four calls back
        return PendingResult(self, ticket, arrays)

    def _outputs(self, lead, planes, want_psf, want_sum, want_fit):
        """dict(psf, psf_sum, fit) of new host arrays (None where not wanted): `lead` is (rows,) or (rows, npos), the
        sum drops the row axis, `planes` is the number of wavelengths or bands."""
        n = self.dimpsf
        return dict(psf=np.empty(lead + (planes, n, n)) if want_psf else None,
                    psf_sum=np.empty(lead[1:] + (planes, n, n)) if want_sum else None,
                    fit=np.empty(lead + (planes, NFIT)) if want_fit else None)

    def reconstruct_async(self, *args, **kwargs):
        """`reconstruct` without waiting for the GPU (on_device = 2): returns a PendingResult whose
        .wait() blocks until the call has finished and returns the same dict.  Up to four such calls
        are in flight per context, overlapping on the pipeline lanes; they complete in order."""
        return self.reconstruct(*args, _async=True, **kwargs)

    def _call_reconstruct(self, inputs, npsflin, outs, on_device):
        seeing, gl, l0, lbda, three, hh, wind_speed, mrec, mres = inputs
        _check(self.lib.mpsfr_reconstruct(
            self._h, seeing.size, _dptr(seeing), _dptr(gl), _dptr(l0), _u8ptr(three), _dptr(hh),
            float(wind_speed), int(npsflin), lbda.size, _dptr(lbda), _u8ptr(mrec), _u8ptr(mres), *outs, on_device))

    def reconstruct(self, lbda, seeing, gl, l0, three_lgs=None, h=(100, 10000), wind_speed=None,
                    npsflin=1, masks=None, want_psf=True, want_sum=True, want_fit=True, _async=False):
        """Host-buffer call.  Returns dict(psf, psf_sum, fit) of float64 arrays (or None)."""
        inputs = self._inputs(lbda, seeing, gl, l0, three_lgs, h, wind_speed, masks)
        arrays = self._outputs((inputs[0].size,), inputs[3].size, want_psf, want_sum, want_fit)
        self._call_reconstruct(inputs, npsflin, _host_outs(arrays), 2 if _async else 0)
        return self._finish(arrays, _async)

    def reconstruct_device(self, lbda, seeing, gl, l0, three_lgs, h, wind_speed, npsflin, masks,
                           psf_ptr, sum_ptr, fit_ptr):
        """Device-buffer call (asynchronous): the three outputs are raw device pointers (int or
        None) on this context's GPU, e.g. torch tensors' data_ptr()."""
        inputs = self._inputs(lbda, seeing, gl, l0, three_lgs, h, wind_speed, masks)
        self._call_reconstruct(inputs, npsflin, _device_outs(psf_ptr, sum_ptr, fit_ptr), 1)

    def reconstruct_field_async(self, *args, **kwargs):
        """`reconstruct_field` without waiting for the GPU (on_device = 2): returns a PendingResult."""
        return self.reconstruct_field(*args, _async=True, **kwargs)

    def _call_field(self, inputs, pos, outs, on_device):
        seeing, gl, l0, lbda, three, hh, wind_speed, mrec, mres = inputs
        _check(self.lib.mpsfr_reconstruct_field(
            self._h, seeing.size, _dptr(seeing), _dptr(gl), _dptr(l0), _u8ptr(three), _dptr(hh),
            float(wind_speed), pos.shape[0], _dptr(pos), lbda.size, _dptr(lbda), _u8ptr(mrec), _u8ptr(mres),
            *outs, on_device))

    def reconstruct_field(self, lbda, seeing, gl, l0, three_lgs=None, h=(100, 10000), positions=((0.0, 0.0),),
                          wind_speed=None, masks=None, want_psf=True, want_sum=True, want_fit=True, _async=False):
        """Field-resolved host-buffer call (mpsfr_reconstruct_field): one stamp and one fit per (row, position,
        wavelength) at `positions` ((npos, 2) arcsec, npos <= 25).  Returns dict(psf (nt, npos, nl, 40, 40),
        psf_sum (npos, nl, 40, 40), fit (nt, npos, nl, NFIT)) of float64 arrays (or None)."""
        pos = field_positions(positions)
        inputs = self._inputs(lbda, seeing, gl, l0, three_lgs, h, wind_speed, masks)
        arrays = self._outputs((inputs[0].size, pos.shape[0]), inputs[3].size, want_psf, want_sum, want_fit)
        self._call_field(inputs, pos, _host_outs(arrays), 2 if _async else 0)
        return self._finish(arrays, _async)

    def reconstruct_field_device(self, lbda, seeing, gl, l0, three_lgs, h, wind_speed, positions, masks,
                                 psf_ptr, sum_ptr, fit_ptr):
        """Device-buffer field call (asynchronous, on_device = 1): outputs are raw device pointers (int or None)
        on this context's GPU, shaped as in reconstruct_field."""
        pos = field_positions(positions)
        inputs = self._inputs(lbda, seeing, gl, l0, three_lgs, h, wind_speed, masks)
        self._call_field(inputs, pos, _device_outs(psf_ptr, sum_ptr, fit_ptr), 1)

    def reconstruct_band_async(self, *args, **kwargs):
        """`reconstruct_band` without waiting for the GPU (on_device = 2): returns a PendingResult."""
        return self.reconstruct_band(*args, _async=True, **kwargs)

    def _band_inputs(self, lbda, weights, seeing, gl, l0, three_lgs, h, wind_speed, npsflin, positions, masks):
        """Checked inputs of a band call, as a ValueError before the library is touched: (the row inputs, the
        weights, npsflin as C takes it, pos or None)."""
        inputs = self._inputs(lbda, seeing, gl, l0, three_lgs, h, wind_speed, masks)
        w = band_weight_matrix(weights, inputs[3].size)
        npsflin, _, pos = _grid_or_positions(npsflin, positions)
        return inputs, w, npsflin, pos

    def _call_band(self, inputs, w, npsflin, pos, outs, on_device):
        seeing, gl, l0, lbda, three, hh, wind_speed, mrec, mres = inputs
        _check(self.lib.mpsfr_reconstruct_band(
            self._h, seeing.size, _dptr(seeing), _dptr(gl), _dptr(l0), _u8ptr(three), _dptr(hh), float(wind_speed),
            npsflin, 0 if pos is None else pos.shape[0], None if pos is None else _dptr(pos), lbda.size, _dptr(lbda),
            w.shape[0], _dptr(w), _u8ptr(mrec), _u8ptr(mres), *outs, on_device))

    def reconstruct_band(self, lbda, weights, seeing, gl, l0, three_lgs=None, h=(100, 10000), wind_speed=None,
                         npsflin=None, positions=None, masks=None, want_psf=True, want_sum=True, want_fit=True,
                         _async=False):
        """Band-integrated host-buffer call (mpsfr_reconstruct_band): the stamps reduced over wavelength with
        `weights` ((nband, nl), each band normalised to sum 1 by the library; see band_weights in psfrec.py) and the
        Moffat fit of every band stamp.  positions=None: the npsflin directions averaged (npsflin None means 1),
        dict(psf (nt, nband, 40, 40), psf_sum (nband, 40, 40), fit (nt, nband, NFIT)); else (npos, 2) arcsec, each
        output gaining an npos axis after the row axis, with npsflin left at None (or 0): a call with positions
        evaluates no npsflin grid."""
        inputs, w, npsflin, pos = self._band_inputs(lbda, weights, seeing, gl, l0, three_lgs, h, wind_speed, npsflin,
                                                    positions, masks)
        nt = inputs[0].size
        arrays = self._outputs((nt,) if pos is None else (nt, pos.shape[0]), w.shape[0], want_psf, want_sum, want_fit)
        self._call_band(inputs, w, npsflin, pos, _host_outs(arrays), 2 if _async else 0)
        return self._finish(arrays, _async)

    def reconstruct_band_device(self, lbda, weights, seeing, gl, l0, three_lgs, h, wind_speed, npsflin, positions,
                                masks, psf_ptr, sum_ptr, fit_ptr):
        """Device-buffer band call (asynchronous, on_device = 1): outputs are raw device pointers (int or None) on
        this context's GPU, shaped as in reconstruct_band."""
        inputs, w, npsflin, pos = self._band_inputs(lbda, weights, seeing, gl, l0, three_lgs, h, wind_speed, npsflin,
                                                    positions, masks)
        self._call_band(inputs, w, npsflin, pos, _device_outs(psf_ptr, sum_ptr, fit_ptr), 1)

    def reconstruct_profile_async(self, *args, **kwargs):
        """`reconstruct_profile` without waiting for the GPU (on_device = 2): returns a PendingResult."""
        return self.reconstruct_profile(*args, _async=True, **kwargs)

    def _profile_inputs(self, lbda, seeing, gl, l0, three_lgs, h, wind_speed, wind_dir, cn2, npsflin, positions,
                        masks):
        """Checked inputs of a profile call: every refusal of mpsfr_reconstruct_profile, as a ValueError, before
        the library is touched.  (The row inputs, the layers (h, wind_speed, wind_dir), the weights, npsflin as C
        takes it, pos or None.)"""
        layers = profile_layers(h, wind_speed, wind_dir)
        inputs = self._inputs(lbda, seeing, gl, l0, three_lgs, (0.0, 0.0), 0.0, masks)
        w = profile_weights(cn2, inputs[0].size, layers[0].size)
        npsflin, _, pos = _grid_or_positions(npsflin, positions)
        return inputs, layers, w, npsflin, pos

    def _call_profile(self, inputs, layers, w, npsflin, pos, outs, on_device):
        seeing, gl, l0, lbda, three, _, _, mrec, mres = inputs
        hh, ws, wd = layers
        _check(self.lib.mpsfr_reconstruct_profile(
            self._h, seeing.size, _dptr(seeing), _dptr(gl), _dptr(l0), _u8ptr(three), hh.size, _dptr(hh), _dptr(ws),
            _dptr(wd), _dptr(w), npsflin, 0 if pos is None else pos.shape[0], None if pos is None else _dptr(pos),
            lbda.size, _dptr(lbda), _u8ptr(mrec), _u8ptr(mres), *outs, on_device))

    def reconstruct_profile(self, lbda, seeing, gl, l0, cn2, h, wind_speed, wind_dir, three_lgs=None, npsflin=None,
                            positions=None, masks=None, want_psf=True, want_sum=True, want_fit=True, _async=False):
        """Host-buffer call with a Cn2 profile (mpsfr_reconstruct_profile): layers h / wind_speed / wind_dir
        ([nlayer], m, m/s, rad), weights cn2 ([nrow, nlayer] or one [nlayer] row for all).  positions=None: the
        npsflin directions averaged, shaped as `reconstruct`; else (npos, 2) arcsec with npsflin = 0, shaped as
        `reconstruct_field`."""
        inputs, layers, w, npsflin, pos = self._profile_inputs(
            lbda, seeing, gl, l0, three_lgs, h, wind_speed, wind_dir, cn2, npsflin, positions, masks)
        nt = inputs[0].size
        arrays = self._outputs((nt,) if pos is None else (nt, pos.shape[0]), inputs[3].size, want_psf, want_sum,
                               want_fit)
        self._call_profile(inputs, layers, w, npsflin, pos, _host_outs(arrays), 2 if _async else 0)
        return self._finish(arrays, _async)

    def reconstruct_profile_device(self, lbda, seeing, gl, l0, cn2, h, wind_speed, wind_dir, three_lgs, npsflin,
                                   positions, masks, psf_ptr, sum_ptr, fit_ptr):
        """Device-buffer profile call (asynchronous, on_device = 1): outputs are raw device pointers (int or None)
        on this context's GPU, shaped as in reconstruct_profile."""
        inputs, layers, w, npsflin, pos = self._profile_inputs(
            lbda, seeing, gl, l0, three_lgs, h, wind_speed, wind_dir, cn2, npsflin, positions, masks)
        self._call_profile(inputs, layers, w, npsflin, pos, _device_outs(psf_ptr, sum_ptr, fit_ptr), 1)

    def simul_psd_profile(self, seeing, l0, cn2, h, wind_speed, wind_dir, three_lgs=False, npsflin=1, positions=None,
                          masks=None):
        """simul_psd_wfm for a Cn2 profile (mpsfr_simul_psd_profile): (ndir, dim, dim) PSD, centred, reference
        units; ndir = npsflin^2, or npos with positions (npsflin = 0)."""
        hh, ws, wd = profile_layers(h, wind_speed, wind_dir)
        w = profile_weights(cn2, 1, hh.size)
        # (npsflin defaults to 1 here, so positions simply replace it)
        npsflin, npos, pos = _grid_or_positions(npsflin if positions is None else None, positions)
        mrec, mres = _masks(masks)
        out = np.empty((npos or npsflin ** 2, self.dim, self.dim))
        _check(self.lib.mpsfr_simul_psd_profile(
            self._h, float(seeing), float(l0), int(bool(three_lgs)), hh.size, _dptr(hh), _dptr(ws), _dptr(wd),
            _dptr(w), npsflin, npos, None if pos is None else _dptr(pos), _u8ptr(mrec), _u8ptr(mres), _dptr(out)))
        return out

    @staticmethod
    def _inputs(lbda, seeing, gl, l0, three_lgs, h, wind_speed, masks):
        """The inputs every reconstruct call shares, as C takes them: (seeing, gl, l0, lbda, three_lgs, h, wind_speed,
        mask_rec, mask_res)."""
        seeing = np.ascontiguousarray(np.atleast_1d(seeing), dtype=np.float64)
        gl = np.ascontiguousarray(np.atleast_1d(gl), dtype=np.float64)
        l0 = np.ascontiguousarray(np.atleast_1d(l0), dtype=np.float64)
        lbda = np.ascontiguousarray(np.atleast_1d(lbda), dtype=np.float64)
        three = np.zeros(seeing.size, np.uint8) if three_lgs is None else \
            np.ascontiguousarray(np.atleast_1d(three_lgs)).astype(np.uint8)
        if wind_speed is None:
            wind_speed = float(np.full_like(np.array(h), 12.5)[0])      # psfrec.py:61
        hh = np.ascontiguousarray(h, dtype=np.float64)
        if hh.size != 2:
            raise ValueError('exactly two layers are supported (psfrec.py:66)')
        return (seeing, gl, l0, lbda, three, hh, wind_speed) + _masks(masks)

    @staticmethod
    def reconstruct_multi_async(ctxs, *args, **kwargs):
        """`reconstruct_multi` without waiting for the GPUs (mpsfr_reconstruct_multi_async): every context takes its
        shard as an asynchronous host-output call; returns a PendingMulti whose .wait() (mpsfr_wait_multi) returns the
        same dict.  One such call may be pending per ctxs[0]."""
        return Context.reconstruct_multi(ctxs, *args, _async=True, **kwargs)

    @staticmethod
    def reconstruct_multi(ctxs, lbda, seeing, gl, l0, three_lgs=None, h=(100, 10000), wind_speed=None,
                          npsflin=1, masks=None, want_psf=True, want_sum=True, want_fit=True, _async=False):
        """`reconstruct` with the rows in contiguous shards over several contexts (one per device,
        one host thread each inside the library: mpsfr_reconstruct_multi) -- the reference's joblib
        fan-out (psfrec.py:1082-1083).  Same outputs as the single-context call."""
        ctxs = list(ctxs)
        seeing, gl, l0, lbda, three, hh, wind_speed, mrec, mres = Context._inputs(lbda, seeing, gl, l0, three_lgs, h,
                                                                                 wind_speed, masks)
        arrays = ctxs[0]._outputs((seeing.size,), lbda.size, want_psf, want_sum, want_fit)
        handles = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
        fn = ctxs[0].lib.mpsfr_reconstruct_multi_async if _async else ctxs[0].lib.mpsfr_reconstruct_multi
        if _async:
            # the refusals the library makes BEFORE it queues anything are made here, with nothing touched:
            # whatever the library itself reports below is a failed shard, after which it has abandoned every
            # pending asynchronous call of every context of the call
            if any(isinstance(t, tuple) for t in ctxs[0]._pending):
                raise MpsfrError(-1, 'a multi-context call is pending on this context: wait for it first')
            c0 = ctxs[0]
            if any((c.dim, c.dimpsf, c.pixscale, c.precision) != (c0.dim, c0.dimpsf, c0.pixscale, c0.precision)
                   for c in ctxs[1:]):
                raise MpsfrError(-1, 'the contexts must share dim, dimpsf, pixscale and precision')
        try:
            _check(fn(handles, len(ctxs), seeing.size, _dptr(seeing), _dptr(gl), _dptr(l0), _u8ptr(three), _dptr(hh),
                      float(wind_speed), int(npsflin), lbda.size, _dptr(lbda), _u8ptr(mrec), _u8ptr(mres),
                      *_host_outs(arrays)))
        except MpsfrError:
            if _async:
                # The library abandoned the shards it had queued on ctxs[0..k-1]; earlier reconstruct_async tickets
                # of the failing and the later contexts are still pending in C with pointers into arrays this side
                # would otherwise forget.  abandon() on EVERY context makes the two sides agree: the library drains
                # and drops what it holds, and the tickets land in `_abandoned` so that a later wait() raises
                # instead of handing back arrays nobody wrote.
                for c in ctxs:
                    c.abandon()
            raise
        if _async:
            # the library holds pointers into `arrays` until mpsfr_wait_multi: every context keeps them alive
            # under the ticket of its shard
            for c in ctxs:
                t = int(c.lib.mpsfr_last_ticket(c._h))
                if t >= 0:
                    c._pending[('multi', t)] = arrays
            return PendingMulti(ctxs, handles, arrays)
        return arrays

    def simul_psd(self, seeing, gl, l0, three_lgs=False, h=(100, 10000), wind_speed=None, npsflin=1, masks=None):
        """simul_psd_wfm (psfrec.py:36-151): (npsflin^2, dim, dim) PSD, centred, reference units."""
        if wind_speed is None:
            wind_speed = float(np.full_like(np.array(h), 12.5)[0])      # psfrec.py:61
        hh = np.ascontiguousarray(h, dtype=np.float64)
        mrec, mres = _masks(masks)
        out = np.empty((int(npsflin) ** 2, self.dim, self.dim))
        _check(self.lib.mpsfr_simul_psd(self._h, float(seeing), float(gl), float(l0), int(bool(three_lgs)), _dptr(hh),
                                        float(wind_speed), int(npsflin), _u8ptr(mrec), _u8ptr(mres), _dptr(out)))
        return out

    def psf_from_psd(self, psd, lbda):
        """psf_muse (psfrec.py:644-686): PSD (dim, dim) or (ndir, dim, dim) -> (nl, 40, 40) stamps before the
        convolutions."""
        psd = np.ascontiguousarray(psd, dtype=np.float64)
        if psd.ndim == 2:
            psd = psd[None]
        if psd.shape[1:] != (self.dim, self.dim):
            raise ValueError('the PSD must be %d x %d for this context' % (self.dim, self.dim))
        lbda = np.ascontiguousarray(np.atleast_1d(lbda), dtype=np.float64)
        out = np.empty((lbda.size, self.dimpsf, self.dimpsf))
        _check(self.lib.mpsfr_psf_from_psd(self._h, psd.shape[0], _dptr(psd), lbda.size, _dptr(lbda), _dptr(out)))
        return out

    def psd_to_psf(self, psd, pup, D, lbda_m, phase_static=None, dimnum=None, out=None):
        """mpsfr_psd_to_psf (psd_to_psf, psfrec.py:689-807): PSD (dim, dim) or (npsd, dim, dim), pupil (npup, npup),
        wavelengths in metres -> (npsd, nl, dimnum, dimnum) full PSFs, each of sum 1.  phase_static is in metres
        (see include/mpsfr.h).  dimnum defaults to dim.  `out`: None (a new host array), or a device pointer (an int,
        e.g. a torch tensor's data_ptr()) to npsd * nl * dimnum^2 float64 on this context's device."""
        psd = np.ascontiguousarray(psd, dtype=np.float64)
        if psd.ndim == 2:
            psd = psd[None]
        if psd.ndim != 3 or psd.shape[1:] != (self.dim, self.dim):
            raise ValueError('the PSD must be %d x %d for this context' % (self.dim, self.dim))
        pup = np.ascontiguousarray(pup, dtype=np.float64)
        if pup.ndim != 2 or pup.shape[0] != pup.shape[1]:
            raise ValueError('the pupil must be a square 2-D array')
        ph = None
        if phase_static is not None:
            ph = np.ascontiguousarray(phase_static, dtype=np.float64)
            if ph.shape != pup.shape:
                raise ValueError('phase_static must have the shape of the pupil %s, not %s' % (pup.shape, ph.shape))
        lbda_m = np.ascontiguousarray(np.atleast_1d(lbda_m), dtype=np.float64).ravel()
        dimnum = self.dim if dimnum is None else int(dimnum)
        res = np.empty((psd.shape[0], lbda_m.size, dimnum, dimnum)) if out is None else None
        _check(self.lib.mpsfr_psd_to_psf(self._h, psd.shape[0], _dptr(psd), pup.shape[0], _dptr(pup),
                                         None if ph is None else _dptr(ph), float(D), lbda_m.size, _dptr(lbda_m),
                                         dimnum, _vptr(res) if out is None else C.c_void_p(int(out)),
                                         0 if out is None else 1))
        return res

    def convolve_stamps(self, lbda, seeing, gl, l0, psf):
        """convolve_final_psf (psfrec.py:874-930) on (ntask, nl, 40, 40) stamps (or (nl, 40, 40) for one task)."""
        lbda = np.ascontiguousarray(np.atleast_1d(lbda), dtype=np.float64)
        seeing = np.ascontiguousarray(np.atleast_1d(seeing), dtype=np.float64)
        gl = np.ascontiguousarray(np.atleast_1d(gl), dtype=np.float64)
        l0 = np.ascontiguousarray(np.atleast_1d(l0), dtype=np.float64)
        st = np.ascontiguousarray(psf, dtype=np.float64)
        single = st.ndim == 3
        st = st.reshape(seeing.size, lbda.size, self.dimpsf, self.dimpsf)
        out = np.empty_like(st)
        _check(self.lib.mpsfr_convolve_stamps(self._h, seeing.size, _dptr(seeing), _dptr(gl), _dptr(l0), lbda.size,
                                              _dptr(lbda), _dptr(st), _dptr(out)))
        return out[0] if single else out

    # ---- the stamp family.  Every C function's arguments are built once, by a _call_* method that takes host arrays
    # (on_device = 0) or raw device pointers (on_device = 1; None or 0 is NULL) in the same places.

    def _call_fit(self, fn, nstamp, stamps, fit, on_device):
        p = _devptr if on_device else _vptr
        _check(fn(self._h, int(nstamp), p(stamps), p(fit), on_device))

    def _call_fit_observed(self, nstamp, stamps, var, flags, fit, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_fit_stamps_observed(self._h, int(nstamp), p(stamps), p(var), flags, p(fit), on_device))

    def _call_fit_psf(self, nstamp, stamps, var, npsf, psf, index, shift, flags, fit, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_fit_stamps_psf(self._h, int(nstamp), p(stamps), p(var), int(npsf), p(psf), p(index),
                                             p(shift), flags, p(fit), on_device))

    def _call_fit_groups(self, nstamp, nsrc, stamps, var, npsf, psf, index, shift, flags, fit, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_fit_groups_psf(self._h, int(nstamp), int(nsrc), p(stamps), p(var), int(npsf), p(psf),
                                             p(index), p(shift), flags, p(fit), on_device))

    def _call_fit_spectra(self, nstar, nl, cubes, var, npsf, psf, index, shift, x, flags, fit, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_fit_spectra_psf(self._h, int(nstar), int(nl), p(cubes), p(var), int(npsf), p(psf),
                                              p(index), p(shift), None if x is None else _dptr(x), flags, p(fit),
                                              on_device))

    def _call_metrics(self, nstamp, stamps, centers, rad, box, frac, out, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_stamp_metrics(self._h, int(nstamp), p(stamps), p(centers), rad.size, _dptr(rad),
                                            box.size, _dptr(box), frac.size, _dptr(frac), p(out), on_device))

    def fit_stamps(self, stamps):
        st = np.ascontiguousarray(stamps, dtype=np.float64).reshape(-1, self.dimpsf, self.dimpsf)
        out = np.empty((st.shape[0], NFIT))
        self._call_fit(self.lib.mpsfr_fit_stamps, st.shape[0], st, out, 0)
        return out

    def fit_stamps_device(self, nstamp, stamps_ptr, fit_ptr):
        """Device-buffer circular fit (asynchronous, on_device = 1): `stamps_ptr` ([nstamp][dimpsf][dimpsf] float64)
        and `fit_ptr` ([nstamp][NFIT] float64) are raw device pointers (int) on this context's GPU; the call is
        queued on the context stream, after any device-output reconstruct of this context."""
        _positive_int('nstamp', nstamp)
        _device_pointers(stamps_ptr=stamps_ptr, fit_ptr=fit_ptr)
        self._call_fit(self.lib.mpsfr_fit_stamps, nstamp, stamps_ptr, fit_ptr, 1)

    def fit_stamps_elliptical(self, stamps):
        """Elliptical Moffat fit (mpsfr_fit_stamps_elliptical) of stamps (..., dimpsf, dimpsf): (n, NFIT_ELL) rows."""
        st = elliptical_stamps(stamps, self.dimpsf)
        out = np.empty((st.shape[0], NFIT_ELL))
        self._call_fit(self.lib.mpsfr_fit_stamps_elliptical, st.shape[0], st, out, 0)
        return out

    def fit_stamps_elliptical_device(self, nstamp, stamps_ptr, fit_ptr):
        """Device-buffer elliptical fit (asynchronous, on_device = 1): `stamps_ptr` ([nstamp][dimpsf][dimpsf] float64)
        and `fit_ptr` ([nstamp][NFIT_ELL] float64) are raw device pointers (int) on this context's GPU; the call is
        queued on the context stream, after any device-output reconstruct of this context."""
        _positive_int('nstamp', nstamp)
        _device_pointers(stamps_ptr=stamps_ptr, fit_ptr=fit_ptr)
        self._call_fit(self.lib.mpsfr_fit_stamps_elliptical, nstamp, stamps_ptr, fit_ptr, 1)

    def fit_stamps_observed(self, stamps, var=None, background=True, circular=True):
        """Weighted Moffat fit of observed stars (mpsfr_fit_stamps_observed) of stamps (..., dimpsf, dimpsf): (n, NFIT_ELL)
        rows in the elliptical layout, with 21 background, 22 err_background, 23 the number of used pixels.  `var`: the
        variance of every pixel (same shape), or None for unit weights.  A NaN pixel, or one whose variance is not
        finite and > 0, is masked.  `background`: fit a constant background; `circular`: a circular Moffat."""
        st, va = observed_stamps(stamps, var, self.dimpsf)
        flags = observed_flags(background, circular)
        out = np.empty((st.shape[0], NFIT_ELL))
        self._call_fit_observed(st.shape[0], st, va, flags, out, 0)
        return out

    def fit_stamps_observed_device(self, nstamp, stamps_ptr, fit_ptr, var_ptr=None, background=True, circular=True):
        """Device-buffer form (asynchronous, on_device = 1): `stamps_ptr` and `var_ptr` ([nstamp][dimpsf][dimpsf]
        float64; var_ptr None: unit weights) and `fit_ptr` ([nstamp][NFIT_ELL] float64) are raw device pointers (int) on
        this context's GPU; the call is queued on the context stream, after any device-output reconstruct of this
        context."""
        _positive_int('nstamp', nstamp)
        _device_pointers(stamps_ptr=stamps_ptr, fit_ptr=fit_ptr)
        flags = observed_flags(background, circular)
        self._call_fit_observed(nstamp, stamps_ptr, var_ptr, flags, fit_ptr, 1)

    def fit_stamps_psf(self, stamps, psf, var=None, psf_index=None, shift=None, background=True, fixed_shift=False):
        """PSF-model fit of observed stars (mpsfr_fit_stamps_psf): the model stamps `psf` (..., dimpsf, dimpsf), resampled
        by cubic convolution, are fitted to the stars `stamps` (..., dimpsf, dimpsf) in a scale F, a shift (dp, dq) in
        pixels and, with `background`, a constant.  (n, NFIT_PSF) rows: 0 F, 1 dp, 2 dq, 3 back, 4 chi2, 5 iterations,
        6-9 their errors, 10 status, 11 the number of used pixels, 12 flux = F sum(psf), 13 err_flux.  `var` and the
        mask as fit_stamps_observed.  `psf_index`: (n,) the model stamp of every star, or None for one model stamp per
        star in order.  `shift`: (n, 2) start values of (dp, dq), or None for the difference of the brightest pixels;
        `fixed_shift`: hold them (then `shift` is required and the problem is linear)."""
        st, va = observed_stamps(stamps, var, self.dimpsf)
        ps, ix, sh, flags = psf_fit_arguments(st.shape[0], psf, psf_index, shift, background, fixed_shift, self.dimpsf)
        out = np.empty((st.shape[0], NFIT_PSF))
        self._call_fit_psf(st.shape[0], st, va, ps.shape[0], ps, ix, sh, flags, out, 0)
        return out

    def fit_stamps_psf_device(self, nstamp, stamps_ptr, npsf, psf_ptr, fit_ptr, var_ptr=None, psf_index_ptr=None,
                              shift_ptr=None, background=True, fixed_shift=False):
        """Device-buffer form (asynchronous, on_device = 1): `stamps_ptr`, `var_ptr` ([nstamp][dimpsf][dimpsf] float64;
        var_ptr None: unit weights), `psf_ptr` ([npsf][dimpsf][dimpsf] float64), `psf_index_ptr` ([nstamp] int32, or None
        with npsf == nstamp), `shift_ptr` ([nstamp][2] float64, or None) and `fit_ptr` ([nstamp][NFIT_PSF] float64) are
        raw device pointers (int) on this context's GPU; the call is queued on the context stream, after any
        device-output reconstruct of this context.  An index out of range or a shift outside the domain makes that
        row status 2."""
        _positive_int('nstamp', nstamp)
        _positive_int('npsf', npsf)
        _device_pointers(stamps_ptr=stamps_ptr, psf_ptr=psf_ptr, fit_ptr=fit_ptr)
        _model_per_star(npsf, nstamp, psf_index_ptr, 'nstamp')
        flags = psf_fit_flags(background, fixed_shift)
        if fixed_shift and not shift_ptr:
            raise ValueError('fixed_shift needs shift_ptr')
        self._call_fit_psf(nstamp, stamps_ptr, var_ptr, npsf, psf_ptr, psf_index_ptr, shift_ptr, flags, fit_ptr, 1)

    def fit_groups_psf(self, stamps, psf, shift, var=None, psf_index=None, background=True, mode='free'):
        """PSF-model fit of blended stars (mpsfr_fit_groups_psf): every stamp (..., dimpsf, dimpsf) holds the same number
        K = 2 .. MAX_GROUP of sources of its model stamp, at the positions `shift` (n, K, 2) in pixels from the model
        stamp's own position; all K are fitted at once.  mode: 'free' (F_k, dp_k, dq_k; `shift` holds the start values),
        'common' (F_k and one offset of all positions; `shift` holds catalogue positions) or 'fixed' (F_k only, closed
        form); with `background` a constant b.  `var`, the mask and `psf_index` as fit_stamps_psf.  (n, NFIT_GROUP)
        rows: 0 back, 1 err_back, 2 chi2, 3 iterations, 4 status, 5 n_used, 6 K; source k at 8 + 8k: F, dp, dq, err_F,
        err_dp, err_dq, flux = F sum(psf), err_flux; 40 .. 45 the correlation coefficients of (F_i, F_j) for (0,1),
        (0,2), (0,3), (1,2), (1,3), (2,3)."""
        st, va = observed_stamps(stamps, var, self.dimpsf)
        ps, ix, sh, flags = group_fit_arguments(st.shape[0], psf, psf_index, shift, background, mode, self.dimpsf)
        out = np.empty((st.shape[0], NFIT_GROUP))
        self._call_fit_groups(st.shape[0], sh.shape[1], st, va, ps.shape[0], ps, ix, sh, flags, out, 0)
        return out

    def fit_groups_psf_device(self, nstamp, nsrc, stamps_ptr, npsf, psf_ptr, shift_ptr, fit_ptr, var_ptr=None,
                              psf_index_ptr=None, background=True, mode='free'):
        """Device-buffer form (asynchronous, on_device = 1): `stamps_ptr`, `var_ptr` ([nstamp][dimpsf][dimpsf] float64;
        var_ptr None: unit weights), `psf_ptr` ([npsf][dimpsf][dimpsf] float64), `psf_index_ptr` ([nstamp] int32, or None
        with npsf == nstamp), `shift_ptr` ([nstamp][nsrc][2] float64) and `fit_ptr` ([nstamp][NFIT_GROUP] float64) are
        raw device pointers (int) on this context's GPU; the call is queued on the context stream, after any
        device-output reconstruct of this context.  An index out of range or a position that is not finite or outside
        the domain makes that row status 2."""
        _positive_int('nstamp', nstamp)
        _positive_int('npsf', npsf)
        _group_size(nsrc)
        _device_pointers(stamps_ptr=stamps_ptr, psf_ptr=psf_ptr, shift_ptr=shift_ptr, fit_ptr=fit_ptr)
        _model_per_star(npsf, nstamp, psf_index_ptr, 'nstamp')
        flags = group_fit_flags(background, mode)
        self._call_fit_groups(nstamp, nsrc, stamps_ptr, var_ptr, npsf, psf_ptr, psf_index_ptr, shift_ptr, flags,
                              fit_ptr, 1)

    def fit_spectra_psf(self, cubes, psf, var=None, psf_index=None, shift=None, background=True, x=None):
        """PSF-model fit of star cubes (mpsfr_fit_spectra_psf): every star is a cube (n, nl, dimpsf, dimpsf) of nl images
        that share one position (dp, dq) -- with `x` (nl values in [-1, 1]) a position dp + sp x_l, dq + sq x_l that
        drifts linearly -- and have a scale F_l and, with `background`, a constant b_l per layer.  `psf`: the model cubes
        (npsf, nl, dimpsf, dimpsf); `psf_index` (n,) or None for one model cube per star in order; `shift` (n, 2) start
        values of (dp, dq), or None for the difference of the brightest pixels of the collapsed images (bright stars
        only); `var` and the mask as fit_stamps_psf.  Returns (head, layers): head (n, NFIT_SPEC): 0 dp, 1 dq, 2 sp,
        3 sq, 4-7 their errors, 8 chi2, 9 iterations, 10 status, 11 used pixels, 12 fitted layers, 13 dof; layers (n, nl,
        NFIT_SPEC_LAYER): 0 F, 1 back, 2 err_F, 3 err_back, 4 flux = F sum(psf_l), 5 err_flux, 6 chi2_l, 7 n_used_l,
        8 status_l (2: the layer was left out)."""
        cu, va, ps, ix, sh, xx, flags = spectra_fit_arguments(cubes, var, psf, psf_index, shift, background, x, self.dimpsf)
        n, nl = cu.shape[:2]
        out = np.empty((n, NFIT_SPEC + NFIT_SPEC_LAYER * nl))
        self._call_fit_spectra(n, nl, cu, va, ps.shape[0], ps, ix, sh, xx, flags, out, 0)
        return out[:, :NFIT_SPEC].copy(), out[:, NFIT_SPEC:].reshape(n, nl, NFIT_SPEC_LAYER).copy()

    def fit_spectra_psf_device(self, nstar, nl, cubes_ptr, npsf, psf_ptr, fit_ptr, var_ptr=None, psf_index_ptr=None,
                               shift_ptr=None, background=True, x=None):
        """Device-buffer form (asynchronous, on_device = 1): `cubes_ptr`, `var_ptr` ([nstar][nl][dimpsf][dimpsf] float64;
        var_ptr None: unit weights), `psf_ptr` ([npsf][nl][dimpsf][dimpsf] float64), `psf_index_ptr` ([nstar] int32, or
        None with npsf == nstar), `shift_ptr` ([nstar][2] float64, or None) and `fit_ptr` ([nstar][NFIT_SPEC +
        NFIT_SPEC_LAYER nl] float64) are raw device pointers (int) on this context's GPU; `x` stays a host array.  The
        call is queued on the context stream, after any device-output reconstruct of this context.  An index out of
        range or a start outside the domain makes that row status 2."""
        _positive_int('nstar', nstar)
        _positive_int('npsf', npsf)
        _spec_layers(nl)
        _device_pointers(cubes_ptr=cubes_ptr, psf_ptr=psf_ptr, fit_ptr=fit_ptr)
        _model_per_star(npsf, nstar, psf_index_ptr)
        flags, xx = spectra_fit_flags(background, x, nl)
        self._call_fit_spectra(nstar, nl, cubes_ptr, var_ptr, npsf, psf_ptr, psf_index_ptr, shift_ptr, xx, flags,
                               fit_ptr, 1)

    def stamp_metrics(self, stamps, radii_px, boxes_px, fractions, centers=None):
        """PSF energy metrics (mpsfr_stamp_metrics) of stamps (..., dimpsf, dimpsf): (n, NMET_HEAD + nrad + nbox +
        nfrac) rows -- flux, peak, peak_p, peak_q, cp, cq, status, 0, then the encircled energies at `radii_px`, the
        ensquared energies in the boxes of side `boxes_px` and the radii holding `fractions` of the flux (pixels).
        `centers`: (n, 2) (p, q) in pixels, or None for the centroid of each stamp."""
        st = metric_stamps(stamps, self.dimpsf)
        rad, box, frac = metric_parameters(radii_px, boxes_px, fractions, self.dimpsf)
        ce = None if centers is None else metric_centers(centers, st.shape[0])
        out = np.empty((st.shape[0], NMET_HEAD + rad.size + box.size + frac.size))
        self._call_metrics(st.shape[0], st, ce, rad, box, frac, out, 0)
        return out

    def stamp_metrics_device(self, nstamp, stamps_ptr, out_ptr, radii_px, boxes_px, fractions, centers_ptr=None):
        """Device-buffer metrics (asynchronous, on_device = 1): `stamps_ptr` ([nstamp][dimpsf][dimpsf] float64), `out_ptr`
        ([nstamp][NMET_HEAD + nrad + nbox + nfrac] float64) and `centers_ptr` ([nstamp][2] float64, or None for the
        centroids) are raw device pointers (int) on this context's GPU; the call is queued on the context stream,
        after any device-output reconstruct of this context."""
        _positive_int('nstamp', nstamp)
        _device_pointers(stamps_ptr=stamps_ptr, out_ptr=out_ptr)
        rad, box, frac = metric_parameters(radii_px, boxes_px, fractions, self.dimpsf)
        self._call_metrics(nstamp, stamps_ptr, centers_ptr, rad, box, frac, out_ptr, 1)

    def _call_cut(self, ny, nx, image, var, nstar, origin, stamps, var_out, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_cut_stamps(self._h, int(ny), int(nx), p(image), p(var), int(nstar), p(origin), p(stamps),
                                         p(var_out), on_device))

    def _call_render(self, ny, nx, image, nstar, npsf, psf, index, origin, shift, scale, flags, out, star_out, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_render_stars(self._h, int(ny), int(nx), p(image), int(nstar), int(npsf), p(psf), p(index),
                                           p(origin), p(shift), p(scale), flags, p(out), p(star_out), on_device))

    def cut_stamps(self, image, origin, var=None):
        """Stamps out of a frame (mpsfr_cut_stamps): `image` (ny, nx), `origin` (n, 2) integers, the frame pixel (row,
        column) of pixel [0][0] of every stamp, on or off the frame (|origin| <= 2^30).  Returns the (n, dimpsf, dimpsf)
        stamps, NaN where a stamp leaves the frame; with `var` (the frame's shape) also the variance stamps, 0 there:
        (stamps, var_stamps).  NaN and var <= 0 are the mask of the observed fits."""
        im, va = frame_images(image, var)
        og = star_origins(origin)
        n = og.shape[0]
        out = np.empty((n, self.dimpsf, self.dimpsf))
        vout = None if va is None else np.empty((n, self.dimpsf, self.dimpsf))
        self._call_cut(im.shape[0], im.shape[1], im, va, n, og, out, vout, 0)
        return out if va is None else (out, vout)

    def cut_stamps_device(self, ny, nx, image_ptr, nstar, origin_ptr, stamps_ptr, var_ptr=None, var_stamps_ptr=None):
        """Device-buffer form (asynchronous, on_device = 1): `image_ptr`, `var_ptr` ([ny][nx] float64; var_ptr None: no
        variances), `origin_ptr` ([nstar][2] int32), `stamps_ptr` and `var_stamps_ptr` ([nstar][dimpsf][dimpsf] float64;
        given exactly when var_ptr is) are raw device pointers (int) on this context's GPU; the call is queued on the
        context stream, after any device-output reconstruct of this context."""
        frame_shape(ny, nx)
        _positive_int('nstar', nstar)
        _device_pointers(image_ptr=image_ptr, origin_ptr=origin_ptr, stamps_ptr=stamps_ptr)
        if bool(var_ptr) != bool(var_stamps_ptr):
            raise ValueError('var_ptr and var_stamps_ptr must both be given or both be None')
        self._call_cut(ny, nx, image_ptr, var_ptr, nstar, origin_ptr, stamps_ptr, var_stamps_ptr, 1)

    def render_stars(self, psf, origin, scale, shift=None, psf_index=None, image=None, shape=None, subtract=False,
                     return_status=False):
        """Model stars into a frame (mpsfr_render_stars): star k is scale[k] times the model stamp psf[psf_index[k]]
        (psf[k] without psf_index), resampled by cubic convolution at the shift (dp, dq) in pixels (`shift` (n, 2), None:
        zeros), with pixel [0][0] of its stamp on the frame pixel origin[k] -- the (F, dp, dq) of fit_stamps_psf on a
        stamp cut at the same origin.  The stars are added to `image` (ny, nx), or to zeros of `shape` = (ny, nx); with
        `subtract` they are subtracted from `image`.  At every pixel the stars are summed in index order, so one call
        equals two calls over a split of the list, bit for bit.  Returns the frame; with `return_status` also the (n,
        NRENDER) rows: 0 status (0 rendered, 1 off the frame), 1 the frame pixels in the star's footprint."""
        im, ny, nx, ps, ix, og, sh, sc, flags = render_arguments(psf, origin, scale, shift, psf_index, image, shape,
                                                                 subtract, self.dimpsf)
        flag('return_status', return_status)
        n = og.shape[0]
        out = np.empty((ny, nx))
        rows = np.empty((n, NRENDER)) if return_status else None
        self._call_render(ny, nx, im, n, ps.shape[0], ps, ix, og, sh, sc, flags, out, rows, 0)
        return (out, rows) if return_status else out

    def render_stars_device(self, ny, nx, nstar, npsf, psf_ptr, origin_ptr, scale_ptr, image_out_ptr, image_ptr=None,
                            shift_ptr=None, psf_index_ptr=None, star_out_ptr=None, subtract=False):
        """Device-buffer form (asynchronous, on_device = 1): `psf_ptr` ([npsf][dimpsf][dimpsf] float64), `origin_ptr`
        ([nstar][2] int32), `scale_ptr` ([nstar] float64), `shift_ptr` ([nstar][2] float64, or None for zeros),
        `psf_index_ptr` ([nstar] int32, or None with npsf == nstar), `image_ptr` ([ny][nx] float64, or None for zeros),
        `image_out_ptr` ([ny][nx] float64; it may be image_ptr) and `star_out_ptr` ([nstar][NRENDER] float64, or None)
        are raw device pointers (int) on this context's GPU; the call is queued on the context stream, after any
        device-output reconstruct of this context.  An index out of range, a shift outside the domain, a scale that is
        not finite or an |origin| above 2^30 makes that star status 2: it is skipped."""
        frame_shape(ny, nx)
        _positive_int('nstar', nstar)
        _positive_int('npsf', npsf)
        _device_pointers(psf_ptr=psf_ptr, origin_ptr=origin_ptr, scale_ptr=scale_ptr, image_out_ptr=image_out_ptr)
        _model_per_star(npsf, nstar, psf_index_ptr)
        flags = render_flags(subtract)
        if subtract and not image_ptr:
            raise ValueError('subtract needs image_ptr')
        self._call_render(ny, nx, image_ptr, nstar, npsf, psf_ptr, psf_index_ptr, origin_ptr, shift_ptr, scale_ptr, flags,
                          image_out_ptr, star_out_ptr, 1)

    def _call_find(self, ny, nx, image, var, psf, half, sep, threshold, max_stars, rows, origin, count, tmap, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_find_stars(self._h, int(ny), int(nx), p(image), p(var), p(psf), int(half), int(sep),
                                         float(threshold), int(max_stars), p(rows), p(origin), p(count), p(tmap),
                                         on_device))

    def find_stars(self, image, psf, *, var=None, half=3, sep=3, threshold=5.0, max_stars=4096, return_map=False):
        """The stars of a frame (mpsfr_find_stars): the matched filter of `image` (ny, nx; `var` of the same shape or
        None) with the (2 half + 1)^2 core of the model stamp `psf` (dimpsf, dimpsf) beside a free local background,
        and the peaks of its statistic T (the significance with var, the amplitude without) at or above `threshold`
        that dominate the (2 sep + 1)^2 square around them.  Returns (rows[:n], origin[:n], nfound): the (n, NFIND)
        rows in pixel order -- 0 row and 1 column position with the parabola's sub-pixel offset, 2 T, 3 the amplitude (the
        `scale` of fit_stamps_psf), 4 the local background, 5 the sharpness (1 for the model, far above for a hot pixel),
        6 the valid pixels of the window, 7 flags --, the (n, 2) int32 origins cut_stamps and render_stars take, and the
        number of peaks in the frame; n = min(nfound, max_stars).  With `return_map` also T (ny, nx)."""
        im, va, ps, half, sep, threshold, max_stars = find_arguments(image, var, psf, half, sep, threshold, max_stars,
                                                                     self.dimpsf)
        flag('return_map', return_map)
        ny, nx = im.shape
        rows = np.empty((max_stars, NFIND))
        origin = np.empty((max_stars, 2), dtype=np.int32)
        count = np.zeros(1, dtype=np.int32)
        tmap = np.empty((ny, nx)) if return_map else None
        self._call_find(ny, nx, im, va, ps, half, sep, threshold, max_stars, rows, origin, count, tmap, 0)
        nfound = int(count[0])
        n = min(nfound, max_stars)
        return (rows[:n], origin[:n], nfound) + ((tmap,) if return_map else ())

    def find_stars_device(self, ny, nx, image_ptr, psf_ptr, half, sep, threshold, max_stars, star_out_ptr, count_ptr, *,
                          var_ptr=None, origin_ptr=None, map_ptr=None):
        """Device-buffer form (asynchronous, on_device = 1): `image_ptr`, `var_ptr` ([ny][nx] float64; None: no
        variances), `psf_ptr` ([dimpsf][dimpsf] float64), `star_out_ptr` ([max_stars][NFIND] float64), `count_ptr` ([1]
        int32), `origin_ptr` ([max_stars][2] int32, or None) and `map_ptr` ([ny][nx] float64, or None) are raw device
        pointers (int) on this context's GPU; the call is queued on the context stream, after any device-output
        reconstruct of this context.  The rows behind the count are NaN with the origin (-2^30, -2^30), which the frame
        calls and the fits skip, so that the next calls can run at the fixed size max_stars.  A core that is not
        finite or constant gives no peaks."""
        frame_shape(ny, nx)
        half, sep, threshold, max_stars = find_parameters(half, sep, threshold, max_stars, self.dimpsf)
        _device_pointers(image_ptr=image_ptr, psf_ptr=psf_ptr, star_out_ptr=star_out_ptr, count_ptr=count_ptr)
        self._call_find(ny, nx, image_ptr, var_ptr, psf_ptr, half, sep, threshold, max_stars, star_out_ptr, origin_ptr,
                        count_ptr, map_ptr, 1)

    def _call_background(self, nl, ny, nx, image, var, box, filter, kappa, max_clip, min_frac, apply_to, mesh, head, bmap,
                         rms, applied, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_frame_background(self._h, int(nl), int(ny), int(nx), p(image), p(var), int(box),
                                               int(filter), float(kappa), int(max_clip), float(min_frac), p(apply_to),
                                               p(mesh), p(head), p(bmap), p(rms), p(applied), on_device))

    def frame_background(self, image, var=None, *, box=32, filter=3, kappa=3.0, max_clip=5, min_frac=0.25, apply_to=None,
                         return_rms=True):
        """The background of a frame (ny, nx) or of every layer of a cube (nl, ny, nx) (mpsfr_frame_background): the
        median and 1.4826 MAD of every `box` x `box` cell (8 .. 64 pixels) under iterated clipping at `kappa` MADs-as-sigma
        (at most `max_clip` passes), over the valid pixels (finite, and `var` finite and > 0: var is a mask, nothing is
        weighted); a cell with fewer than `min_frac` of its pixels valid is filled from its neighbours; a median over
        `filter` x `filter` cells (1, 3, 5); cubic interpolation to the frame.  Returns (map, rms, mesh, head): the
        maps of the input's shape (rms None without `return_rms`), mesh (nl, my, mx, NBACK) -- 0 level, 1 rms, 2 raw
        level, 3 raw rms, 4 pixels used, 5 valid pixels, 6 clipping passes, 7 flags (BACK_FILLED, BACK_CLIP_CAP,
        BACK_FLAT) -- and head (nl, NBACK_HEAD): 0 status (0 fine, 1 some cells filled, 2 no valid cell), 1 valid and 2
        filled cells; without the layer axis for a frame.  With `apply_to` (the input's shape) also apply_to - map, as
        a fifth value."""
        im, va, ap, box, filter, kappa, max_clip, min_frac = background_arguments(image, var, apply_to, box, filter, kappa,
                                                                                  max_clip, min_frac)
        flag('return_rms', return_rms)
        nl = im.shape[0] if im.ndim == 3 else 1
        ny, nx = im.shape[-2:]
        my, mx = -(-ny // box), -(-nx // box)
        lead = im.shape[:-2]
        mesh = np.empty(lead + (my, mx, NBACK))
        head = np.empty(lead + (NBACK_HEAD,))
        bmap = np.empty(im.shape)
        rms = np.empty(im.shape) if return_rms else None
        applied = None if ap is None else np.empty(im.shape)
        self._call_background(nl, ny, nx, im, va, box, filter, kappa, max_clip, min_frac, ap, mesh, head, bmap, rms,
                              applied, 0)
        return (bmap, rms, mesh, head) + (() if ap is None else (applied,))

    def frame_background_device(self, nl, ny, nx, image_ptr, mesh_ptr, head_ptr, *, var_ptr=None, map_ptr=None,
                                rms_ptr=None, apply_to_ptr=None, applied_ptr=None, box=32, filter=3, kappa=3.0,
                                max_clip=5, min_frac=0.25):
        """Device-buffer form (asynchronous, on_device = 1): `image_ptr`, `var_ptr`, `apply_to_ptr`, `map_ptr`, `rms_ptr`
        and `applied_ptr` ([nl][ny][nx] float64; the optional ones None), `mesh_ptr` ([nl][my][mx][NBACK] float64) and
        `head_ptr` ([nl][NBACK_HEAD] float64) are raw device pointers (int) on this context's GPU; the call is queued on
        the context stream, after any device-output reconstruct of this context, without a host synchronisation.
        apply_to_ptr and applied_ptr are given together; they may be the same buffer, and applied_ptr may not be
        image_ptr."""
        nl, ny, nx = background_shape(nl, ny, nx)
        box, filter, kappa, max_clip, min_frac = background_parameters(box, filter, kappa, max_clip, min_frac)
        _device_pointers(image_ptr=image_ptr, mesh_ptr=mesh_ptr, head_ptr=head_ptr)
        if bool(apply_to_ptr) != bool(applied_ptr):
            raise ValueError('apply_to_ptr and applied_ptr must both be None or both be device pointers')
        if applied_ptr and int(applied_ptr) == int(image_ptr):
            raise ValueError('applied_ptr may not be image_ptr')
        self._call_background(nl, ny, nx, image_ptr, var_ptr, box, filter, kappa, max_clip, min_frac, apply_to_ptr,
                              mesh_ptr, head_ptr, map_ptr, rms_ptr, applied_ptr, 1)

    def _call_group(self, ny, nx, nstar, pos, stride, crit, max_groups, label, groups, origin, shift, count, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_group_stars(self._h, int(ny), int(nx), int(nstar), p(pos), int(stride), float(crit),
                                          int(max_groups), p(label), p(groups), p(origin), p(shift), p(count),
                                          on_device))

    def group_stars(self, pos, crit, shape, *, max_groups=None):
        """Friends-of-friends groups of stars (mpsfr_group_stars): `pos` (nstar, stride >= 2) holds (row, column) in its
        first two columns -- the rows of find_stars as they are --, rows with a NaN are fillers; `shape` = (ny, nx) is
        the frame; stars closer than `crit` pixels are linked and a group is a connected component.  Returns (label,
        groups[:n], origin[:n], shift[:n], counts): the (nstar,) int32 label of every star (the smallest index of its
        group; -1 for a filler), the (n, NGROUP) int32 group rows -- 0 members, 1 flags (GROUP_OVERSIZE, GROUP_WIDE),
        2 label, 4..7 the members ascending, -1 beyond them -- ordered by class (1, 2, 3, 4 members, oversize) and by
        label within a class, the (n, 2) int32 origins cut_stamps takes, the (n, MAX_GROUP, 2) shifts of the members
        from their stamp's centre pixel (0 beyond the members) and the six counts: all groups, then each class;
        n = min(counts[0], max_groups), and max_groups=None stands for nstar.  The library writes the shifts at the
        pitch of each class (group_shift_rows); here they are returned one group per row."""
        po, ny, nx, crit, max_groups = group_arguments(pos, crit, shape, max_groups)
        nstar, stride = po.shape
        label = np.empty(nstar, dtype=np.int32)
        groups = np.empty((max_groups, NGROUP), dtype=np.int32)
        origin = np.empty((max_groups, 2), dtype=np.int32)
        shift = np.empty((max_groups, MAX_GROUP, 2))
        counts = np.zeros(1 + MAX_GROUP + 1, dtype=np.int32)
        self._call_group(ny, nx, nstar, po, stride, crit, max_groups, label, groups, origin, shift, counts, 0)
        n = min(int(counts[0]), max_groups)
        return label, groups[:n], origin[:n], group_shift_rows(shift, counts)[:n], counts

    def group_stars_device(self, ny, nx, nstar, pos_ptr, stride, crit, max_groups, label_ptr, group_ptr, count_ptr, *,
                           origin_ptr=None, shift_ptr=None):
        """Device-buffer form (asynchronous, on_device = 1): `pos_ptr` ([nstar][stride] float64), `label_ptr` ([nstar]
        int32), `group_ptr` ([max_groups][NGROUP] int32), `count_ptr` ([6] int32), `origin_ptr` ([max_groups][2] int32)
        and `shift_ptr` ([max_groups][MAX_GROUP][2] float64; both or neither) are raw device pointers (int) on this
        context's GPU; the call is queued on the context stream.  With the counts c and offset_k = c[1] + .. + c[k - 1],
        origin_ptr + 8 offset_k bytes and shift_ptr + 64 offset_k bytes are what cut_stamps_device and
        fit_groups_psf_device (fit_stamps_psf_device for k = 1) take for the c[k] groups of k stars.  A position out of
        range is a filler with the label -2."""
        frame_shape(ny, nx)
        nstar, stride, crit, max_groups = group_parameters(nstar, stride, crit, max_groups)
        _device_pointers(pos_ptr=pos_ptr, label_ptr=label_ptr, group_ptr=group_ptr, count_ptr=count_ptr)
        if bool(origin_ptr) != bool(shift_ptr):
            raise ValueError('origin_ptr and shift_ptr must both be None or both be device pointers')
        self._call_group(ny, nx, nstar, pos_ptr, stride, crit, max_groups, label_ptr, group_ptr, origin_ptr, shift_ptr,
                         count_ptr, 1)

    def _call_frame_fit(self, ny, nx, image, var, nstar, npsf, psf, index, origin, shift, scale0, radius, flags, max_iter,
                        tol, rows, head, resid, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_fit_frame_psf(self._h, int(ny), int(nx), p(image), p(var), int(nstar), int(npsf), p(psf),
                                            p(index), p(origin), p(shift), p(scale0), float(radius), flags,
                                            int(max_iter), float(tol), p(rows), p(head), p(resid), on_device))

    def fit_frame_psf(self, image, psf, origin, *, var=None, shift=None, psf_index=None, scale0=None, radius=8.0,
                      background=True, max_iter=100, tol=1e-10, return_residual=False):
        """Crowded-field photometry (mpsfr_fit_frame_psf): the fluxes of all stars of `image` (ny, nx; `var` of the
        same shape or None) at once, star k being F_k times the model stamp psf[psf_index[k]] (psf[k] without
        psf_index) resampled at `shift` (n, 2) pixels with its stamp's pixel [0][0] on origin[k] -- as render_stars
        takes them.  One weighted linear least-squares problem over the valid pixels within `radius` (1 .. 20 pixels)
        of a star, with one constant if `background`, solved by preconditioned conjugate gradients from `scale0` (n,;
        None: zeros) to the relative residual `tol` or max_iter (1 .. 1000) steps.  Returns (rows, head) and, with
        return_residual, the frame minus the fitted stars.  rows (n, NFRAMEFIT): 0 F, 1 its conditional error (the
        other stars held fixed), 2 flux, 3 its error, 4 overlap (sum of the star's off-diagonal terms of the normal
        matrix over its diagonal term: 0 for a star alone), 5 valid pixels in its disc, 6 its diagonal term, 7 status
        (0 fitted, 1 off the frame, 2 left out).  head (NFRAMEFIT,): 0 b, 1 its error, 2 chi2, 3 pixels fitted, 4
        iterations, 5 the last relative residual, 6 stars fitted, 7 status (0 converged, 1 max_iter reached, 2 nothing
        fitted)."""
        im, va, ps, ix, og, sh, s0, radius, flags, max_iter, tol = frame_fit_arguments(
            image, var, psf, psf_index, origin, shift, scale0, radius, background, max_iter, tol, self.dimpsf)
        flag('return_residual', return_residual)
        ny, nx = im.shape
        n = og.shape[0]
        rows = np.empty((n, NFRAMEFIT))
        head = np.empty(NFRAMEFIT)
        resid = np.empty((ny, nx)) if return_residual else None
        self._call_frame_fit(ny, nx, im, va, n, ps.shape[0], ps, ix, og, sh, s0, radius, flags, max_iter, tol, rows, head,
                             resid, 0)
        return (rows, head) + ((resid,) if return_residual else ())

    def fit_frame_psf_device(self, ny, nx, image_ptr, nstar, npsf, psf_ptr, origin_ptr, star_out_ptr, head_ptr, *,
                             var_ptr=None, shift_ptr=None, psf_index_ptr=None, scale0_ptr=None, resid_ptr=None,
                             radius=8.0, background=True, max_iter=100, tol=1e-10):
        """Device-buffer form (asynchronous, on_device = 1): `image_ptr`, `var_ptr`, `resid_ptr` ([ny][nx] float64;
        var_ptr None: unit weights, resid_ptr None: no residual frame), `psf_ptr` ([npsf][dimpsf][dimpsf] float64),
        `origin_ptr` ([nstar][2] int32), `shift_ptr` ([nstar][2] float64, or None for zeros), `psf_index_ptr` ([nstar]
        int32, or None with npsf == nstar), `scale0_ptr` ([nstar] float64, or None for zeros), `star_out_ptr`
        ([nstar][NFRAMEFIT] float64) and `head_ptr` ([NFRAMEFIT] float64) are raw device pointers (int) on this
        context's GPU; the whole solve is queued on the context stream, after any device-output reconstruct of this
        context, without a host synchronisation.  An index out of range, a shift outside the domain or an |origin|
        above 2^30 makes that star status 2; the finder's filler rows are such stars."""
        nstar = _frame_fit_device(ny, nx, nstar, npsf, psf_index_ptr, image_ptr=image_ptr, psf_ptr=psf_ptr,
                                  origin_ptr=origin_ptr, star_out_ptr=star_out_ptr, head_ptr=head_ptr)
        radius, flags, max_iter, tol = frame_fit_parameters(radius, background, max_iter, tol)
        self._call_frame_fit(ny, nx, image_ptr, var_ptr, nstar, npsf, psf_ptr, psf_index_ptr, origin_ptr, shift_ptr,
                             scale0_ptr, radius, flags, max_iter, tol, star_out_ptr, head_ptr, resid_ptr, 1)

    def _call_frame_free(self, ny, nx, image, var, nstar, npsf, psf, index, origin, shift, scale0, radius, flags,
                         max_iter, tol, free, rows, shift_out, head, resid, on_device):
        p = _devptr if on_device else _vptr
        max_outer, pos_tol, max_step, max_move, min_snr = free
        _check(self.lib.mpsfr_fit_frame_psf_free(self._h, int(ny), int(nx), p(image), p(var), int(nstar), int(npsf),
                                                 p(psf), p(index), p(origin), p(shift), p(scale0), float(radius), flags,
                                                 int(max_iter), float(tol), int(max_outer), float(pos_tol),
                                                 float(max_step), float(max_move), float(min_snr), p(rows), p(shift_out),
                                                 p(head), p(resid), on_device))

    def fit_frame_psf_free(self, image, psf, origin, *, var=None, shift=None, psf_index=None, scale0=None, radius=8.0,
                           background=True, max_iter=100, tol=1e-10, max_outer=8, pos_tol=1e-3, max_step=0.5,
                           max_move=2.0, min_snr=3.0, return_residual=False):
        """Crowded-field photometry with free positions (mpsfr_fit_frame_psf_free): fit_frame_psf with the shifts of
        the stars as unknowns.  `shift` is the start; the valid pixels, the accepted stars and the discs of `radius`
        around the START centres are decided from it once.  An opening solve of the fluxes, then up to `max_outer`
        (0 .. 16) Gauss-Newton steps over the fluxes and the shifts of the free stars -- the accepted ones with
        F > min_snr err_F --, every step clipped per axis to `max_step` (0 .. 1] px and every shift to within `max_move`
        (0 .. 4] px of its start and 8 px of its origin, until the largest step is <= `pos_tol` px; then a closing
        solve at the final shifts.  Every inner solve is fit_frame_psf's, to `tol` relative to its right-hand side or
        `max_iter` steps.  Returns (rows, shifts, head) and, with return_residual, the frame minus the fitted stars at
        the final shifts.  rows (n, NFRAMEFREE): 0-7 as fit_frame_psf at the final shifts, 8-9 the final shift, 10-11
        its conditional errors, 12-13 final minus start, 14 flags (FRAME_FREE_HELD, FRAME_FREE_BOUND,
        FRAME_FREE_CLIPPED), 15 the outer steps in which the star was free.  shifts (n, 2): columns 8-9 as
        render_stars and fit_frame_psf take them.  head (NFRAMEFREE_HEAD,): 0-7 as fit_frame_psf for the closing solve
        (7: 0 only if the positions and the closing solve have both converged), 8 outer steps, 9 the last largest
        step, 10 free stars in the last step, 11 inner iterations in all."""
        im, va, ps, ix, og, sh, s0, radius, flags, max_iter, tol = frame_fit_arguments(
            image, var, psf, psf_index, origin, shift, scale0, radius, background, max_iter, tol, self.dimpsf)
        free = frame_free_parameters(max_outer, pos_tol, max_step, max_move, min_snr)
        flag('return_residual', return_residual)
        ny, nx = im.shape
        n = og.shape[0]
        rows = np.empty((n, NFRAMEFREE))
        shifts = np.empty((n, 2))
        head = np.empty(NFRAMEFREE_HEAD)
        resid = np.empty((ny, nx)) if return_residual else None
        self._call_frame_free(ny, nx, im, va, n, ps.shape[0], ps, ix, og, sh, s0, radius, flags, max_iter, tol, free,
                              rows, shifts, head, resid, 0)
        return (rows, shifts, head) + ((resid,) if return_residual else ())

    def fit_frame_psf_free_device(self, ny, nx, image_ptr, nstar, npsf, psf_ptr, origin_ptr, star_out_ptr,
                                  shift_out_ptr, head_ptr, *, var_ptr=None, shift_ptr=None, psf_index_ptr=None,
                                  scale0_ptr=None, resid_ptr=None, radius=8.0, background=True, max_iter=100, tol=1e-10,
                                  max_outer=8, pos_tol=1e-3, max_step=0.5, max_move=2.0, min_snr=3.0):
        """Device-buffer form (asynchronous, on_device = 1) of fit_frame_psf_free: the pointers of
        fit_frame_psf_device, with `star_out_ptr` ([nstar][NFRAMEFREE] float64), `shift_out_ptr` ([nstar][2] float64:
        what render_stars_device and fit_frame_psf_device take as shift_ptr) and `head_ptr` ([NFRAMEFREE_HEAD]
        float64).  The whole call -- every solve of every outer step -- is queued on the context stream without a host
        synchronisation."""
        nstar = _frame_fit_device(ny, nx, nstar, npsf, psf_index_ptr, image_ptr=image_ptr, psf_ptr=psf_ptr,
                                  origin_ptr=origin_ptr, star_out_ptr=star_out_ptr, shift_out_ptr=shift_out_ptr,
                                  head_ptr=head_ptr)
        radius, flags, max_iter, tol = frame_fit_parameters(radius, background, max_iter, tol)
        free = frame_free_parameters(max_outer, pos_tol, max_step, max_move, min_snr)
        self._call_frame_free(ny, nx, image_ptr, var_ptr, nstar, npsf, psf_ptr, psf_index_ptr, origin_ptr, shift_ptr,
                              scale0_ptr, radius, flags, max_iter, tol, free, star_out_ptr, shift_out_ptr, head_ptr,
                              resid_ptr, 1)

    def _call_cube_fit(self, nl, ny, nx, cube, var, nstar, npsf, psf, index, origin, shift, layer_shift, scale0, radius,
                       flags, max_iter, tol, layer_batch, rows, head, resid, on_device):
        p = _devptr if on_device else _vptr
        _check(self.lib.mpsfr_fit_cube_psf(self._h, int(nl), int(ny), int(nx), p(cube), p(var), int(nstar), int(npsf),
                                           p(psf), p(index), p(origin), p(shift), p(layer_shift), p(scale0),
                                           float(radius), flags, int(max_iter), float(tol), int(layer_batch), p(rows),
                                           p(head), p(resid), on_device))

    def fit_cube_psf(self, cube, psf, origin, *, var=None, shift=None, layer_shift=None, psf_index=None, scale0=None,
                     radius=8.0, background=True, max_iter=100, tol=1e-10, layer_batch=0, return_residual=False):
        """Crowded-field photometry of a cube (mpsfr_fit_cube_psf): fit_frame_psf on every layer of `cube` (nl, ny, nx;
        `var` of the same shape or None), the layers of a batch side by side on the GPU.  `psf` (npsf, nl, dimpsf,
        dimpsf): star k of layer l is psf[psf_index[k], l] (psf[k, l] without psf_index); origin, shift, psf_index per
        star for all layers; `layer_shift` (nl, 2) pixels or None, one offset per layer added to every star's shift
        (the sums must stay within FIT_PSF_MAX_SHIFT); `scale0` (nl, n) or None; `layer_batch` layers at once (0: as
        many as the library's budget of work memory holds).  Returns rows (nl, n, NFRAMEFIT), head (nl, NFRAMEFIT) and,
        with return_residual, the residual cube -- layer by layer the bits of fit_frame_psf on that layer."""
        cu, va, ps, ix, og, sh, ls, s0, radius, flags, max_iter, tol, layer_batch = cube_fit_arguments(
            cube, var, psf, psf_index, origin, shift, layer_shift, scale0, radius, background, max_iter, tol, layer_batch,
            self.dimpsf)
        flag('return_residual', return_residual)
        nl, ny, nx = cu.shape
        n = og.shape[0]
        rows = np.empty((nl, n, NFRAMEFIT))
        head = np.empty((nl, NFRAMEFIT))
        resid = np.empty((nl, ny, nx)) if return_residual else None
        self._call_cube_fit(nl, ny, nx, cu, va, n, ps.shape[0], ps, ix, og, sh, ls, s0, radius, flags, max_iter, tol,
                            layer_batch, rows, head, resid, 0)
        return (rows, head) + ((resid,) if return_residual else ())

    def fit_cube_psf_device(self, nl, ny, nx, cube_ptr, nstar, npsf, psf_ptr, origin_ptr, star_out_ptr, head_ptr, *,
                            var_ptr=None, shift_ptr=None, layer_shift_ptr=None, psf_index_ptr=None, scale0_ptr=None,
                            resid_ptr=None, radius=8.0, background=True, max_iter=100, tol=1e-10, layer_batch=0):
        """Device-buffer form (asynchronous, on_device = 1) of fit_cube_psf: `cube_ptr`, `var_ptr`, `resid_ptr`
        ([nl][ny][nx] float64), `psf_ptr` ([npsf][nl][dimpsf][dimpsf] float64), `origin_ptr`, `shift_ptr`,
        `psf_index_ptr` as for fit_frame_psf_device, `layer_shift_ptr` ([nl][2] float64 or None), `scale0_ptr`
        ([nl][nstar] float64 or None), `star_out_ptr` ([nl][nstar][NFRAMEFIT] float64) and `head_ptr` ([nl][NFRAMEFIT]
        float64) are raw device pointers (int) on this context's GPU; all batches are queued on the context stream
        without a host synchronisation.  A star whose shift plus the layer's offset leaves the domain is status 2 in
        that layer only."""
        nl = cube_fit_layers(nl)
        nstar = _frame_fit_device(ny, nx, nstar, npsf, psf_index_ptr, cube_ptr=cube_ptr, psf_ptr=psf_ptr,
                                  origin_ptr=origin_ptr, star_out_ptr=star_out_ptr, head_ptr=head_ptr)
        radius, flags, max_iter, tol = frame_fit_parameters(radius, background, max_iter, tol)
        layer_batch = cube_fit_batch(layer_batch)
        self._call_cube_fit(nl, ny, nx, cube_ptr, var_ptr, nstar, npsf, psf_ptr, psf_index_ptr, origin_ptr, shift_ptr,
                            layer_shift_ptr, scale0_ptr, radius, flags, max_iter, tol, layer_batch, star_out_ptr, head_ptr,
                            resid_ptr, 1)

    def _call_cube_free(self, nl, ny, nx, cube, var, nstar, npsf, psf, index, origin, shift, layer_shift, scale0, radius,
                        flags, max_iter, tol, free, rows, head, pos, shift_out, call, resid, on_device):
        p = _devptr if on_device else _vptr
        max_outer, pos_tol, max_step, max_move, min_snr = free
        _check(self.lib.mpsfr_fit_cube_psf_free(self._h, int(nl), int(ny), int(nx), p(cube), p(var), int(nstar),
                                                int(npsf), p(psf), p(index), p(origin), p(shift), p(layer_shift),
                                                p(scale0), float(radius), flags, int(max_iter), float(tol),
                                                int(max_outer), float(pos_tol), float(max_step), float(max_move),
                                                float(min_snr), p(rows), p(head), p(pos), p(shift_out), p(call),
                                                p(resid), on_device))

    def fit_cube_psf_free(self, cube, psf, origin, *, var=None, shift=None, layer_shift=None, psf_index=None,
                          scale0=None, radius=8.0, background=True, max_iter=100, tol=1e-10, max_outer=8, pos_tol=1e-3,
                          max_step=0.5, max_move=2.0, min_snr=3.0, return_residual=False):
        """Crowded-field photometry of a cube with free positions (mpsfr_fit_cube_psf_free): ONE shift per star from
        all layers of `cube` jointly -- fit_frame_psf_free's Gauss-Newton loop on the layers of fit_cube_psf, every
        layer with its own models psf[:, l] and its own offset layer_shift[l], all layers side by side on the GPU.
        The arrays are fit_cube_psf's (`shift` is the start), the outer loop's parameters fit_frame_psf_free's.  A
        layer carries a star when the star is accepted there with F > min_snr err_F; a star is free when some layer
        carries it; a layer with no accepted star or too few pixels is dead (head status 2) and the others are blind
        to it.  Returns (rows, pos, shifts, head, call) and, with return_residual, the residual cube at the final
        shifts.  rows (nl, n, NFRAMEFIT), head (nl, NFRAMEFIT): fit_cube_psf's columns of the closing solve (head 4 the
        closing solve's iterations, 5 the layer's own relative residual, 7: 2 for a dead layer, else the call's
        status).  pos (n, NCUBEFREE_POS): 0-1 the final shift, 2-3 its conditional errors, 4-5 final minus start, 6
        flags (FRAME_FREE_HELD, FRAME_FREE_BOUND, FRAME_FREE_CLIPPED), 7 the outer steps in which the star was free.
        shifts (n, 2): what fit_cube_psf takes as shift.  call (NCUBEFREE_CALL,): 0 chi2 summed, 1 its degrees of
        freedom, 2 outer steps, 3 the last largest step, 4 free stars in the last step, 5 inner iterations in all, 6
        status (0 positions and closing solve converged, 1 anything else fitted, 2 every layer dead), 7 the last
        joint relative residual.  All layers are resident: a call above CUBE_FREE_WORK_BYTES of work memory is
        refused (take the positions from fewer layers, the spectra from fit_cube_psf)."""
        cu, va, ps, ix, og, sh, ls, s0, radius, flags, max_iter, tol, free = cube_free_arguments(
            cube, var, psf, psf_index, origin, shift, layer_shift, scale0, radius, background, max_iter, tol, max_outer,
            pos_tol, max_step, max_move, min_snr, self.dimpsf)
        flag('return_residual', return_residual)
        nl, ny, nx = cu.shape
        n = og.shape[0]
        rows = np.empty((nl, n, NFRAMEFIT))
        head = np.empty((nl, NFRAMEFIT))
        pos = np.empty((n, NCUBEFREE_POS))
        shifts = np.empty((n, 2))
        call = np.empty(NCUBEFREE_CALL)
        resid = np.empty((nl, ny, nx)) if return_residual else None
        self._call_cube_free(nl, ny, nx, cu, va, n, ps.shape[0], ps, ix, og, sh, ls, s0, radius, flags, max_iter, tol,
                             free, rows, head, pos, shifts, call, resid, 0)
        return (rows, pos, shifts, head, call) + ((resid,) if return_residual else ())

    def fit_cube_psf_free_device(self, nl, ny, nx, cube_ptr, nstar, npsf, psf_ptr, origin_ptr, star_out_ptr, head_ptr,
                                 pos_ptr, shift_out_ptr, call_ptr, *, var_ptr=None, shift_ptr=None, layer_shift_ptr=None,
                                 psf_index_ptr=None, scale0_ptr=None, resid_ptr=None, radius=8.0, background=True,
                                 max_iter=100, tol=1e-10, max_outer=8, pos_tol=1e-3, max_step=0.5, max_move=2.0,
                                 min_snr=3.0):
        """Device-buffer form (asynchronous, on_device = 1) of fit_cube_psf_free: the pointers of fit_cube_psf_device,
        with `pos_ptr` ([nstar][NCUBEFREE_POS] float64), `shift_out_ptr` ([nstar][2] float64: what fit_cube_psf_device
        takes as shift_ptr) and `call_ptr` ([NCUBEFREE_CALL] float64).  The whole call -- every solve of every outer
        step, all layers -- is queued on the context stream without a host synchronisation."""
        nl = cube_fit_layers(nl)
        nstar = _frame_fit_device(ny, nx, nstar, npsf, psf_index_ptr, cube_ptr=cube_ptr, psf_ptr=psf_ptr,
                                  origin_ptr=origin_ptr, star_out_ptr=star_out_ptr, head_ptr=head_ptr, pos_ptr=pos_ptr,
                                  shift_out_ptr=shift_out_ptr, call_ptr=call_ptr)
        radius, flags, max_iter, tol = frame_fit_parameters(radius, background, max_iter, tol)
        free = frame_free_parameters(max_outer, pos_tol, max_step, max_move, min_snr)
        cube_free_work(nl, ny, nx, nstar)
        self._call_cube_free(nl, ny, nx, cube_ptr, var_ptr, nstar, npsf, psf_ptr, psf_index_ptr, origin_ptr, shift_ptr,
                             layer_shift_ptr, scale0_ptr, radius, flags, max_iter, tol, free, star_out_ptr, head_ptr,
                             pos_ptr, shift_out_ptr, call_ptr, resid_ptr, 1)

    def debug_fetch(self, what, shape):
        out = np.empty(int(np.prod(shape)))
        n = _check(self.lib.mpsfr_debug_fetch(self._h, what.encode(), _dptr(out), out.size))
        if n != out.size:
            raise ValueError('%s: library returned %d values, expected %d' % (what, n, out.size))
        return out.reshape(shape)

    def profile(self):
        """{kernel name: (total_ms, launches)} accumulated since the last profile_reset()."""
        res = {}
        for i in range(self.lib.mpsfr_profile_count()):
            ms, n = C.c_double(), C.c_long()
            _check(self.lib.mpsfr_profile_get(self._h, i, C.byref(ms), C.byref(n)))
            res[self.lib.mpsfr_profile_name(i).decode()] = (ms.value, n.value)
        return res

    def profile_names(self):
        """Kernel names in id order (the ids `profile_only` takes)."""
        return [self.lib.mpsfr_profile_name(i).decode()
                for i in range(self.lib.mpsfr_profile_count())]

    def profile_reset(self):
        _check(self.lib.mpsfr_profile_reset(self._h))


class PendingResult:
    """An asynchronous host-output call (Context.reconstruct_async): the arrays of `wait()` are filled
    by the library when the ticket is waited for."""

    def __init__(self, ctx, ticket, arrays):
        self.ctx, self.ticket, self._arrays, self._done = ctx, ticket, arrays, False

    def wait(self):
        if not self._done:
            if self.ticket in self.ctx._pending:         # (not abandoned, not completed by a sync)
                _check(self.ctx.lib.mpsfr_wait(self.ctx._h, self.ticket))
                self.ctx._handed_over(self.ticket)
            elif self.ticket in self.ctx._abandoned:
                raise MpsfrError(-1, 'ticket %d was abandoned (Context.abandon): its results were dropped' % self.ticket)
            self._done = True
        return self._arrays


class PendingMulti:
    """An asynchronous multi-context call (Context.reconstruct_multi_async)."""

    def __init__(self, ctxs, handles, arrays):
        self.ctxs, self._handles, self._arrays, self._done = list(ctxs), handles, arrays, False

    def wait(self):
        if not self._done:
            try:
                _check(self.ctxs[0].lib.mpsfr_wait_multi(self._handles, len(self.ctxs)))
            finally:
                for c in self.ctxs:
                    for t in [t for t in c._pending if isinstance(t, tuple) and c._pending[t] is self._arrays]:
                        del c._pending[t]
            self._done = True
        return self._arrays


class ContextPool:
    """Independent batches pipelined through several contexts (each has its own HIP stream and
    workspaces): `next()` hands out the contexts in turn, so that consecutive `reconstruct_device`
    calls run concurrently on the GPU -- the transforms of one batch overlap the fit of the one
    before (two contexts: +24 % PSFs/s on the bench workload).  Each batch needs its own output
    buffers until its context has been synchronised."""

    def __init__(self, n=2, **kwargs):
        self.contexts = [Context(**kwargs) for _ in range(max(1, int(n)))]
        self._i = 0

    def next(self):
        c = self.contexts[self._i % len(self.contexts)]
        self._i += 1
        return c

    def set_option(self, key, value):
        for c in self.contexts:
            c.set_option(key, value)

    def sync(self):
        for c in self.contexts:
            c.sync()

    def close(self):
        for c in self.contexts:
            c.close()
        self.contexts = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

