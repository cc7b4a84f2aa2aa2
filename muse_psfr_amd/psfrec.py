"""Drop-in Python API of the reference's PSF-reconstruction path, on the MI355X.

Mirrors ``muse_psfr.psfrec`` (reference psfrec.py) for this path: ``compute_psf`` (:933-978),
``compute_psf_from_sparta`` (:981-1120), ``create_sparta_table`` (:1123-1141), ``fit_psf_cube``
(:861-871), ``muse_intrinsic_psf`` (:1144-1171), ``fit_psf_with_polynom`` (:1174-1215) -- same names,
argument meaning, return structure, log messages and error behaviour.  All numerics run in
``libmpsfr.so`` (HIP); the reference's joblib fan-out over rows (:1082-1083) becomes one batched
GPU call.  There is no CPU fallback.

Extra keyword-only arguments (defaults = the reference's hard-coded values, so existing callers see
no difference): ``dim=1280`` (:955), ``dimpsf=40`` (:658), ``pixscale=0.2`` (:659, :899, :868),
``precision='mixed'|'f64'``, ``cutoff_masks='host'|'exact'|(rec, res)``, ``device=0``.

astropy is used for tables / FITS when it is importable (then the return types are astropy's, as
in the reference); otherwise the small NumPy implementations in ``_minifits`` / ``Table`` below.
"""
import functools
import logging
import os
from collections import OrderedDict

import numpy as np

from . import _args, _lib, _minifits
from ._lib import Context, MpsfrError, E_GRID

MIN_L0 = 8    # minimum L0 in m (psfrec.py:30)
MAX_L0 = 30   # maximum L0 in m (psfrec.py:31)

logger = logging.getLogger(__name__)

_FIT_COLS = ('lbda', 'center', 'flux', 'fwhm', 'n', 'peak', 'err_center', 'err_flux', 'err_fwhm',
             'err_n', 'err_peak')
# mpdaf's moffat_fit(circular=False) columns: fwhm / err_fwhm are (major, minor), rot / err_rot in degrees
_FIT_COLS_ELL = ('lbda', 'center', 'flux', 'fwhm', 'n', 'rot', 'peak', 'err_center', 'err_flux', 'err_fwhm', 'err_n',
                 'err_rot', 'err_peak')


_ASTROPY = []


def _astropy():
    """(astropy.io.fits, astropy.table.Table), or (None, None) without a working astropy.  The
    outcome is kept: a failed import costs 0.1 ms every time, a fifth of a one-row compute_psf."""
    if not _ASTROPY:
        try:
            from astropy.io import fits
            from astropy.table import Table as ATable
            _ASTROPY.append((fits, ATable))
        except Exception:  # noqa: BLE001 - absent or broken astropy: use the NumPy implementations
            _ASTROPY.append((None, None))
    return _ASTROPY[0]


class Table:
    """Tiny stand-in for astropy.table.Table (used only when astropy is absent): ordered columns
    of equal length plus a ``meta`` dict."""

    def __init__(self, columns=None, meta=None):
        self.columns = OrderedDict((k, np.asarray(v)) for k, v in (columns or {}).items())
        self.meta = dict(meta or {})

    @property
    def colnames(self):
        return list(self.columns)

    def __len__(self):
        return 0 if not self.columns else len(next(iter(self.columns.values())))

    def __getitem__(self, key):
        if isinstance(key, str):
            return self.columns[key]
        return Table(OrderedDict((k, v[key]) for k, v in self.columns.items()), self.meta)

    def __setitem__(self, key, value):
        n = len(self)
        v = np.asarray(value)
        self.columns[key] = np.full(n, v) if v.ndim == 0 else v

    def __contains__(self, key):
        return key in self.columns

    @classmethod
    def read(cls, hdu):
        d = hdu.data
        meta = {k: v for k, v in hdu.header.items()
                if k not in ('XTENSION', 'BITPIX', 'NAXIS', 'NAXIS1', 'NAXIS2', 'PCOUNT', 'GCOUNT',
                             'TFIELDS', 'EXTNAME') and not k.startswith(('TTYPE', 'TFORM', 'TDIM'))}
        return cls(OrderedDict((n, np.array(d[n])) for n in d.dtype.names), meta)


@functools.lru_cache(maxsize=1)
def host_cutoff_masks():
    """The cut-off masks of psfrec.py:257 (>=) and :435 (>) evaluated with this host's NumPy in
    exactly the reference's way: |f cos(arctan(fy/fx))| and |f sin(arctan(fy/fx))| against
    fc = 1.5.  On the |k| = 24 lines the outcome depends on last-bit libm rounding, so the
    reference itself is platform dependent there ("cut-off masks"); computing them here
    keeps a user's results identical to what the reference gives on the same machine."""
    fx = np.fft.fftfreq(80, 8.0 / 40)[:, np.newaxis]
    fy = fx.T
    f = np.sqrt(fx ** 2 + fy ** 2)
    with np.errstate(all='ignore'):
        arg = fy / fx
    arg[0, 0] = 0
    arg = np.arctan(arg)
    f_x = f * np.cos(arg)
    f_y = f * np.sin(arg)
    fc = 1 / (2 * (8.0 / 24.0))
    rec = (f != 0) & (np.abs(f_x) >= fc) | (np.abs(f_y) >= fc)
    res = (f != 0) & (np.abs(f_x) > fc) | (np.abs(f_y) > fc)
    return rec, res


_contexts = {}


def get_context(dim=1280, pixscale=0.2, dimpsf=40, precision='mixed', device=0, replica=0):
    """Cached GPU context for (dim, pixscale, dimpsf, precision, device); `replica` > 0: a further
    context on the same device (fan-out tests run two shards on one GPU)."""
    key = (int(dim), float(pixscale), int(dimpsf), precision, int(device), int(replica))
    if key not in _contexts:
        _contexts[key] = Context(dim=dim, pixscale=pixscale, dimpsf=dimpsf, precision=precision,
                                 device=device)
    return _contexts[key]


def _resolve_masks(cutoff_masks):
    if cutoff_masks is None or (isinstance(cutoff_masks, str) and cutoff_masks == 'exact'):
        return None
    if isinstance(cutoff_masks, str):
        if cutoff_masks != 'host':
            raise ValueError("cutoff_masks must be 'host', 'exact' or a (rec, res) pair")
        return host_cutoff_masks()
    return cutoff_masks


# Fan-out over several GPUs pays from this many tasks per device (a 100-row batch takes 0.3 ms)
FANOUT_MIN_TASKS_PER_DEVICE = 32


def _fanout_devices(devices, device, ntask, n_jobs):
    """The devices a batch of `ntask` tasks runs on.  An explicit list `devices` is taken as given
    (repeats allowed: several contexts on one GPU).  An explicit `device` is that device and nothing
    else.  Both left at None: every visible GPU when the batch is large enough and the caller did not
    ask for one job (n_jobs = 1; n_jobs > 1 caps the number of devices, like it caps the reference's
    worker processes, psfrec.py:1082) -- unless the process is one rank of a one-rank-per-GPU launch
    (WORLD_SIZE / LOCAL_RANK set, distributed.py): a rank stays on its own device, LOCAL_RANK."""
    if devices is not None:
        devs = [int(d) for d in devices]
        if not devs:
            raise ValueError('devices must not be empty')
        return devs
    if device is not None:
        return [int(device)]
    if 'WORLD_SIZE' in os.environ or 'LOCAL_RANK' in os.environ:
        return [int(os.environ.get('LOCAL_RANK', 0))]
    if n_jobs == 1:
        return [0]
    from ._lib import device_count
    n = device_count()
    if n_jobs is not None and n_jobs > 1:
        n = min(n, int(n_jobs))
    n = min(n, ntask // FANOUT_MIN_TASKS_PER_DEVICE)
    if n <= 1:
        return [0]
    return list(range(n))


def _reconstruct(lbda, tasks, npsflin, h, dim, dimpsf, pixscale, precision, cutoff_masks, device,
                 want_psf=True, devices=None, n_jobs=1):
    if isinstance(tasks, tuple) and len(tasks) == 2 and isinstance(tasks[0], np.ndarray):
        st, t3 = tasks                  # ([ntask][3] seeing / GL / L0, [ntask] three-laser mode)
        see, gl, l0 = (np.ascontiguousarray(st[:, k], dtype=float) for k in range(3))
        three = np.asarray(t3).astype(np.uint8)
    else:                               # list of (seeing, GL, L0, three_lgs_mode)
        see = np.array([t[0] for t in tasks], dtype=float)
        gl = np.array([t[1] for t in tasks], dtype=float)
        l0 = np.array([t[2] for t in tasks], dtype=float)
        three = np.array([1 if t[3] else 0 for t in tasks], dtype=np.uint8)
    masks = _resolve_masks(cutoff_masks)
    devs = _fanout_devices(devices, device, see.size, n_jobs)

    def run(dev, replica, a, b):
        ctx = get_context(dim, pixscale, dimpsf, precision, dev, replica)
        return ctx.reconstruct(lbda, see[a:b], gl[a:b], l0[a:b], three[a:b], h, npsflin=npsflin,
                               masks=masks, want_psf=want_psf)
    try:
        if len(devs) == 1:
            res = run(devs[0], 0, 0, see.size)
            res['devices'] = devs
            return res
        # Row shards over the devices, one context per device and one host thread each inside the
        # library (mpsfr_reconstruct_multi): the reference's joblib fan-out (psfrec.py:1082-1083).
        # Per-task results do not depend on the sharding; the stamp sums are added in device order.
        replica = [devs[:i].count(d) for i, d in enumerate(devs)]
        ctxs = [get_context(dim, pixscale, dimpsf, precision, d, r) for d, r in zip(devs, replica)]
        res = Context.reconstruct_multi(ctxs, lbda, see, gl, l0, three, h, npsflin=npsflin, masks=masks,
                                        want_psf=want_psf)
        res['devices'] = devs
        return res
    except MpsfrError as e:
        if e.code == E_GRID:
            # the reference fails here with a ValueError from scipy's interpn (psfrec.py:663-683)
            raise ValueError(str(e)) from None
        raise


PIPELINE_MIN_TASKS = 125      # a single-device table of at least twice as many tasks goes through asynchronous parts
PIPELINE_PARTS = 2            # one part per pipeline lane (with the FIT_ROWS columns written in C -- mpsfr_fit_rows --
                              # the parts' host work no longer pays for more: 1000 rows x 35 lambda at 512^2 take
                              # 2.41 / 2.49 / 2.62 / 2.64 ms in 2 / 3 / 4 / 5 parts)


def _reconstruct_pipelined(lbda, stats, three, laser_idx, npsflin, h, dim, dimpsf, pixscale, precision,
                           cutoff_masks, dev):
    """compute_psf_from_sparta's batch as asynchronous parts (PIPELINE_PARTS) on one context, the FIT_ROWS records of a
    part assembled while the next parts are on the GPU.  Returns (dict(psf_sum, devices, rec), records)."""
    ntask, nlam = len(stats), lbda.size
    nparts = max(2, min(PIPELINE_PARTS, ntask // PIPELINE_MIN_TASKS))
    bounds = [ntask * k // nparts for k in range(nparts + 1)]
    masks = _resolve_masks(cutoff_masks)
    ctx = get_context(dim, pixscale, dimpsf, precision, dev, 0)
    see, gl, l0 = (np.ascontiguousarray(stats[:, k], dtype=float) for k in range(3))
    t3 = np.asarray(three).astype(np.uint8)
    psum = None
    # Whatever goes wrong between the first asynchronous call and the last wait -- a library error in a
    # later part, a MemoryError in the template, a KeyboardInterrupt -- the parts already queued are
    # abandoned (the library drains and forgets their output arrays, which the context kept alive until
    # now): nothing is left behind that a later call on the cached context could write through.
    try:
        pend = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            pend.append(ctx.reconstruct_async(lbda, see[a:b], gl[a:b], l0[a:b], t3[a:b], h, npsflin=npsflin,
                                              masks=masks, want_psf=False))
        rec, blk = _fit_rows_template(lbda, stats, laser_idx)          # (while the GPU works)
        for (a, b), p in zip(zip(bounds[:-1], bounds[1:]), pend):
            r = p.wait()
            _fit_rows_fill(blk[a * nlam:b * nlam], r['fit'], pixscale)
            psum = r['psf_sum'] if psum is None else psum + r['psf_sum']
    except BaseException as e:
        ctx.abandon()
        if isinstance(e, MpsfrError) and e.code == E_GRID:
            raise ValueError(str(e)) from None
        raise
    return dict(psf_sum=psum, devices=[dev], rec=True), rec


def _fit_columns(lbda, fit, pixscale):
    """fit: (n, NFIT) rows of libmpsfr -> the columns fit_psf_cube keeps (psfrec.py:866-870)."""
    fit = np.asarray(fit)
    n = fit.shape[0]
    cols = OrderedDict()
    cols['lbda'] = np.asarray(lbda, dtype=float)
    cols['center'] = fit[:, 1:3].copy()
    cols['flux'] = fit[:, 15].copy()
    cols['fwhm'] = np.repeat(fit[:, 5:6] * pixscale, 2, axis=1)
    cols['n'] = fit[:, 4].copy()
    cols['peak'] = fit[:, 0].copy()
    cols['err_center'] = fit[:, 9:11].copy()
    with np.errstate(all='ignore'):
        rel = np.sqrt((fit[:, 8] / fit[:, 0]) ** 2 + (2 * fit[:, 11] / fit[:, 3]) ** 2 +
                      (fit[:, 12] / (fit[:, 4] - 1)) ** 2)
    cols['err_flux'] = np.abs(fit[:, 15]) * rel
    cols['err_fwhm'] = np.repeat(fit[:, 13:14] * pixscale, 2, axis=1)
    cols['err_n'] = fit[:, 12].copy()
    cols['err_peak'] = fit[:, 8].copy()
    assert tuple(cols) == _FIT_COLS and all(len(v) == n for v in cols.values())
    return cols


def _fit_columns_ell(lbda, fit, pixscale):
    """fit: (n, NFIT_ELL) elliptical fit rows of libmpsfr -> the columns of _FIT_COLS_ELL (fwhm in arcsec)."""
    fit = np.asarray(fit)
    n = fit.shape[0]
    cols = OrderedDict()
    cols['lbda'] = np.asarray(lbda, dtype=float)
    cols['center'] = fit[:, 1:3].copy()
    cols['flux'] = fit[:, 19].copy()
    cols['fwhm'] = fit[:, 7:9] * pixscale
    cols['n'] = fit[:, 5].copy()
    cols['rot'] = fit[:, 6].copy()
    cols['peak'] = fit[:, 0].copy()
    cols['err_center'] = fit[:, 12:14].copy()
    cols['err_flux'] = fit[:, 20].copy()
    cols['err_fwhm'] = fit[:, 14:16] * pixscale
    cols['err_n'] = fit[:, 17].copy()
    cols['err_rot'] = fit[:, 16].copy()
    cols['err_peak'] = fit[:, 11].copy()
    assert tuple(cols) == _FIT_COLS_ELL and all(len(v) == n for v in cols.values())
    return cols


def _check_circular(circular):
    return bool(_args.flag('circular', circular))


def _check_precision(precision):
    if precision not in ('mixed', 'f64'):
        raise ValueError("precision must be 'mixed' or 'f64'")


def _grid_or_field(npsflin, positions):
    """What a call with optional positions evaluates: None for the npsflin x npsflin grid, else the caller's positions,
    validated (any number of them)."""
    if positions is None:
        _args.grid_side(npsflin)
        return None
    return _lib.field_positions(positions, max_n=None)


def _two_layer_atmosphere(seeing, GL, L0, h):
    """(seeing, GL, L0) as floats of a call on the reference's two-layer atmosphere (ValueError)."""
    try:
        seeing, GL, L0 = float(seeing), float(GL), float(L0)
    except (TypeError, ValueError):
        raise ValueError('seeing, GL and L0 must be scalars') from None
    if not (seeing > 0 and L0 > 0 and 0 <= GL <= 1):
        raise ValueError('need seeing > 0, L0 > 0 and 0 <= GL <= 1')
    if np.asarray(h).size != 2:
        raise ValueError('exactly two layers are supported (psfrec.py:66)')
    return seeing, GL, L0


_FIT_ROWS_DTYPE = np.dtype([('lbda', 'f8'), ('center', 'f8', (2,)), ('flux', 'f8'), ('fwhm', 'f8', (2,)),
                            ('n', 'f8'), ('peak', 'f8'), ('err_center', 'f8', (2,)), ('err_flux', 'f8'),
                            ('err_fwhm', 'f8', (2,)), ('err_n', 'f8'), ('err_peak', 'f8'), ('SEEING', 'f8'),
                            ('GL', 'f8'), ('L0', 'f8'), ('row_idx', 'i8'), ('lgs_idx', 'i8')])


def _fit_rows_template(lbda, stats, laser_idx):
    """The FIT_ROWS table of compute_psf_from_sparta (psfrec.py:1086-1101) as one structured array with the
    columns that only depend on the inputs filled in (lbda, SEEING, GL, L0, row_idx, lgs_idx) -- work for
    the time the GPU is busy.  Returns (records, their (n, 20) float64 view)."""
    ntask, nlam = len(stats), len(lbda)
    assert _FIT_ROWS_DTYPE.itemsize == 160 and _FIT_ROWS_DTYPE.names[:11] == _FIT_COLS
    blk = np.empty((ntask * nlam, 20))
    # record layout: 0 lbda, 1-2 center, 3 flux, 4-5 fwhm, 6 n, 7 peak, 8-9 err_center, 10 err_flux,
    # 11-12 err_fwhm, 13 err_n, 14 err_peak, 15 SEEING, 16 GL, 17 L0, 18 row_idx, 19 lgs_idx
    b3 = blk.reshape(ntask, nlam, 20)
    b3[:, :, 0] = np.asarray(lbda, dtype=float)[None, :]
    b3[:, :, 15:18] = np.asarray(stats, dtype=float)[:, None, :]
    ib = blk.view(np.int64).reshape(ntask, nlam, 20)
    ib[:, :, 18] = np.arange(1, ntask + 1)[:, None]
    ib[:, :, 19] = np.asarray(laser_idx, dtype=np.int64)[:, None]
    return blk.view(_FIT_ROWS_DTYPE).reshape(ntask * nlam), blk


def _fit_rows_fill(blk, fit, pixscale):
    """The fit columns of FIT_ROWS (the values of _fit_columns) into the rows `blk` ((n, 20) view of the
    records) from the library's fit rows `fit` (.., NFIT): one pass in C (mpsfr_fit_rows), straight into the
    records -- the NumPy form (a row-wise gather + six strided column operations) took 0.28 ms per 8750 rows,
    a third of the host's critical path behind the last part of a large table."""
    _lib.fit_rows(fit, pixscale, blk[:, 1:15])


def _fit_rows_records(lbda, fit, pixscale, stats, laser_idx):
    """FIT_ROWS from the fit rows of all tasks, (ntask, nl, NFIT)."""
    rec, blk = _fit_rows_template(lbda, stats, laser_idx)
    _fit_rows_fill(blk, fit, pixscale)
    return rec


def _make_table(cols, meta=None):
    _, ATable = _astropy()
    if ATable is not None:
        t = ATable(cols)
        t.meta.update(meta or {})
        return t
    return Table(cols, meta)


_FIT_COLS_OBS = ('back', 'err_back', 'npix')


def _fit_columns_obs(lbda, fit, pixscale, circular):
    """fit: (n, NFIT_ELL) rows of the weighted fit -> the columns of _FIT_COLS (circular) or _FIT_COLS_ELL, then
    back, err_back, npix."""
    fit = np.asarray(fit)
    cols = _fit_columns_ell(lbda, fit, pixscale)
    if circular:
        cols = OrderedDict((k, cols[k]) for k in _FIT_COLS)
    cols['back'] = fit[:, 21].copy()
    cols['err_back'] = fit[:, 22].copy()
    cols['npix'] = fit[:, 23].astype(np.int64)
    return cols


def _observed_cube(cube, var):
    """(data, var) of the observed path of fit_psf_cube.  `cube`: an array, a masked array, or an mpdaf-style object
    with .data (masked pixels become NaN) and .var; `var`: None (unit weights), an array of the cube's shape, or True
    for the object's own .var."""
    own_var = None
    if isinstance(cube, np.ndarray):              # plain or masked array (observed_stamps turns masked into NaN)
        data = cube
    elif hasattr(cube, 'data'):                   # an mpdaf-style object
        data, own_var = cube.data, getattr(cube, 'var', None)
        mask = getattr(cube, 'mask', None)
        if mask is not None and mask is not np.ma.nomask and not isinstance(data, np.ma.MaskedArray):
            data = np.ma.MaskedArray(data, mask=mask)
    else:
        data = cube
    if var is True:
        var = own_var
        if var is None:
            raise ValueError('var=True needs a cube with a .var plane')
    elif var is False:
        var = None
    return _lib.observed_stamps(data, var)


def fit_psf_cube(lbda, psfcube, *, circular=True, var=None, fit_back=False, pixscale=0.2, precision='mixed',
                 device=0):
    """Fit a Moffat PSF on each wavelength plane of the psfcube (psfrec.py:861-871).

    circular=False: an elliptical Moffat (mpdaf's moffat_fit(circular=False)); the table has the columns of
    _FIT_COLS_ELL, with fwhm / err_fwhm as (major, minor) in arcsec and rot / err_rot in degrees (major axis from
    the column axis towards the row axis, in [0, 180)).

    var / fit_back: the weighted fit of observed stars (mpdaf's moffat_fit(weight=True, fit_back=...)), taken when
    `var` is given or fit_back is True.  var: the variance of every pixel (an array of the cube's shape), or True for
    the .var of an mpdaf-style cube; NaN or masked pixels and pixels whose variance is not finite and > 0 are left
    out.  The table then has the columns of the circular / elliptical fit plus back, err_back and npix (the number
    of pixels used)."""
    circular = _check_circular(circular)
    _args.flag('fit_back', fit_back)
    if var is not None or fit_back:
        data, va = _observed_cube(psfcube, var)
        if np.size(lbda) != data.shape[0]:
            raise ValueError('need one wavelength per plane of psfcube')
        ctx = get_context(128, pixscale, data.shape[-1], precision, device)
        fit = ctx.fit_stamps_observed(data, va, background=bool(fit_back), circular=circular)
        return _make_table(_fit_columns_obs(lbda, fit, pixscale, circular))
    if not circular:
        data = _lib.elliptical_stamps(psfcube)
        if np.size(lbda) != data.shape[0]:
            raise ValueError('need one wavelength per plane of psfcube')
        ctx = get_context(128, pixscale, data.shape[-1], precision, device)
        return _make_table(_fit_columns_ell(lbda, ctx.fit_stamps_elliptical(data), pixscale))
    data = np.asarray(getattr(psfcube, 'data', psfcube), dtype=float)
    ctx = get_context(128, pixscale, data.shape[-1], precision, device)
    return _make_table(_fit_columns(lbda, ctx.fit_stamps(data), pixscale))


_FIT_COLS_PSF = ('scale', 'shift', 'back', 'flux', 'chi2', 'npix', 'status', 'err_scale', 'err_shift', 'err_back',
                 'err_flux')


def _fit_columns_psf(fit, pixscale):
    """fit: (n, NFIT_PSF) rows of the PSF-model fit -> the columns of _FIT_COLS_PSF (shift in arcsec)."""
    fit = np.asarray(fit)
    cols = OrderedDict()
    cols['scale'] = fit[:, 0].copy()
    cols['shift'] = fit[:, 1:3] * pixscale
    cols['back'] = fit[:, 3].copy()
    cols['flux'] = fit[:, 12].copy()
    cols['chi2'] = fit[:, 4].copy()
    cols['npix'] = fit[:, 11].astype(np.int64)
    cols['status'] = fit[:, 10].astype(np.int64)
    cols['err_scale'] = fit[:, 6].copy()
    cols['err_shift'] = fit[:, 7:9] * pixscale
    cols['err_back'] = fit[:, 9].copy()
    cols['err_flux'] = fit[:, 13].copy()
    assert tuple(cols) == _FIT_COLS_PSF
    return cols


def fit_stars_with_psf(stars, psf, *, var=None, psf_index=None, shift=None, fit_back=True, fixed_shift=False,
                       pixscale=0.2, precision='mixed', device=0):
    """PSF-fitting photometry: fit the model stamps `psf` (..., 40, 40) -- e.g. reconstructed PSFs -- to the observed
    stars `stars`, each in a flux scale, a sub-pixel shift and (fit_back) a constant background.  The model is resampled
    by cubic convolution and counts as zero outside its stamp.

    stars / var: what fit_psf_cube(var=...) accepts (an array, a masked array or an mpdaf-style object; var an array,
    True for the object's own .var, or None for unit weights).  psf_index: the model stamp of every star, or None for
    one model stamp per star in order.  shift: (n, 2) start values of the shift (row, column) in arcsec, or None for
    the difference of the brightest pixels; fixed_shift=True holds them (the problem is then linear).

    Returns a table with one row per star: scale (F), shift (2, arcsec), back, flux = F sum(psf), chi2 (the weighted
    sum of squares: the goodness of the reconstruction on this star), npix (pixels used), status (0 a minimum, 1 not
    converged or against the 8-pixel bound of the shift, 2 not fitted), err_scale, err_shift (2, arcsec), err_back,
    err_flux (errors scaled by sqrt(chi2 / dof))."""
    _args.flag('fit_back', fit_back)
    _args.flag('fixed_shift', fixed_shift)
    _pixscale(pixscale)
    data, va = _observed_cube(stars, var)
    sh = _shift_pixels(shift, pixscale)
    ctx = get_context(128, pixscale, data.shape[-1], precision, device)
    fit = ctx.fit_stamps_psf(data, psf, var=va, psf_index=psf_index, shift=sh, background=bool(fit_back),
                             fixed_shift=bool(fixed_shift))
    return _make_table(_fit_columns_psf(fit, pixscale))


_FIT_COLS_SPEC = ('shift', 'err_shift', 'drift', 'err_drift', 'chi2', 'npix', 'nlayers', 'status', 'flux', 'err_flux',
                  'scale', 'back', 'layer_status', 'lbda')


def _fit_columns_spec(head, layers, lbda, pixscale):
    """head (n, NFIT_SPEC), layers (n, nl, NFIT_SPEC_LAYER) of the fit of star cubes -> the columns of _FIT_COLS_SPEC
    (position and drift in arcsec; the drift over half the wavelength range)."""
    head, layers = np.asarray(head), np.asarray(layers)
    cols = OrderedDict()
    cols['shift'] = head[:, 0:2] * pixscale
    cols['err_shift'] = head[:, 4:6] * pixscale
    cols['drift'] = head[:, 2:4] * pixscale
    cols['err_drift'] = head[:, 6:8] * pixscale
    cols['chi2'] = head[:, 8].copy()
    cols['npix'] = head[:, 11].astype(np.int64)
    cols['nlayers'] = head[:, 12].astype(np.int64)
    cols['status'] = head[:, 10].astype(np.int64)
    cols['flux'] = layers[:, :, 4].copy()
    cols['err_flux'] = layers[:, :, 5].copy()
    cols['scale'] = layers[:, :, 0].copy()
    cols['back'] = layers[:, :, 1].copy()
    cols['layer_status'] = layers[:, :, 8].astype(np.int64)
    cols['lbda'] = np.broadcast_to(np.asarray(lbda, dtype=float), layers.shape[:2]).copy()
    assert tuple(cols) == _FIT_COLS_SPEC
    return cols


def fit_star_spectra_with_psf(cubes, psf, lbda, *, var=None, psf_index=None, shift=None, fit_back=True, drift=False,
                              pixscale=0.2, precision='mixed', device=0):
    """Spectra of stars from a data cube by PSF fitting: every star is a cube (n, nl, 40, 40) of its images at the nl
    wavelengths `lbda`, and `psf` (npsf, nl, 40, 40) holds the model -- e.g. reconstructed PSFs -- of every wavelength.
    All layers of a star share one position; each has a flux scale and (fit_back) a constant background.  drift=True
    lets the position move linearly with wavelength: shift + drift x, x = (lbda - mid) / half-range in [-1, 1].  A
    layer without enough valid pixels (a masked sky line) is left out and the others are fitted without it.

    var: the variances (the cubes' shape) or None; NaN pixels and invalid variances are masked.  psf_index: the model
    cube of every star, or None for one per star in order.  shift: (n, 2) start position (row, column) in arcsec, or
    None for the difference of the brightest pixels of the collapsed images, which only serves stars that stand above
    the noise there: start faint stars from a catalogue position.

    Returns a table with one row per star: shift, err_shift, drift, err_drift (2, arcsec), chi2, npix, nlayers (the
    layers fitted), status (0 a minimum, 1 not converged or against the 8-pixel bound, 2 not fitted) and the (n, nl)
    columns flux = scale sum(psf_l), err_flux, scale, back, layer_status (2: left out) and lbda.  The errors are those
    of the joint fit, scaled by sqrt(chi2 / dof)."""
    _args.flag('fit_back', fit_back)
    _args.flag('drift', drift)
    _pixscale(pixscale)
    lb = _args.array('lbda', lbda).ravel()
    if lb.size < 1 or not np.all(np.isfinite(lb)):
        raise ValueError('lbda must hold one finite wavelength per layer')
    if np.ndim(cubes) not in (3, 4) or np.shape(cubes)[-3] != lb.size:
        raise ValueError('cubes must have the shape (n, %d, 40, 40): one layer per wavelength' % lb.size)
    x = None
    if drift:
        lo, hi = lb.min(), lb.max()
        if not hi > lo:
            raise ValueError('drift=True needs at least two different wavelengths')
        x = np.clip((lb - 0.5 * (lo + hi)) / (0.5 * (hi - lo)), -1.0, 1.0)
    sh = _shift_pixels(shift, pixscale)
    ctx = get_context(128, pixscale, np.shape(cubes)[-1], precision, device)
    head, layers = ctx.fit_spectra_psf(cubes, psf, var=var, psf_index=psf_index, shift=sh, background=bool(fit_back), x=x)
    return _make_table(_fit_columns_spec(head, layers, lb, pixscale))


_FIT_COLS_GROUP = ('group', 'source', 'scale', 'shift', 'flux', 'err_scale', 'err_shift', 'err_flux', 'back', 'err_back',
                   'chi2', 'npix', 'status', 'max_corr')
_GROUP_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))      # fit_out[40 .. 45] of mpsfr_fit_groups_psf


def _group_positions(positions, n, pixscale):
    """The `positions` argument of fit_star_groups_with_psf -> a list of n arrays (n_k, 2) in pixels, n_k = 1 ..
    MAX_GROUP, finite and inside the domain of the fit (ValueError)."""
    try:
        arr = np.asarray(positions, dtype=float)
    except (TypeError, ValueError):
        arr = None
    if arr is not None and arr.ndim == 3:
        if arr.shape[0] != n or arr.shape[2] != 2:
            raise ValueError('positions must have the shape (%d, K, 2)' % n)
        nan = np.isnan(arr).all(axis=2)
        groups = [g[~m] for g, m in zip(arr, nan)]
    else:
        try:
            groups = [np.asarray(g, dtype=float).reshape(-1, 2) for g in positions]
        except (TypeError, ValueError):
            raise ValueError('positions must be an (n, K, 2) array or one (n_k, 2) array per stamp') from None
        if len(groups) != n:
            raise ValueError('positions must hold one entry per stamp (%d), got %d' % (n, len(groups)))
    out = []
    for g in groups:
        if not 1 <= len(g) <= _lib.MAX_GROUP:
            raise ValueError('a stamp holds 1 to %d sources, not %d' % (_lib.MAX_GROUP, len(g)))
        px = g / pixscale
        if not np.all(np.abs(px) <= _lib.FIT_PSF_MAX_SHIFT):          # (NaN fails)
            raise ValueError('the positions must be finite and within %g pixels of the stamp centre'
                             % _lib.FIT_PSF_MAX_SHIFT)
        out.append(px)
    return out


def fit_star_groups_with_psf(stars, psf, positions, *, var=None, psf_index=None, fit_back=True, mode='free',
                             pixscale=0.2, precision='mixed', device=0):
    """PSF-fitting photometry of blended stars: every stamp of `stars` holds one to four stars of its model stamp `psf`
    (..., 40, 40), which are fitted at once -- each in a flux scale, the positions according to `mode`, and (fit_back)
    one constant background per stamp.

    positions: where the stars of each stamp are, (row, column) in arcsec from the model stamp's own position: a
    sequence with one (n_k, 2) array per stamp, or an (n, K, 2) array whose all-NaN rows mean "no such source".
    mode: 'free' (every position is fitted from the given start), 'common' (the relative positions are held and one
    offset of the whole group is fitted: catalogue positions) or 'fixed' (positions held; the problem is linear).
    stars / var / psf_index: as fit_stars_with_psf.  The stamps are bucketed by their number of stars and fitted with
    one library call per size; a single star goes to the PSF-model fit of fit_stars_with_psf ('common' is then a
    free shift).  No star may be farther than 8 pixels from the stamp centre.

    Returns a table with one row per star, in input order: group (the stamp), source (its number in the stamp), scale
    (F), shift (2, arcsec), flux = F sum(psf), err_scale, err_shift (2, arcsec), err_flux, then the group's back,
    err_back, chi2, npix and status (as fit_stars_with_psf) repeated on each of its rows, and max_corr: the largest
    |correlation coefficient| of this star's F with that of another star of the stamp (0 for a single star) -- how
    blended its flux is."""
    _args.flag('fit_back', fit_back)
    if not (np.isfinite(pixscale) and pixscale > 0):
        raise ValueError('pixscale must be positive')
    _lib.group_fit_flags(bool(fit_back), mode)
    data, va = _observed_cube(stars, var)
    n = data.shape[0]
    ps, ix, _, _ = _lib.psf_fit_arguments(n, psf, psf_index, None, True, False, data.shape[-1])
    ix = np.arange(n, dtype=np.int32) if ix is None else ix
    groups = _group_positions(positions, n, pixscale)
    sizes = np.array([len(g) for g in groups])
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])           # the first table row of each stamp
    nrow = int(sizes.sum())
    cols = OrderedDict()
    cols['group'] = np.repeat(np.arange(n), sizes)
    cols['source'] = np.concatenate([np.arange(k) for k in sizes])
    for name in _FIT_COLS_GROUP[2:]:
        wide = name in ('shift', 'err_shift')
        cols[name] = np.zeros((nrow, 2) if wide else nrow, dtype=np.int64 if name in ('npix', 'status') else float)
    ctx = get_context(128, pixscale, data.shape[-1], precision, device)
    for K in np.unique(sizes):
        idx = np.flatnonzero(sizes == K)
        sh = np.array([groups[i] for i in idx])                    # (m, K, 2), pixels
        sub_var = None if va is None else va[idx]
        if K == 1:
            fit = ctx.fit_stamps_psf(data[idx], ps, var=sub_var, psf_index=ix[idx], shift=sh[:, 0], background=bool(fit_back),
                                     fixed_shift=mode == 'fixed')
            head = fit[:, [3, 9, 4, 11, 10]]
            src = fit[:, None, [0, 1, 2, 6, 7, 8, 12, 13]]
            corr = np.zeros((len(idx), 1))
        else:
            fit = ctx.fit_groups_psf(data[idx], ps, sh, var=sub_var, psf_index=ix[idx], background=bool(fit_back), mode=mode)
            head = fit[:, [0, 1, 2, 5, 4]]
            src = fit[:, 8:8 + 8 * K].reshape(len(idx), K, 8)
            cm = np.zeros((len(idx), _lib.MAX_GROUP, _lib.MAX_GROUP))
            for c, (i, j) in enumerate(_GROUP_PAIRS):
                cm[:, i, j] = cm[:, j, i] = np.abs(fit[:, 40 + c])
            corr = cm.max(axis=2)[:, :K]
        rows = (first[idx][:, None] + np.arange(K)[None, :]).ravel()
        flat = src.reshape(-1, 8)
        cols['scale'][rows] = flat[:, 0]
        cols['shift'][rows] = flat[:, 1:3] * pixscale
        cols['flux'][rows] = flat[:, 6]
        cols['err_scale'][rows] = flat[:, 3]
        cols['err_shift'][rows] = flat[:, 4:6] * pixscale
        cols['err_flux'][rows] = flat[:, 7]
        for c, name in enumerate(('back', 'err_back', 'chi2', 'npix', 'status')):
            cols[name][rows] = np.repeat(head[:, c], K)
        cols['max_corr'][rows] = corr.ravel()
    assert tuple(cols) == _FIT_COLS_GROUP
    return _make_table(cols)


def _pixscale(pixscale):
    if not (np.isfinite(pixscale) and pixscale > 0):
        raise ValueError('pixscale must be positive')


def _sharp_bounds(sharp):
    try:
        lo, hi = sharp
        lo, hi = (None if v is None else float(v) for v in (lo, hi))
    except (TypeError, ValueError):
        raise ValueError('sharp must be (lower, upper), each a number or None') from None
    if any(v is not None and np.isnan(v) for v in (lo, hi)):
        raise ValueError('sharp bounds must not be NaN')
    return lo, hi


def find_stars(image, psf, var=None, *, threshold=5.0, half=3, sep=None, sharp=(None, None), max_stars=4096,
               pixscale=0.2, precision='mixed', device=0):
    """The stars of a frame, on the GPU: the matched filter of `image` (ny, nx) with the (2 half + 1)^2 core of the
    model stamp `psf` (40, 40) -- e.g. a reconstructed PSF -- beside a free local background, and the peaks of its
    statistic at or above `threshold` that dominate the (2 sep + 1)^2 square around them (sep=None: half).  With the
    variance frame `var` the statistic is the significance of the amplitude in sigma; without, the amplitude itself.
    NaN pixels and var <= 0 are masked.  sharp = (lower, upper): keep only the rows whose sharpness lies within the
    bounds (None: open) -- 1 is the model itself, a cosmic ray lies far above, a galaxy below.  More peaks than
    max_stars cost a second call.

    Returns a table, brightest statistic first (ties in pixel order): position (2, pixels: row, column), origin (2,
    int32: what cut_stamps, render_star_field and subtract_stars take), statistic, scale (the amplitude: the start of
    the fit's F), back, sharp, npix (valid pixels of the window), flags (1, 2: no parabola along rows, columns; 4: no
    sharpness) and shift (2, arcsec): the start value fit_stars_with_psf(shift=...) takes for stamps cut at origin."""
    _pixscale(pixscale)
    lo, hi = _sharp_bounds(sharp)
    sep = half if sep is None else sep
    ctx = get_context(128, pixscale, np.shape(psf)[-1] if np.ndim(psf) >= 2 else 40, precision, device)
    rows, origin, nfound = ctx.find_stars(image, psf, var=var, half=half, sep=sep, threshold=threshold,
                                          max_stars=max_stars)
    if nfound > rows.shape[0]:
        rows, origin, nfound = ctx.find_stars(image, psf, var=var, half=half, sep=sep, threshold=threshold,
                                              max_stars=nfound)
    with np.errstate(invalid='ignore'):
        keep = np.ones(rows.shape[0], dtype=bool)
        if lo is not None:
            keep &= rows[:, 5] >= lo
        if hi is not None:
            keep &= rows[:, 5] <= hi
    rows, origin = rows[keep], origin[keep]
    order = np.argsort(-rows[:, 2], kind='stable')
    rows, origin = rows[order], origin[order]
    cols = OrderedDict()
    cols['position'] = rows[:, 0:2].copy()
    cols['origin'] = origin.astype(np.int32)
    cols['statistic'] = rows[:, 2].copy()
    cols['scale'] = rows[:, 3].copy()
    cols['back'] = rows[:, 4].copy()
    cols['sharp'] = rows[:, 5].copy()
    cols['npix'] = rows[:, 6].astype(np.int64)
    cols['flags'] = rows[:, 7].astype(np.int64)
    cols['shift'] = (rows[:, 0:2] - (origin + ctx.dimpsf // 2)) * pixscale
    return _make_table(cols)


def _star_positions(positions):
    """(n, 2) float64 (row, column) in pixels from an (n, 2) array or a find_stars table (its `position` column)."""
    try:
        pos = positions['position']
    except (KeyError, IndexError, TypeError, ValueError):
        pos = positions
    try:
        pos = np.asarray(pos, dtype=float)
    except (TypeError, ValueError):
        raise ValueError('positions must be a numeric array or a find_stars table') from None
    if pos.ndim != 2 or pos.shape[1] != 2 or pos.shape[0] < 1:
        raise ValueError('positions must have the shape (n, 2)')
    return np.ascontiguousarray(pos)


def _group_all(ctx, pos, crit, shape):
    """ctx.group_stars with room for every group; also the row of every star's group in the tables (-1: a filler)."""
    label, groups, origin, shift, counts = ctx.group_stars(pos, crit, shape)
    row = np.full(pos.shape[0], -1, dtype=np.int64)
    row[groups[:, 2]] = np.arange(groups.shape[0])
    star_row = np.where(label >= 0, row[np.maximum(label, 0)], -1)
    return label, groups, origin, shift, counts, star_row


def group_stars(positions, crit, shape=None, *, pixscale=0.2, precision='mixed', device=0):
    """Friends-of-friends groups of stars, on the GPU (DAOPHOT's GROUP): stars closer than `crit` pixels (at most 16)
    are linked, and a group is a connected component -- the stars that have to be fitted together.  `positions`: an
    (n, 2) array of (row, column) in pixels, or a find_stars table; rows with a NaN belong to no group.  `shape`:
    (ny, nx) of the frame, in which the positions lie within [-1, ny] x [-1, nx]; None: the smallest frame that
    holds them.

    Returns (stars, groups).  stars, one row per position in input order: label (the smallest index of the star's
    group, -1 for a NaN row), size (members of its group) and flags (those of its group).  groups, ordered by size
    (1, 2, 3, 4 members, then larger ones) and by label within a size: label, size, members (4; the indices in
    ascending order, -1 beyond the group, the four smallest of a larger group), origin (2, int32: the stamp
    cut_star_stamps-like calls take, centred on the group), shift (4, 2, pixels: every member from the centre pixel of
    that stamp) and flags (1: more than four members, no origin -- group again with a smaller crit; 2: a member lies
    more than 8 pixels from the stamp's centre, beyond the domain of the fits)."""
    _pixscale(pixscale)
    pos = _star_positions(positions)
    if shape is None:
        finite = pos[np.all(np.isfinite(pos), axis=1)]
        shape = (1, 1) if finite.size == 0 else tuple(int(max(1, np.ceil(v))) for v in finite.max(axis=0))
    ctx = get_context(128, pixscale, 40, precision, device)
    label, groups, origin, shift, counts, star_row = _group_all(ctx, pos, crit, shape)
    stars = OrderedDict()
    stars['label'] = label.astype(np.int64)
    stars['size'] = np.where(star_row >= 0, groups[np.maximum(star_row, 0), 0], 0).astype(np.int64)
    stars['flags'] = np.where(star_row >= 0, groups[np.maximum(star_row, 0), 1], 0).astype(np.int64)
    cols = OrderedDict()
    cols['label'] = groups[:, 2].astype(np.int64)
    cols['size'] = groups[:, 0].astype(np.int64)
    cols['members'] = groups[:, 4:8].astype(np.int64)
    cols['origin'] = origin.astype(np.int32)
    cols['shift'] = shift.copy()
    cols['flags'] = groups[:, 1].astype(np.int64)
    return _make_table(stars), _make_table(cols, {'counts': [int(c) for c in counts]})


_FIT_COLS_FOUND = _FIT_COLS_GROUP + ('nsrc', 'label', 'crowded')


def fit_found_stars(image, psf, found, *, var=None, crit, fit_back=True, mode='free', crowded='skip', radius=8.0,
                    pixscale=0.2, precision='mixed', device=0):
    """PSF-fitting photometry of the stars found in a frame, singles and blends alike, on the GPU: the stars `found` (a
    find_stars table or an (n, 2) array of (row, column) in pixels) are grouped by friends of friends at the critical
    separation `crit` (pixels, at most 16); one stamp per group is cut out of `image` (`var`: its variance frame or
    None), centred on the group, and the model stamp `psf` (40, 40) is fitted to all stars of a group at once -- a
    single star as fit_stars_with_psf does, two to four as fit_star_groups_with_psf does (fit_back, mode: as there),
    with one cut and one fit call per group size that occurs.

    Returns (fit, origin) in the form subtract_stars takes (with psf_index = zeros for the one model): `origin`
    (ngroup, 2) int32 holds the stamp origin of every group, and `fit` has one row per star in input order with the
    columns of fit_star_groups_with_psf -- `group` indexes `origin`, `source` numbers the star within its group -- plus
    nsrc (stars in its group), label (the smallest star index of its group) and crowded: True for the stars of a group
    of more than four or of one wider than the fit's domain (a member farther than 8 pixels from the stamp centre).
    With crowded='skip' those are not fitted: their rows carry status 2 and NaN.  With crowded='frame' the fitted
    singles and blends are subtracted from the frame and the crowded stars are solved together on that residual, as
    fit_crowded_stars does, at their found positions within `radius` pixels and with fit_back as given: their rows get
    scale, flux and the conditional errors (err_scale, err_flux), the shift from their own stamp origin with error 0,
    the back, err_back, chi2 and npix of the frame solve and max_corr NaN; `origin` gains one row per such star and
    their `group` column points at it, so that subtract_stars(image, psf, origin, fit) removes every star.  With
    crowded='free' the same, with the positions of the crowded stars refined beside their fluxes as
    refine_crowded_stars does (its defaults): their rows get the refined shift and its conditional error."""
    _args.flag('fit_back', fit_back)
    if crowded not in ('skip', 'frame', 'free'):
        raise ValueError("crowded must be 'skip', 'frame' or 'free'")
    _lib.frame_fit_parameters(radius, bool(fit_back), 1, 0.5)
    _pixscale(pixscale)
    _lib.group_fit_flags(bool(fit_back), mode)
    pos = _star_positions(found)
    if not np.all(np.isfinite(pos)):
        raise ValueError('the positions of the stars must be finite')
    im, va = _lib.frame_images(image, var)
    ps = np.ascontiguousarray(_args.array('psf', psf))
    if ps.ndim != 2 or ps.shape[0] != ps.shape[1]:
        raise ValueError('psf must be one model stamp (40, 40)')
    ctx = get_context(128, pixscale, ps.shape[-1], precision, device)
    label, groups, origin, shift, counts, star_row = _group_all(ctx, pos, crit, im.shape)
    nstar = pos.shape[0]
    order = np.lexsort((np.arange(nstar), label))                  # the stars of a group together, ascending
    first = np.concatenate([[True], label[order][1:] != label[order][:-1]])
    start = np.maximum.accumulate(np.where(first, np.arange(nstar), 0))
    source = np.empty(nstar, dtype=np.int64)
    source[order] = np.arange(nstar) - start
    cols = OrderedDict()
    cols['group'] = star_row.copy()
    cols['source'] = source
    for name in _FIT_COLS_GROUP[2:]:
        wide = name in ('shift', 'err_shift')
        if name in ('npix', 'status'):
            cols[name] = np.full(nstar, 2 if name == 'status' else 0, dtype=np.int64)
        else:
            cols[name] = np.full((nstar, 2) if wide else nstar, np.nan)
    off = _lib.group_offsets(counts)
    for K in range(1, _lib.MAX_GROUP + 1):
        idx = np.arange(off[K - 1], off[K])
        idx = idx[(groups[idx, 1] & _lib.GROUP_WIDE) == 0]
        if idx.size == 0:
            continue
        res = ctx.cut_stamps(im, origin[idx], var=va)
        stamps, sub_var = (res, None) if va is None else res
        zeros = np.zeros(idx.size, dtype=np.int32)
        if K == 1:
            fit = ctx.fit_stamps_psf(stamps, ps[None], var=sub_var, psf_index=zeros, shift=shift[idx, 0],
                                     background=bool(fit_back), fixed_shift=mode == 'fixed')
            head = fit[:, [3, 9, 4, 11, 10]]
            src = fit[:, None, [0, 1, 2, 6, 7, 8, 12, 13]]
            corr = np.zeros((idx.size, 1))
        else:
            fit = ctx.fit_groups_psf(stamps, ps[None], shift[idx, :K], var=sub_var, psf_index=zeros,
                                     background=bool(fit_back), mode=mode)
            head = fit[:, [0, 1, 2, 5, 4]]
            src = fit[:, 8:8 + 8 * K].reshape(idx.size, K, 8)
            cm = np.zeros((idx.size, _lib.MAX_GROUP, _lib.MAX_GROUP))
            for c, (i, j) in enumerate(_GROUP_PAIRS):
                cm[:, i, j] = cm[:, j, i] = np.abs(fit[:, 40 + c])
            corr = cm.max(axis=2)[:, :K]
        rows = groups[idx, 4:4 + K].astype(np.int64).ravel()       # the stars themselves: input order
        flat = src.reshape(-1, 8)
        cols['scale'][rows] = flat[:, 0]
        cols['shift'][rows] = flat[:, 1:3] * pixscale
        cols['flux'][rows] = flat[:, 6]
        cols['err_scale'][rows] = flat[:, 3]
        cols['err_shift'][rows] = flat[:, 4:6] * pixscale
        cols['err_flux'][rows] = flat[:, 7]
        for c, name in enumerate(('back', 'err_back', 'chi2', 'npix', 'status')):
            cols[name][rows] = np.repeat(head[:, c], K)
        cols['max_corr'][rows] = corr.ravel()
    cols['nsrc'] = groups[star_row, 0].astype(np.int64)
    cols['label'] = label.astype(np.int64)
    cols['crowded'] = groups[star_row, 1] != 0
    assert tuple(cols) == _FIT_COLS_FOUND
    origin = origin.astype(np.int32)
    rows = np.flatnonzero(cols['crowded'])
    if crowded != 'skip' and rows.size:
        resid, _ = subtract_stars(im, ps, origin, cols, psf_index=np.zeros(origin.shape[0], dtype=np.int32),
                                  pixscale=pixscale, precision=precision, device=device)
        own = (np.rint(pos[rows]) - ps.shape[-1] // 2).astype(np.int32)
        shift_px = pos[rows] - (own + ps.shape[-1] // 2)
        start = None
        try:
            start = np.nan_to_num(np.asarray(found['scale'], dtype=float)[rows], nan=0.0, posinf=0.0, neginf=0.0)
        except (KeyError, IndexError, TypeError, ValueError):
            pass
        err_px = np.zeros((rows.size, 2))
        if crowded == 'free':
            out, shift_px, head = ctx.fit_frame_psf_free(resid, ps[None], own, var=va, shift=shift_px,
                                                         psf_index=np.zeros(rows.size, dtype=np.int32), scale0=start,
                                                         radius=radius, background=bool(fit_back))
            err_px = out[:, 10:12]
        else:
            out, head = ctx.fit_frame_psf(resid, ps[None], own, var=va, shift=shift_px,
                                          psf_index=np.zeros(rows.size, dtype=np.int32), scale0=start, radius=radius,
                                          background=bool(fit_back))
        ok = out[:, 7] == 0
        fill = rows[ok]
        cols['scale'][fill] = out[ok, 0]
        cols['flux'][fill] = out[ok, 2]
        cols['err_scale'][fill] = out[ok, 1]
        cols['err_flux'][fill] = out[ok, 3]
        cols['shift'][fill] = shift_px[ok] * pixscale
        cols['err_shift'][fill] = err_px[ok] * pixscale
        cols['back'][fill] = head[0]
        cols['err_back'][fill] = head[1]
        cols['chi2'][fill] = head[2]
        cols['npix'][fill] = int(head[3])
        cols['status'][fill] = int(head[7])
        cols['group'][rows] = origin.shape[0] + np.arange(rows.size)
        origin = np.concatenate([origin, own])
    return _make_table(cols), origin


_FIT_COLS_CROWDED = ('scale', 'shift', 'flux', 'err_scale', 'err_flux', 'overlap', 'npix', 'status')


def _crowded_inputs(psf, positions, psf_index, fit_back, start, pixscale):
    """(psf, psf_index, start, origin, shift in pixels) of fit_crowded_stars and refine_crowded_stars: the model stamps,
    the stars placed as cut_star_stamps places stamps, the start resolved."""
    _pixscale(pixscale)
    _args.flag('fit_back', fit_back)
    pos = _star_positions(positions)
    n = pos.shape[0]
    ps = _args.array('psf', psf, unwrap=True)
    if ps.ndim < 2 or ps.shape[-1] != ps.shape[-2] or ps.size == 0:
        raise ValueError('psf must have the shape (..., 40, 40)')
    dimpsf = ps.shape[-1]
    if not np.all(np.isfinite(pos)) or np.any(np.abs(pos) > _lib.MAX_ORIGIN - dimpsf):
        raise ValueError('positions must be finite and within 2^30 pixels')
    if psf_index is None and ps.size == dimpsf * dimpsf:
        psf_index = np.zeros(n, dtype=np.int32)
    if isinstance(start, str):
        if start != 'found':
            raise ValueError("start must be None, 'found' or one value per star")
        try:
            start = np.asarray(positions['scale'], dtype=float)
        except (KeyError, IndexError, TypeError, ValueError):
            raise ValueError("start='found' needs a find_stars table") from None
    origin = (np.rint(pos) - dimpsf // 2).astype(np.int32)
    shift_px = pos - (origin + dimpsf // 2)
    return ps, psf_index, start, origin, shift_px


_BACK_COLS = ('level', 'rms', 'raw_level', 'raw_rms', 'n_used', 'n_valid', 'passes', 'flags')
SKY_MAX_PASSES = 8


def background_map(image, var=None, *, box=32, filter=3, kappa=3.0, max_clip=5, min_frac=0.25, pixscale=0.2,
                   precision='mixed', device=0):
    """The background of a frame (ny, nx) or of every layer of a cube (nl, ny, nx), on the GPU: a mesh of `box` x `box`
    cells (8 .. 64 pixels), in each the median and 1.4826 x the median absolute deviation of the valid pixels under
    iterated clipping at `kappa` such sigmas (at most `max_clip` passes) -- exact order statistics, no sums --, a cell
    with fewer than `min_frac` of its pixels valid filled from its neighbours, a median filter over `filter` x
    `filter` cells (1, 3, 5) and a bicubic interpolation to the frame that continues gradients to the frame's edge.
    NaN pixels and var <= 0 are masked; var is a mask only.  Mask the stars (NaN) or pass the residual of a fit.

    Returns (map, rms, mesh): the background and its noise at every pixel, of the input's shape -- rms squared is a
    usable `var` for find_stars -- and a table with one row per cell in (layer, row, column) order: level, rms (after
    filter and fill), raw_level, raw_rms (NaN for a cell without enough valid pixels), n_used, n_valid, passes, flags
    (1 filled from neighbours, 2 clipping ended at max_clip, 4 MAD = 0).  mesh.meta: box, shape (the mesh: (my, mx), with
    nl in front for a cube), status (0 fine, 1 some cells filled, 2 no valid cell), valid_cells, filled_cells -- per
    layer for a cube."""
    _pixscale(pixscale)
    ctx = get_context(128, pixscale, 40, precision, device)
    bmap, rms, mesh, head = ctx.frame_background(image, var, box=box, filter=filter, kappa=kappa, max_clip=max_clip,
                                                 min_frac=min_frac)
    rows = mesh.reshape(-1, _lib.NBACK)
    cols = OrderedDict()
    for k, name in enumerate(_BACK_COLS):
        cols[name] = rows[:, k].copy() if k < 4 else rows[:, k].astype(np.int64)
    per_layer = (lambda v: [int(x) for x in v]) if head.ndim == 2 else int
    meta = OrderedDict([('box', int(box)), ('shape', tuple(mesh.shape[:-1])), ('status', per_layer(head[..., 0])),
                        ('valid_cells', per_layer(head[..., 1])), ('filled_cells', per_layer(head[..., 2]))])
    return bmap, rms, _make_table(cols, meta)


def _sky_parameters(sky):
    """(passes, background parameters) of the `sky` argument of fit_crowded_stars: True or a dict (ValueError)."""
    if sky is True:
        sky = {}
    if not isinstance(sky, dict):
        raise ValueError('sky must be None, True or a dict of background_map parameters and passes')
    par = dict(box=32, filter=3, kappa=3.0, max_clip=5, min_frac=0.25, passes=2)
    unknown = set(sky) - set(par)
    if unknown:
        raise ValueError('sky: unknown keys %s' % sorted(unknown))
    par.update(sky)
    passes = par.pop('passes')
    passes = _args.integer('passes', passes, 1, SKY_MAX_PASSES,
                           'sky: passes must be an integer between 1 and %d' % SKY_MAX_PASSES)
    box, filt, kappa, max_clip, min_frac = _lib.background_parameters(par['box'], par['filter'], par['kappa'],
                                                                      par['max_clip'], par['min_frac'])
    return passes, dict(box=box, filter=filt, kappa=kappa, max_clip=max_clip, min_frac=min_frac)


def fit_crowded_stars(image, psf, positions, *, var=None, psf_index=None, radius=8.0, fit_back=True, start=None,
                      max_iter=100, tol=1e-10, return_residual=False, sky=None, return_sky=False, pixscale=0.2,
                      precision='mixed', device=0):
    """Crowded-field PSF photometry, on the GPU: the fluxes of ALL stars of a frame at known positions in one linear
    least-squares solve -- no limit on how many stars touch each other; the step for the groups fit_found_stars
    marks `crowded`.  `image` (ny, nx), `var` its variance frame or None (NaN pixels and var <= 0 are masked);
    `positions` an (n, 2) array of (row, column) in pixels or a find_stars table; `psf` (..., 40, 40) model stamps,
    e.g. reconstructed PSFs, star k taking psf[psf_index[k]] (one stamp: every star takes it).  The fit runs over the
    valid pixels within `radius` (1 .. 20) pixels of a star, with one constant background under fit_back, by
    preconditioned conjugate gradients to the relative residual `tol` or max_iter steps, from `start`: None (zeros),
    'found' (the `scale` column of a find_stars table) or n values.

    Returns (fit, origin) in the form subtract_stars takes (pass it the same psf_index): origin[k] =
    rint(positions[k]) - 20 as cut_star_stamps places stamps, and `fit` with one row per star: scale (F), shift (2,
    arcsec, echoed: the position from the stamp centre), flux, err_scale and err_flux (CONDITIONAL errors: the other
    stars held fixed), overlap (the sum of the star's off-diagonal terms of the normal matrix over its diagonal term;
    far from 0 the conditional error is optimistic), npix (valid pixels within `radius` of the star) and status (0
    fitted, 1 off the frame, 2 left out: no valid pixel, or no model there).  fit.meta: back, err_back, chi2, npix
    (pixels of the solve), iterations, residual (the last relative preconditioned residual), status (0 converged, 1
    max_iter reached, 2 nothing fitted).  With return_residual also the frame minus the fitted stars.

    sky: None (the default: the single solve above), True or a dict of background_map's parameters (box, filter, kappa,
    max_clip, min_frac) and `passes` (default 2): a background that varies over the frame is estimated between solves
    instead of being pushed into the fluxes.  From map_0 = 0, for p = 1 .. passes: image - map_(p-1) is fitted with one
    constant, and map_p = map_(p-1) + the background map of that fit's residual; the final fit, with fit_back as given
    and started from the last fluxes, runs on image - map_passes.  fit.meta gains sky_passes; with return_sky the
    map is appended to the returned tuple (the residual is that of the final fit: the sky is taken out of it)."""
    ps, psf_index, start, origin, shift_px = _crowded_inputs(psf, positions, psf_index, fit_back, start, pixscale)
    dimpsf = ps.shape[-1]
    _args.flag('return_sky', return_sky)
    if sky is None and return_sky:
        raise ValueError('return_sky needs sky')
    passes, sky_par = (0, None) if sky is None else _sky_parameters(sky)
    ctx = get_context(128, pixscale, dimpsf, precision, device)
    sky_map = None
    if passes:
        image, var = _lib.frame_images(image, var)
        sky_map = np.zeros(image.shape)
        frame = image
        for _ in range(passes):
            rows, _, resid = ctx.fit_frame_psf(frame, ps, origin, var=var, shift=shift_px, psf_index=psf_index,
                                               scale0=start, radius=radius, background=True, max_iter=max_iter, tol=tol,
                                               return_residual=True)
            sky_map = sky_map + ctx.frame_background(resid, var, return_rms=False, **sky_par)[0]
            frame = image - sky_map
            start = np.where(np.isfinite(rows[:, 0]), rows[:, 0], 0.0)
        image = frame
    res = ctx.fit_frame_psf(image, ps, origin, var=var, shift=shift_px, psf_index=psf_index, scale0=start,
                            radius=radius, background=bool(fit_back), max_iter=max_iter, tol=tol,
                            return_residual=return_residual)
    rows, head = res[0], res[1]
    cols = OrderedDict()
    cols['scale'] = rows[:, 0].copy()
    cols['shift'] = shift_px * pixscale
    cols['flux'] = rows[:, 2].copy()
    cols['err_scale'] = rows[:, 1].copy()
    cols['err_flux'] = rows[:, 3].copy()
    cols['overlap'] = rows[:, 4].copy()
    cols['npix'] = rows[:, 5].astype(np.int64)
    cols['status'] = rows[:, 7].astype(np.int64)
    assert tuple(cols) == _FIT_COLS_CROWDED
    meta = OrderedDict([('back', float(head[0])), ('err_back', float(head[1])), ('chi2', float(head[2])),
                        ('npix', int(head[3])), ('iterations', int(head[4])), ('residual', float(head[5])),
                        ('status', int(head[7]))])
    if passes:
        meta['sky_passes'] = passes
    fit = _make_table(cols, meta)
    return (fit, origin) + ((res[2],) if return_residual else ()) + ((sky_map,) if return_sky else ())


_FIT_COLS_REFINED = ('scale', 'shift', 'position', 'flux', 'err_scale', 'err_shift', 'err_flux', 'overlap', 'moved', 'npix',
                     'free', 'flags', 'status')


def refine_crowded_stars(image, psf, positions, *, var=None, psf_index=None, radius=8.0, fit_back=True, start=None,
                         max_iter=100, tol=1e-10, max_outer=8, pos_tol=1e-3, max_step=0.5, max_move=2.0, min_snr=3.0,
                         return_residual=False, pixscale=0.2, precision='mixed', device=0):
    """Crowded-field PSF photometry with free positions, on the GPU: fit_crowded_stars with the positions of the stars
    refined beside their fluxes -- all stars at once, by Gauss-Newton, no limit on how many stars touch each other.
    image, var, psf, psf_index, positions, radius, fit_back, start, max_iter and tol: as fit_crowded_stars; `positions`
    is the start.  The pixels fitted are those within `radius` of the START positions and stay.  Up to `max_outer`
    (0 .. 16) steps move the stars whose flux stands `min_snr` conditional errors above zero, every step clipped to
    `max_step` (0 .. 1] pixels per axis and every star kept within `max_move` (0 .. 4] pixels of its start, until the
    largest step is <= `pos_tol` pixels; the fluxes returned are solved at the final positions.

    Returns (fit, origin) in the form subtract_stars takes (pass it the same psf_index): origin as fit_crowded_stars
    places it, from the START positions -- it does not move --, and `fit` with one row per star: scale (F), shift (2,
    arcsec: the REFINED position from the stamp centre), position (2, pixels: the refined (row, column)), flux,
    err_scale, err_shift (2, arcsec) and err_flux (CONDITIONAL errors: the other stars held fixed), overlap, moved (2,
    arcsec: refined minus start), npix, free (the steps in which the star moved), flags (FRAME_FREE_HELD,
    FRAME_FREE_BOUND, FRAME_FREE_CLIPPED of muse_psfr_amd) and status (0 fitted, 1 off the frame, 2 left out).
    fit.meta: back, err_back, chi2, npix, iterations (of the closing solve), residual, status (0 positions and fluxes
    converged, 1 fitted but not converged, 2 nothing fitted), outer (steps done), step (the last largest step, pixels),
    nfree (stars free in the last step), inner (iterations of all solves).  With return_residual also the frame minus
    the fitted stars at the refined positions."""
    ps, psf_index, start, origin, shift_px = _crowded_inputs(psf, positions, psf_index, fit_back, start, pixscale)
    dimpsf = ps.shape[-1]
    ctx = get_context(128, pixscale, dimpsf, precision, device)
    res = ctx.fit_frame_psf_free(image, ps, origin, var=var, shift=shift_px, psf_index=psf_index, scale0=start,
                                 radius=radius, background=bool(fit_back), max_iter=max_iter, tol=tol,
                                 max_outer=max_outer, pos_tol=pos_tol, max_step=max_step, max_move=max_move,
                                 min_snr=min_snr, return_residual=return_residual)
    rows, shifts, head = res[0], res[1], res[2]
    cols = OrderedDict()
    cols['scale'] = rows[:, 0].copy()
    cols['shift'] = shifts * pixscale
    cols['position'] = (origin + dimpsf // 2) + shifts
    cols['flux'] = rows[:, 2].copy()
    cols['err_scale'] = rows[:, 1].copy()
    cols['err_shift'] = rows[:, 10:12] * pixscale
    cols['err_flux'] = rows[:, 3].copy()
    cols['overlap'] = rows[:, 4].copy()
    cols['moved'] = rows[:, 12:14] * pixscale
    cols['npix'] = rows[:, 5].astype(np.int64)
    cols['free'] = rows[:, 15].astype(np.int64)
    cols['flags'] = rows[:, 14].astype(np.int64)
    cols['status'] = rows[:, 7].astype(np.int64)
    assert tuple(cols) == _FIT_COLS_REFINED
    meta = OrderedDict([('back', float(head[0])), ('err_back', float(head[1])), ('chi2', float(head[2])),
                        ('npix', int(head[3])), ('iterations', int(head[4])), ('residual', float(head[5])),
                        ('status', int(head[7])), ('outer', int(head[8])), ('step', float(head[9])),
                        ('nfree', int(head[10])), ('inner', int(head[11]))])
    fit = _make_table(cols, meta)
    return (fit, origin) + ((res[3],) if return_residual else ())


def _crowded_spectra_inputs(psf, positions, lbda, psf_index, layer_shift, fit_back, start, pixscale):
    """(psf (npsf, nl, 40, 40), psf_index, lbda, layer_shift in pixels, start, origin, shift in pixels) of
    fit_crowded_spectra and refine_crowded_spectra: the model cubes, the stars placed as cut_star_stamps places stamps,
    the start resolved."""
    _pixscale(pixscale)
    _args.flag('fit_back', fit_back)
    pos = _star_positions(positions)
    n = pos.shape[0]
    ps = _args.array('psf', psf, unwrap=True)
    if ps.ndim not in (3, 4) or ps.shape[-1] != ps.shape[-2] or ps.size == 0:
        raise ValueError('psf must have the shape (nl, 40, 40) or (npsf, nl, 40, 40)')
    dimpsf = ps.shape[-1]
    if not np.all(np.isfinite(pos)) or np.any(np.abs(pos) > _lib.MAX_ORIGIN - dimpsf):
        raise ValueError('positions must be finite and within 2^30 pixels')
    if ps.ndim == 3:
        if psf_index is not None:
            raise ValueError('psf_index needs psf of the shape (npsf, nl, 40, 40)')
        ps = ps[None]
        psf_index = np.zeros(n, dtype=np.int32)
    nl = ps.shape[1]
    if lbda is not None:
        lbda = np.array(_args.array('lbda', lbda))          # (the caller's array is not handed on)
        if lbda.shape != (nl,):
            raise ValueError('lbda must hold one wavelength per layer (%d)' % nl)
    if layer_shift is not None:
        layer_shift = _args.array('layer_shift', layer_shift) / pixscale
    if isinstance(start, str):
        if start != 'found':
            raise ValueError("start must be None, 'found' or (nl, n) values")
        try:
            found = np.asarray(positions['scale'], dtype=float)
        except (KeyError, IndexError, TypeError, ValueError):
            raise ValueError("start='found' needs a find_stars table") from None
        start = np.broadcast_to(found, (nl, n))
    origin = (np.rint(pos) - dimpsf // 2).astype(np.int32)
    shift_px = pos - (origin + dimpsf // 2)
    return ps, psf_index, lbda, layer_shift, start, origin, shift_px


_FIT_COLS_CROWDED_SPECTRA = ('shift', 'scale', 'flux', 'err_scale', 'err_flux', 'overlap', 'npix', 'status')
_META_CROWDED_SPECTRA = ('back', 'err_back', 'chi2', 'npix', 'iterations', 'residual', 'status')


def fit_crowded_spectra(cube, psf, positions, *, lbda=None, var=None, psf_index=None, layer_shift=None, radius=8.0,
                        fit_back=True, start=None, max_iter=100, tol=1e-10, layer_batch=0, return_residual=False,
                        pixscale=0.2, precision='mixed', device=0):
    """Crowded-field PSF spectroscopy, on the GPU: the spectra of ALL stars of a cube at known positions -- the solve
    of fit_crowded_stars on every wavelength layer, the layers side by side in one call, bit for bit what a loop of
    fit_crowded_stars over the layers gives.  `cube` (nl, ny, nx), `var` its variance cube or None (NaN pixels and var
    <= 0 are masked); `positions` an (n, 2) array of (row, column) in pixels or a find_stars table, the same in every
    layer; `layer_shift` (nl, 2) arcsec or None: the offset of a layer common to all stars (differential refraction),
    added to every star's position in that layer -- a position plus offset must stay within 8 pixels of the star's
    stamp centre; `psf` (nl, 40, 40), one model cube for every star, e.g. the reconstructed PSF per wavelength, or
    (npsf, nl, 40, 40) with star k taking psf[psf_index[k]].  radius, fit_back, max_iter, tol: as fit_crowded_stars,
    per layer.  `start`: None (zeros), 'found' (the `scale` column of a find_stars table, for every layer) or (nl, n)
    values.  `layer_batch`: layers solved side by side (0: as many as the library's work memory budget holds).
    `lbda` (nl,): wavelengths, echoed into fit.meta.

    Returns (fit, origin): origin as fit_crowded_stars places it, and `fit` with one row per star: shift (2, arcsec,
    echoed: the position from the stamp centre, without the layer's offset) and the (n, nl) columns scale, flux,
    err_scale, err_flux, overlap, npix and status of fit_crowded_stars.  fit.meta holds the per-layer arrays (nl,) back,
    err_back, chi2, npix, iterations, residual and status, and lbda if given.  With return_residual also the cube minus
    the fitted stars."""
    ps, psf_index, lbda, layer_shift, start, origin, shift_px = _crowded_spectra_inputs(
        psf, positions, lbda, psf_index, layer_shift, fit_back, start, pixscale)
    dimpsf = ps.shape[-1]
    ctx = get_context(128, pixscale, dimpsf, precision, device)
    res = ctx.fit_cube_psf(cube, ps, origin, var=var, shift=shift_px, layer_shift=layer_shift, psf_index=psf_index,
                           scale0=start, radius=radius, background=bool(fit_back), max_iter=max_iter, tol=tol,
                           layer_batch=layer_batch, return_residual=return_residual)
    rows, head = res[0], res[1]                                    # (nl, n, 8), (nl, 8)
    cols = OrderedDict()
    cols['shift'] = shift_px * pixscale
    for name, c in (('scale', 0), ('flux', 2), ('err_scale', 1), ('err_flux', 3), ('overlap', 4)):
        cols[name] = np.ascontiguousarray(rows[:, :, c].T)
    cols['npix'] = np.ascontiguousarray(rows[:, :, 5].T).astype(np.int64)
    cols['status'] = np.ascontiguousarray(rows[:, :, 7].T).astype(np.int64)
    assert tuple(cols) == _FIT_COLS_CROWDED_SPECTRA
    meta = OrderedDict()
    for name, c in zip(_META_CROWDED_SPECTRA, (0, 1, 2, 3, 4, 5, 7)):
        meta[name] = head[:, c].astype(np.int64) if name in ('npix', 'iterations', 'status') else head[:, c].copy()
    if lbda is not None:
        meta['lbda'] = lbda
    fit = _make_table(cols, meta)
    return (fit, origin) + ((res[2],) if return_residual else ())


_FIT_COLS_REFINED_SPECTRA = ('shift', 'position', 'scale', 'flux', 'err_scale', 'err_shift', 'err_flux', 'overlap', 'moved',
                             'npix', 'free', 'flags', 'status')
_META_REFINED_SPECTRA = ('chi2_all', 'dof', 'outer', 'step', 'nfree', 'inner', 'call_status', 'call_residual')


def _take_layers(a, sel):
    """The layers `sel` of a cube-like argument (an array, a masked array or an object with .data), or None."""
    if a is None:
        return None
    if not isinstance(a, np.ma.MaskedArray):
        a = getattr(a, 'data', a)
    if not isinstance(a, np.ma.MaskedArray):
        try:
            a = np.asarray(a, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('cube and var must be numeric arrays') from None
    if a.ndim != 3:
        raise ValueError('cube and var must have the shape (nl, ny, nx)')
    return a[sel]


def refine_crowded_spectra(cube, psf, positions, *, lbda=None, var=None, psf_index=None, layer_shift=None,
                           position_layers=None, radius=8.0, fit_back=True, start=None, max_iter=100, tol=1e-10,
                           max_outer=8, pos_tol=1e-3, max_step=0.5, max_move=2.0, min_snr=3.0, return_residual=False,
                           pixscale=0.2, precision='mixed', device=0):
    """Crowded-field PSF spectroscopy with free positions, on the GPU: fit_crowded_spectra with ONE position per star
    refined from the layers of the cube jointly -- every layer with its own PSF and its own offset `layer_shift`, all
    stars and all layers in one Gauss-Newton loop (refine_crowded_stars' on the whole cube).  cube, psf, positions
    (the start), lbda, var, psf_index, layer_shift, radius, fit_back, start, max_iter, tol: as fit_crowded_spectra;
    max_outer, pos_tol, max_step, max_move, min_snr: as refine_crowded_stars.  A layer moves a star only where the
    star's flux stands `min_snr` conditional errors above zero in that layer.

    `position_layers`: an index array or a slice of the layers that determine the positions; None: all layers, which
    must then fit into the library's work memory budget (CUBE_FREE_WORK_BYTES).  With a proper subset the positions
    are refined on those layers, and the spectra of the WHOLE cube are then solved at the refined positions by
    fit_crowded_spectra's solve -- this is how a cube of thousands of layers is served: positions from a few dozen
    layers, spectra from all.

    Returns (fit, origin): origin as fit_crowded_spectra places it, from the START positions, and `fit` with one row
    per star: shift (2, arcsec: the REFINED position from the stamp centre, without the layer's offset), position (2,
    pixels), err_shift (2, arcsec, conditional), moved (2, arcsec: refined minus start), free (the steps in which the
    star moved), flags (FRAME_FREE_HELD, FRAME_FREE_BOUND, FRAME_FREE_CLIPPED) and the (n, nl) columns scale, flux,
    err_scale, err_flux, overlap, npix and status of fit_crowded_spectra.  fit.meta: the per-layer arrays of
    fit_crowded_spectra, the head of the position call -- chi2_all, dof, outer, step, nfree, inner, call_status (0
    positions and closing solve converged, 1 anything else fitted, 2 nothing fitted), call_residual --,
    position_layers, and lbda if given.  With return_residual also the cube minus the fitted stars at the refined
    positions."""
    ps, psf_index, lbda, layer_shift, start, origin, shift_px = _crowded_spectra_inputs(
        psf, positions, lbda, psf_index, layer_shift, fit_back, start, pixscale)
    dimpsf, nl = ps.shape[-1], ps.shape[1]
    if position_layers is None:
        sel = np.arange(nl)
    else:
        try:
            sel = np.arange(nl)[position_layers]
        except (IndexError, TypeError, ValueError):
            raise ValueError('position_layers must be a slice or an array of layer indices in 0 .. %d' % (nl - 1)) from None
        sel = np.atleast_1d(sel)
        if sel.ndim != 1 or sel.size == 0 or np.unique(sel).size != sel.size:
            raise ValueError('position_layers must name at least one layer, and each layer once')
    whole = sel.size == nl and np.array_equal(sel, np.arange(nl))
    ctx = get_context(128, pixscale, dimpsf, precision, device)
    free = dict(radius=radius, background=bool(fit_back), max_iter=max_iter, tol=tol, max_outer=max_outer,
                pos_tol=pos_tol, max_step=max_step, max_move=max_move, min_snr=min_snr)
    if whole:
        res = ctx.fit_cube_psf_free(cube, ps, origin, var=var, shift=shift_px, layer_shift=layer_shift,
                                    psf_index=psf_index, scale0=start, return_residual=return_residual, **free)
        rows, pos_rows, shifts, head, call = res[:5]
        resid = res[5] if return_residual else None
    else:
        sub_start = None if start is None else np.asarray(start, dtype=np.float64)
        if sub_start is not None and sub_start.shape != (nl, origin.shape[0]):
            raise ValueError('start must have the shape (%d, %d)' % (nl, origin.shape[0]))
        sub_cube = _take_layers(cube, sel)
        if _take_layers(cube, slice(None)).shape[0] != nl:
            raise ValueError('cube must have the %d layers of psf' % nl)
        if layer_shift is not None and np.shape(layer_shift) != (nl, 2):
            raise ValueError('layer_shift must have the shape (%d, 2)' % nl)
        _, pos_rows, shifts, _, call = ctx.fit_cube_psf_free(
            sub_cube, ps[:, sel], origin, var=_take_layers(var, sel), shift=shift_px,
            layer_shift=None if layer_shift is None else layer_shift[sel], psf_index=psf_index,
            scale0=None if sub_start is None else sub_start[sel], **free)
        res = ctx.fit_cube_psf(cube, ps, origin, var=var, shift=shifts, layer_shift=layer_shift, psf_index=psf_index,
                               scale0=start, radius=radius, background=bool(fit_back), max_iter=max_iter, tol=tol,
                               return_residual=return_residual)
        rows, head = res[0], res[1]
        resid = res[2] if return_residual else None
    cols = OrderedDict()
    cols['shift'] = shifts * pixscale
    cols['position'] = (origin + dimpsf // 2) + shifts
    for name, c in (('scale', 0), ('flux', 2), ('err_scale', 1)):
        cols[name] = np.ascontiguousarray(rows[:, :, c].T)
    cols['err_shift'] = pos_rows[:, 2:4] * pixscale
    for name, c in (('err_flux', 3), ('overlap', 4)):
        cols[name] = np.ascontiguousarray(rows[:, :, c].T)
    cols['moved'] = pos_rows[:, 4:6] * pixscale
    cols['npix'] = np.ascontiguousarray(rows[:, :, 5].T).astype(np.int64)
    cols['free'] = pos_rows[:, 7].astype(np.int64)
    cols['flags'] = pos_rows[:, 6].astype(np.int64)
    cols['status'] = np.ascontiguousarray(rows[:, :, 7].T).astype(np.int64)
    assert tuple(cols) == _FIT_COLS_REFINED_SPECTRA
    meta = OrderedDict()
    for name, c in zip(_META_CROWDED_SPECTRA, (0, 1, 2, 3, 4, 5, 7)):
        meta[name] = head[:, c].astype(np.int64) if name in ('npix', 'iterations', 'status') else head[:, c].copy()
    for name, c in zip(_META_REFINED_SPECTRA, range(8)):
        meta[name] = int(call[c]) if name in ('outer', 'nfree', 'inner', 'call_status') else float(call[c])
    meta['position_layers'] = sel.copy()
    if lbda is not None:
        meta['lbda'] = lbda
    fit = _make_table(cols, meta)
    return (fit, origin) + ((resid,) if return_residual else ())


def cut_star_stamps(image, positions, var=None, dimpsf=40, *, pixscale=0.2, precision='mixed', device=0):
    """Stamps of stars out of a frame, on the GPU: `image` (ny, nx), `positions` (n, 2) the (row, column) star centres
    in pixels.  Stamp k starts at origin[k] = rint(positions[k]) - dimpsf // 2, so the star sits within half a pixel of
    the stamp's pixel (dimpsf // 2, dimpsf // 2); where a stamp leaves the frame its pixels are NaN (variance 0), which
    the fits mask.  var: the variance frame (the image's shape) or None.

    Returns (stamps, var_stamps or None, origin): (n, dimpsf, dimpsf) arrays and the (n, 2) int32 origins that
    render_star_field and subtract_stars take."""
    pos = _args.array('positions', positions)
    if pos.ndim != 2 or pos.shape[1] != 2 or pos.shape[0] < 1:
        raise ValueError('positions must have the shape (n, 2)')
    if not np.all(np.isfinite(pos)) or np.any(np.abs(pos) > _lib.MAX_ORIGIN - dimpsf):
        raise ValueError('positions must be finite and within 2^30 pixels')
    origin = (np.rint(pos) - dimpsf // 2).astype(np.int32)
    ctx = get_context(128, pixscale, dimpsf, precision, device)
    res = ctx.cut_stamps(image, origin, var=var)
    return (res, None, origin) if var is None else (res[0], res[1], origin)


def _shift_pixels(shift, pixscale):
    return None if shift is None else _args.array('shift', shift) / pixscale


def render_star_field(shape, psf, origin, scale, shift=None, psf_index=None, pixscale=0.2, *, image=None,
                      return_status=False, precision='mixed', device=0):
    """A star field from model stamps, on the GPU: star k is scale[k] times the model stamp psf[psf_index[k]] (psf[k]
    without psf_index; (..., 40, 40), e.g. reconstructed PSFs) resampled by cubic convolution at the sub-pixel `shift`
    (n, 2) (row, column) in arcsec, like the fit tables; None: no shift), with its stamp's pixel [0][0] on the frame
    pixel origin[k].  The stars are added to `image`, or to an empty frame of `shape` = (ny, nx).  Returns the frame;
    with return_status also the (n,) render status (0 rendered, 1 off the frame)."""
    _pixscale(pixscale)
    ctx = get_context(128, pixscale, np.shape(psf)[-1] if np.ndim(psf) >= 2 else 40, precision, device)
    res = ctx.render_stars(psf, origin, scale, shift=_shift_pixels(shift, pixscale), psf_index=psf_index, image=image,
                           shape=shape, return_status=return_status)
    return (res[0], res[1][:, 0].astype(np.int64)) if return_status else res


def subtract_stars(image, psf, origin, fit, psf_index=None, pixscale=0.2, keep=None, *, precision='mixed', device=0):
    """The residual frame of PSF-fitting photometry: `image` minus the fitted models of the stars of `fit`, a table of
    fit_stars_with_psf (row k is the star whose stamp was cut at origin[k]) or of fit_star_groups_with_psf (one row per
    source; its `group` column indexes `origin` and `psf_index`).  psf / psf_index as the fit took them; pixscale the
    one the fit used (the tables hold the shift in arcsec).  Rows with status & 3 == 2 (not fitted) are not subtracted;
    `keep` is an optional boolean mask of rows to leave in the frame -- subtract the neighbours and keep the target.
    A row whose scale or shift is not finite, or whose shift lies beyond 8 pixels, is skipped like a status-2 row.

    Returns (residual, status): the frame and per row 0 subtracted, 1 the star's footprint misses the frame, 2 skipped
    because of its values, -1 not asked for (status 2 in the table, or kept)."""
    _pixscale(pixscale)
    try:
        sc = np.asarray(fit['scale'], dtype=float).ravel()
        sh = np.asarray(fit['shift'], dtype=float).reshape(-1, 2) / pixscale
        st = np.asarray(fit['status']).astype(np.int64).ravel()
    except (KeyError, TypeError, ValueError, IndexError):
        raise ValueError('fit must be a table with the columns scale, shift and status') from None
    nrow = sc.size
    if nrow < 1 or sh.shape[0] != nrow or st.size != nrow:
        raise ValueError('fit must hold at least one row')
    try:
        grp = np.asarray(fit['group']).astype(np.int64).ravel()
    except KeyError:
        grp = np.arange(nrow)
    if grp.size != nrow:
        raise ValueError('the group column must hold one entry per row')
    og = _lib.star_origins(origin)
    if np.any(grp < 0) or np.any(grp >= og.shape[0]):
        raise ValueError('origin must hold one row per star (or group) of the fit')
    ngroup = og.shape[0]
    ps, ix, _, _ = _lib.psf_fit_arguments(ngroup, psf, psf_index, None, True, False, np.shape(psf)[-1])
    ix = np.arange(ngroup, dtype=np.int32) if ix is None else ix
    if keep is None:
        kp = np.zeros(nrow, dtype=bool)
    else:
        kp = np.asarray(keep)
        if kp.dtype != np.bool_ or kp.shape != (nrow,):
            raise ValueError('keep must be a boolean mask with one entry per row of fit')
    im, _ = _lib.frame_images(image)
    status = np.full(nrow, -1, dtype=np.int64)
    want = ((st & 3) != 2) & ~kp
    with np.errstate(invalid='ignore'):
        good = np.isfinite(sc) & np.all(np.abs(sh) <= _lib.FIT_PSF_MAX_SHIFT, axis=1)
    status[want & ~good] = 2
    rows = np.flatnonzero(want & good)
    if rows.size == 0:
        return im.copy(), status
    ctx = get_context(128, pixscale, ps.shape[-1], precision, device)
    res, out = ctx.render_stars(ps, og[grp[rows]], sc[rows], shift=sh[rows], psf_index=ix[grp[rows]], image=im,
                                subtract=True, return_status=True)
    status[rows] = out[:, 0].astype(np.int64)
    return res, status


METRIC_RADII = (0.2, 0.4, 0.6, 1.0, 2.0)      # default encircled-energy radii [arcsec]
METRIC_BOXES = (0.2, 0.4, 0.6, 1.0)           # default ensquared-energy box sides [arcsec] (0.2": the WFM spaxel)
METRIC_FRACTIONS = (0.5, 0.8)                 # default fractions of the EE radii
_METRIC_COLS = ('ee', 'sqe', 'r_ee')


def _metrics_request(metrics, pixscale, dimpsf=40):
    """The `metrics` argument of the compute_* functions -> None, or dict(radii, boxes, fractions [arcsec], center)
    with the defaults of psf_metrics filled in and the values validated (ValueError)."""
    if metrics is None or metrics is False:
        return None
    req = dict(radii=METRIC_RADII, boxes=METRIC_BOXES, fractions=METRIC_FRACTIONS, center='centroid')
    if metrics is not True:
        if not isinstance(metrics, dict):
            raise ValueError('metrics must be None, True or a dict(radii=, boxes=, fractions=, center=)')
        extra = set(metrics) - set(req)
        if extra:
            raise ValueError('unknown metrics key(s): %s' % ', '.join(sorted(map(str, extra))))
        req.update(metrics)
    _metric_arguments(req['radii'], req['boxes'], req['fractions'], req['center'], pixscale, dimpsf)
    return req


def _metric_arguments(radii, boxes, fractions, center, pixscale, dimpsf, nstamp=None):
    """Validated (radii_px, boxes_px, fractions, radii, boxes, centers) of a psf_metrics call: the pixel arrays of the
    library call, the arcsec arrays of the meta, and the (nstamp, 2) centres or None (the centroid).  ValueError."""
    try:
        ps = float(pixscale)
    except (TypeError, ValueError):
        raise ValueError('pixscale must be a positive number') from None
    if not (np.isfinite(ps) and ps > 0):
        raise ValueError('pixscale must be a positive number')
    arc = []
    for name, v in (('radii', radii), ('boxes', boxes)):
        try:
            arc.append(np.atleast_1d(np.asarray(() if v is None else v, dtype=float)))
        except (TypeError, ValueError):
            raise ValueError('%s must be numbers (arcsec)' % name) from None
    rad, box, frac = _lib.metric_parameters(arc[0] / ps, arc[1] / ps, fractions, dimpsf)
    if isinstance(center, str):
        if center not in ('centroid', 'stamp'):
            raise ValueError("center must be 'centroid', 'stamp' or an (n, 2) array of (p, q) in pixels")
        ce = None
        if center == 'stamp' and nstamp is not None:
            ce = np.full((nstamp, 2), (dimpsf - 1) / 2.0)
    elif center is None:
        raise ValueError("center must be 'centroid', 'stamp' or an (n, 2) array of (p, q) in pixels")
    elif nstamp is None:
        try:
            ce = np.asarray(center, dtype=float)
        except (TypeError, ValueError):
            raise ValueError('center must be an (n, 2) array of (p, q) in pixels') from None
        if ce.ndim != 2 or ce.shape[1] != 2 or not np.all(np.isfinite(ce)):
            raise ValueError('center must be a finite (n, 2) array of (p, q) in pixels')
    else:
        ce = _lib.metric_centers(center, nstamp)
    return rad, box, frac, arc[0], arc[1], ce


def _metric_columns(rows, nrad, nbox, nfrac, pixscale):
    """Library metric rows (n, NMET_HEAD + nrad + nbox + nfrac) -> the columns of psf_metrics (r_ee in arcsec)."""
    h = _lib.NMET_HEAD
    cols = OrderedDict()
    cols['flux'] = rows[:, 0].copy()
    cols['peak'] = rows[:, 1].copy()
    cols['center'] = rows[:, 4:6].copy()
    cols['ee'] = rows[:, h:h + nrad].copy()
    cols['sqe'] = rows[:, h + nrad:h + nrad + nbox].copy()
    cols['r_ee'] = rows[:, h + nrad + nbox:h + nrad + nbox + nfrac] * pixscale
    cols['status'] = rows[:, 6].astype(np.int64)
    return cols


def _metric_meta(radii, boxes, fractions, center):
    """The parameters of a metrics table for its meta / FITS header: MRAD1.., MBOX1.. [arcsec], MFRAC1.., MCENTER."""
    meta = OrderedDict()
    for key, vals in (('MRAD', radii), ('MBOX', boxes), ('MFRAC', fractions)):
        for k, v in enumerate(np.atleast_1d(vals)):
            meta['%s%d' % (key, k + 1)] = float(v)
    meta['MCENTER'] = center if isinstance(center, str) else 'given'
    return meta


def psf_metrics(psfcube, radii=METRIC_RADII, boxes=METRIC_BOXES, fractions=METRIC_FRACTIONS, center='centroid', *,
                pixscale=0.2, precision='mixed', device=0):
    """Energy metrics of PSF stamps, on the GPU (mpsfr_stamp_metrics): the encircled energy inside the ``radii``, the
    ensquared energy in the boxes of side ``boxes`` (both in arcsec, with the exact overlap of every pixel -- no pixel
    mask) and the radii [arcsec] that hold the ``fractions`` of the light, as fractions of the flux on the stamp.

    ``psfcube``: stamps of any leading shape (..., dimpsf, dimpsf).  ``center``: ``'centroid'`` (the flux-weighted first
    moment of each stamp), ``'stamp'`` (the geometric centre of the stamp, pixel coordinate (dimpsf - 1) / 2 = 19.5 in
    both axes) or an (n, 2) array of (p, q) in pixels, e.g. the ``center`` column of a fit table.  The reconstructed
    stamps of this package peak at pixel (20, 20) (their centroid lies within 0.07 px of it), half a pixel from the
    geometric centre: ``'stamp'`` is meant for stamps that are symmetric about the middle of the array, for the
    reconstructed ones use ``'centroid'`` or the fit centres.

    Returns a table, one row per stamp, with the columns flux (sum of the stamp), peak (brightest pixel), center (p, q
    in pixels), ee (n, nrad), sqe (n, nbox), r_ee (n, nfrac; arcsec) and status (0; 1: an EE radius is not converged; 2:
    non-finite pixels or flux <= 0 -- ee, sqe, r_ee are NaN); radii, boxes, fractions and the centre rule are in the meta
    (MRADk, MBOXk, MFRACk, MCENTER).  The arithmetic is fp64 whatever ``precision`` (which only selects the cached
    context).  Every refusal is a ValueError raised before a GPU context exists."""
    st = _lib.metric_stamps(psfcube)
    rad, box, frac, ra, ba, ce = _metric_arguments(radii, boxes, fractions, center, pixscale, st.shape[-1], st.shape[0])
    _check_precision(precision)
    ctx = get_context(128, pixscale, st.shape[-1], precision, device)
    rows = ctx.stamp_metrics(st, rad, box, frac, centers=ce)
    return _make_table(_metric_columns(rows, rad.size, box.size, frac.size, float(pixscale)),
                       _metric_meta(ra, ba, frac, center))


def _append_metrics(cols, psf, req, ctx, pixscale):
    """The ee, sqe, r_ee columns of the stamps `psf` (row for row with the fit columns of `cols`) appended to `cols`."""
    st = _lib.metric_stamps(psf, psf.shape[-1])
    rad, box, frac, _, _, ce = _metric_arguments(req['radii'], req['boxes'], req['fractions'], req['center'], pixscale,
                                                 st.shape[-1], st.shape[0])
    m = _metric_columns(ctx.stamp_metrics(st, rad, box, frac, centers=ce), rad.size, box.size, frac.size,
                        float(pixscale))
    for k in _METRIC_COLS:
        cols[k] = m[k]


def _metrics_hdu(lead, psf, req, ctx, pixscale, meta, name):
    """A METRICS_* HDU: the columns `lead` (an OrderedDict, one row per stamp of `psf`), then those of psf_metrics
    (2-D columns without entries are left out: a FITS column needs a width)."""
    st = _lib.metric_stamps(psf, psf.shape[-1])
    rad, box, frac, ra, ba, ce = _metric_arguments(req['radii'], req['boxes'], req['fractions'], req['center'],
                                                   pixscale, st.shape[-1], st.shape[0])
    cols = OrderedDict(lead)
    m = _metric_columns(ctx.stamp_metrics(st, rad, box, frac, centers=ce), rad.size, box.size, frac.size,
                        float(pixscale))
    cols.update((k, v) for k, v in m.items() if v.ndim == 1 or v.shape[1] > 0)
    hmeta = OrderedDict(meta)
    hmeta.update(_metric_meta(ra, ba, frac, req['center']))
    return _table_hdu(cols, hmeta, name)


def simul_psd_wfm(Cn2, h, seeing, L0, zenith=0., plot=False, npsflin=1, dim=1280, three_lgs_mode=False,
                  verbose=True, *, precision='mixed', cutoff_masks='host', device=0, wind_speed=None, wind_dir=None):
    """Residual phase PSD of the MUSE wide-field mode for each evaluation direction (psfrec.py:36-151):
    (npsflin**2, dim, dim) float64, DC at [dim/2, dim/2], in nm^2 m^2 like the reference's.  Two layers
    (`Cn2` = their weights, normalised here as psfrec.py:57-58 does); the zenith angle only rescales r0
    (psfrec.py:108, 183-187).

    With ``wind_dir`` (radians, one per layer) the atmosphere is a Cn2 profile of 1 to 8 layers: ``h`` their
    altitudes, ``wind_speed`` their speeds (scalar or per layer; by default np.full_like(h, 12.5) as
    psfrec.py:61 has it -- 12 m/s for integer altitudes).  ``wind_speed`` without ``wind_dir`` is refused
    (ValueError): the two-layer call keeps the reference's winds."""
    if wind_dir is not None:
        if wind_speed is None:
            wind_speed = np.full_like(np.array(h), 12.5)
        hh, ws, wd = _lib.profile_layers(h, wind_speed, wind_dir)
        w = _lib.profile_weights(np.ravel(np.array(Cn2, dtype=float)), 1, hh.size)
        if plot:
            direction_perf(npsflin, plot=True)
        seeing_los = float(seeing) / np.cos(np.deg2rad(zenith)) ** (3 / 5)
        ctx = get_context(dim, 0.2, 40, precision, device)
        return ctx.simul_psd_profile(seeing_los, L0, w[0], hh, ws, wd, three_lgs_mode, npsflin=npsflin,
                                     masks=_resolve_masks(cutoff_masks))
    if wind_speed is not None:
        raise ValueError('wind_speed is a profile argument: give wind_dir too (without it the reference\'s '
                         'atmosphere applies, psfrec.py:61)')
    Cn2 = np.array(Cn2, dtype=float)
    if Cn2.size != 2 or len(h) != 2:
        raise ValueError('exactly two layers are supported (psfrec.py:66 fixes two wind directions)')
    Cn2 = Cn2 / Cn2.sum()
    if verbose and three_lgs_mode:
        logger.info('Using three lasers mode')
    if plot:
        direction_perf(npsflin, plot=True)
    seeing_los = float(seeing) / np.cos(np.deg2rad(zenith)) ** (3 / 5)
    ctx = get_context(dim, 0.2, 40, precision, device)
    return ctx.simul_psd(seeing_los, Cn2[0], L0, three_lgs_mode, h, npsflin=npsflin,
                         masks=_resolve_masks(cutoff_masks))


def psf_muse(psd, lambdamuse, *, pixscale=0.2, precision='mixed', device=0):
    """PSF stamps (nl, 40, 40) at the wavelengths `lambdamuse` [nm] from a residual PSD (psfrec.py:644-686:
    structure function, OTF, crop to the field of the stamp, bilinear sampling; the mean over the
    directions when the PSD has three dimensions).  Any real PSD image of a supported size."""
    psd = np.asarray(psd, dtype=float)
    ctx = get_context(psd.shape[-1], pixscale, 40, precision, device)
    try:
        return ctx.psf_from_psd(psd, np.atleast_1d(np.asarray(lambdamuse, dtype=float)))
    except MpsfrError as e:
        if e.code == E_GRID:
            raise ValueError(str(e)) from None
        raise


# ---- psd_to_psf (psfrec.py:689-807) and the pupil / resampling helpers its callers use -----------------

_P2P_SIZES = (128, 256, 512, 1024, 1280)    # the transform lengths libmpsfr plans for


def seeing2r01(seeing, lbda, zenith):
    """r0 [m] at the wavelength `lbda` [um] and zenith angle `zenith` [deg] of a seeing [arcsec] given at
    0.5 um (psfrec.py:183-187)."""
    r0_500 = 0.976 * 0.5 / seeing / 4.85
    airmass_term = np.cos(np.deg2rad(zenith)) ** (3 / 5)
    return r0_500 * (lbda * 2) ** (6 / 5) * airmass_term


def pupil_mask(radius, width, oc=0, inverse=False):
    """Telescope pupil (psfrec.py:190-203): an int array (width, width), 1 where the distance to the centre
    ((width - 1) / 2), in units of `radius` pixels, is in [oc, 1); `inverse` swaps 0 and 1."""
    c = (width - 1) / 2
    ax = np.arange(width)
    rho = np.hypot((ax - c)[:, None], (ax - c)[None, :]) / radius
    inside = (rho >= oc) & (rho < 1)
    return (~inside if inverse else inside).astype(int)


def crop(arr, center, size):
    """arr[center - size:center + size] along the first two axes (psfrec.py:629-632)."""
    lo, hi = int(center) - int(size), int(center) + int(size)
    return arr[lo:hi, lo:hi]


def interpolate(arr, xout, method='linear'):
    """Bilinear sampling of the square image `arr` (sample (i, j) at integer coordinates) at the points
    xout[0], xout[1] (psfrec.py:635-641: scipy's interpn on (arange(n), arange(n)), here in NumPy).  Points
    outside the grid raise ValueError as interpn does; 'cubic' raises NotImplementedError as the reference."""
    if method == 'cubic':
        raise NotImplementedError('FIXME: use gridddata or spline ?')
    if method != 'linear':
        raise ValueError('method must be linear')
    arr = np.asarray(arr)
    n = arr.shape[0]
    if arr.ndim != 2 or arr.shape[1] != n:
        raise ValueError('There are %d points and %d values in dimension 1' % (n, arr.shape[-1]))
    pts = np.asarray(xout, dtype=float).T
    if pts.shape[-1] != 2:
        raise ValueError('The requested sample points xi have dimension %d but this RegularGridInterpolator '
                         'has dimension 2' % pts.shape[-1])
    x, y = pts[..., 0], pts[..., 1]
    for d, v in enumerate((x, y)):
        if not np.logical_and(v >= 0, v <= n - 1).all():
            raise ValueError('One of the requested xi is out of bounds in dimension %d' % d)
    i = np.clip(np.floor(x).astype(int), 0, max(n - 2, 0))
    j = np.clip(np.floor(y).astype(int), 0, max(n - 2, 0))
    i1, j1 = np.minimum(i + 1, n - 1), np.minimum(j + 1, n - 1)
    wx, wy = x - i, y - j
    out = (arr[i, j] * (1 - wx) * (1 - wy) + arr[i1, j] * wx * (1 - wy) +
           arr[i, j1] * (1 - wx) * wy + arr[i1, j1] * wx * wy)
    return out.T


def psd_to_psf(psd, pup, D, lbda, phase_static=None, samp=None, FoV=None, return_all=False, *,
               precision='mixed', device=0):
    """PSF of a residual phase PSD and a pupil (psfrec.py:689-807), on the GPU in fp64 whatever `precision`
    (which only selects the cached context).

    psd   : (dim, dim) PSD, centred, in nm^2 m^2 at the PSF wavelength; or (npsd, dim, dim)
    pup   : (npup, npup) pupil, any real values (apodisation, spiders, segment gaps)
    D     : pupil diameter [m]
    lbda  : PSF wavelength [m], a scalar or a 1-D array
    phase_static : (npup, npup) static phase or None.  It is used as the reference's code uses it,
            exp(2 pi i phase_static / lbda) with lbda in metres, so it is in METRES (the reference's
            docstring says nm).
    samp  : output sampling (pixels per diffraction element); None means dim / npup.  (The reference
            raises TypeError for None.)
    FoV   : PSF field [arcsec]; only the reference's numerical field FoVnum is supported.

    Returns the (dimnum, dimnum) PSF of sum 1, dimnum = int(fix(dim samp / sampnum / 2)) 2, with the
    leading axes (npsd, nl) of a PSD stack and of a wavelength array; with `return_all`,
    (psf, sampout, FoV) as psfrec.py:803-805.
    Refused before any GPU work: FoV != FoVnum (NotImplementedError, as the reference's cubic
    interpolation), samp > dim / npup (ValueError; the reference fails with TypeError), a phase_static
    of another shape than pup (ValueError), a grid or dimnum without a planned transform (ValueError).
    """
    psd = np.asarray(psd, dtype=float)
    pup = np.asarray(pup, dtype=float)
    if psd.ndim not in (2, 3) or psd.shape[-1] != psd.shape[-2]:
        raise ValueError('psd must be (dim, dim) or (npsd, dim, dim)')
    if pup.ndim != 2 or pup.shape[0] != pup.shape[1]:
        raise ValueError('pup must be a square 2-D array')
    lb = np.asarray(lbda, dtype=float)
    if lb.ndim > 1:
        raise ValueError('lbda must be a scalar or a 1-D array')
    dim = psd.shape[-1]
    npup = pup.shape[0]
    sampnum = dim / npup
    if dim < 2 * npup:
        logger.info("the PSD horizon must be at least two time larger than "
                    "the pupil diameter")
    sampin = sampnum if samp is None else samp
    if sampin < 2:
        logger.info('PSF should be at least nyquist sampled')
    dimnum = int(np.fix(dim * (sampin / sampnum) / 2)) * 2
    sampout = dimnum / npup
    if sampin > sampnum:
        raise ValueError('samp=%g > dim / npup = %g: the PSD would have to be extrapolated; '
                         'use a larger PSD' % (sampin, sampnum))
    logger.debug('input sampling: %.2f, output sampling: %.2f, max num sampling: %.2f',
                 sampin, sampout, sampnum)
    FoVnum = (lb / (sampnum * D)) * dim / (4.85 * 1.e-6)
    if FoV is None:
        FoV = FoVnum
    if not np.allclose(FoV, FoVnum):
        raise NotImplementedError('FIXME: use gridddata or spline ?')
    if phase_static is not None:
        phase_static = np.asarray(phase_static, dtype=float)
        if phase_static.shape != pup.shape:
            logger.info("pup and static phase must have the same number of pixels")
            raise ValueError('phase_static must have the shape of pup %s, not %s'
                             % (pup.shape, phase_static.shape))
    if logger.isEnabledFor(logging.DEBUG):
        for fv, fn in zip(np.broadcast_to(FoV, lb.shape).ravel(), FoVnum.ravel()):
            logger.debug('input FoV: %.2f, output FoV: %.2f, Num FoV: %.2f', fv, fn, fn)
    if dim not in _P2P_SIZES:
        raise ValueError('grid dim=%d not supported %s' % (dim, _P2P_SIZES))
    if dimnum not in _P2P_SIZES or dimnum < npup:
        raise ValueError('dimnum=%d not supported (one of %s, and >= npup=%d)' % (dimnum, _P2P_SIZES, npup))
    ctx = get_context(dim, 0.2, 40, precision, device)
    out = ctx.psd_to_psf(psd, pup, D, lb.ravel(), phase_static=phase_static, dimnum=dimnum)
    if psd.ndim == 2:
        out = out[0]
    if lb.ndim == 0:
        out = out[..., 0, :, :]
    if return_all:
        return out, sampout, FoVnum * dimnum / dim
    return out


def convolve_final_psf(lbda, seeing, GL, L0, psf, *, pixscale=0.2, precision='mixed', device=0):
    """Convolve with the tip-tilt and MUSE PSFs to get the final PSF (psfrec.py:874-930).  `psf`:
    (nl, 40, 40)."""
    psf = np.asarray(psf, dtype=float)
    ctx = get_context(128, pixscale, psf.shape[-1], precision, device)
    return ctx.convolve_stamps(lbda, seeing, GL, L0, psf)


def compute_psf(lbda, seeing, GL, L0, npsflin=1, h=(100, 10000), three_lgs_mode=False,
                verbose=True, *, dim=1280, dimpsf=40, pixscale=0.2, precision='mixed',
                cutoff_masks='host', device=0, metrics=None):
    """Reconstruct a PSF from a set of seeing, GL, and L0 values (psfrec.py:933-978).

    Returns ``(table, psf)``: the per-wavelength Moffat fit table (with SEEING, GL, L0 columns and
    meta) and the (nl, 40, 40) float64 PSF cube.  ``metrics``: None (the table above), True or a
    dict(radii=, boxes=, fractions=, center=) (see psf_metrics): the columns ee, sqe, r_ee of ``psf`` follow."""
    mreq = _metrics_request(metrics, pixscale, dimpsf)
    lbda = np.atleast_1d(np.asarray(lbda, dtype=float))
    if verbose:
        logger.info('Compute PSF with seeing=%.2f GL=%.2f L0=%.2f', seeing, GL, L0)
        if three_lgs_mode:
            logger.info('Using three lasers mode')
    r = _reconstruct(lbda, [(seeing, GL, L0, three_lgs_mode)], npsflin, h, dim, dimpsf, pixscale,
                     precision, cutoff_masks, device)
    cols = _fit_columns(lbda, r['fit'][0], pixscale)
    nl = lbda.size
    cols['SEEING'] = np.full(nl, float(seeing))
    cols['GL'] = np.full(nl, float(GL))
    cols['L0'] = np.full(nl, float(L0))
    if mreq is not None:
        _append_metrics(cols, r['psf'][0], mreq, get_context(dim, pixscale, dimpsf, precision, r['devices'][0]),
                        pixscale)
    res = _make_table(cols, {'SEEING': float(seeing), 'GL': float(GL), 'L0': float(L0)})
    return res, r['psf'][0]


def _field_columns(lbda, pos, fit, pixscale, columns=None):
    """Columns of a field fit table from fit rows (npos, nl, NFIT): rows ordered (position, wavelength);
    dir_idx (0-based index into `pos`), x, y (arcsec), then the columns of _fit_columns (lbda first), or of
    `columns` (_fit_columns_ell for elliptical fit rows)."""
    pos = np.asarray(pos, dtype=float)
    lbda = np.asarray(lbda, dtype=float)
    npos, nl = pos.shape[0], lbda.size
    fit = np.asarray(fit).reshape(npos * nl, -1)
    cols = OrderedDict()
    cols['dir_idx'] = np.repeat(np.arange(npos), nl)
    cols['x'] = np.repeat(pos[:, 0], nl)
    cols['y'] = np.repeat(pos[:, 1], nl)
    cols.update((columns or _fit_columns)(np.tile(lbda, npos), fit, pixscale))
    return cols


def _field_request(positions, npsflin):
    """The positions of a field call: direction_perf(npsflin) as (npos, 2) when `positions` is None, else the
    caller's, validated (any number of them: calls of at most 25 are made)."""
    if positions is None:
        return np.ascontiguousarray(direction_perf(_args.grid_side(npsflin)).T)
    return _lib.field_positions(positions, max_n=None)


def _field_groups(npos):
    """Position ranges of the library calls a field request is split into (at most 25 positions each)."""
    m = _lib.MAX_FIELD_POSITIONS
    return [(a, min(a + m, npos)) for a in range(0, npos, m)]


def compute_field_psf(lbda, seeing, GL, L0, positions=None, npsflin=1, h=(100, 10000), three_lgs_mode=False,
                      verbose=True, *, dim=1280, dimpsf=40, pixscale=0.2, precision='mixed',
                      cutoff_masks='host', device=0, circular=True, metrics=None):
    """Field-resolved form of compute_psf: the PSF at every field position instead of their mean.

    ``positions``: (npos, 2) array of (x, y) in arcsec (|x|, |y| <= 60, the convention of direction_perf:
    x = dirperf[0]); None = direction_perf(npsflin).  Stamp (p, l) is what compute_psf returns for a PSD of the
    single direction p: psf_muse, convolve_final_psf, Moffat fit -- nothing is averaged over positions.

    Returns ``(table, psf)``: ``psf`` (npos, nl, dimpsf, dimpsf) float64; ``table`` npos x nl rows ordered
    (position, wavelength) with the columns dir_idx (0-based), x, y, lbda, the fit columns of compute_psf and
    SEEING, GL, L0 (values in the meta too).  circular=False: the fit columns are those of an elliptical Moffat
    fitted to ``psf`` (fit_psf_cube(..., circular=False)); ``psf`` is the same.  ``metrics``: as compute_psf -- the
    columns ee, sqe, r_ee of every stamp, row for row with the fit columns."""
    circular = _check_circular(circular)
    mreq = _metrics_request(metrics, pixscale, dimpsf)
    lbda = np.atleast_1d(np.asarray(lbda, dtype=float))
    if lbda.ndim != 1 or lbda.size < 1 or not np.all(np.isfinite(lbda)) or np.any(lbda <= 0):
        raise ValueError('lbda must be a non-empty 1-D array of positive wavelengths (nm)')
    seeing, GL, L0 = _two_layer_atmosphere(seeing, GL, L0, h)
    _check_precision(precision)
    pos = _field_request(positions, npsflin)
    masks = _resolve_masks(cutoff_masks)
    if verbose:
        logger.info('Compute field PSF at %d positions with seeing=%.2f GL=%.2f L0=%.2f', len(pos), seeing, GL, L0)
        if three_lgs_mode:
            logger.info('Using three lasers mode')
    ctx = get_context(dim, pixscale, dimpsf, precision, device)
    nl = lbda.size
    psf = np.empty((len(pos), nl, dimpsf, dimpsf))
    fit = np.empty((len(pos), nl, _lib.NFIT))
    try:
        for a, b in _field_groups(len(pos)):
            r = ctx.reconstruct_field(lbda, [seeing], [GL], [L0], [1 if three_lgs_mode else 0], h, pos[a:b],
                                      masks=masks, want_sum=False)
            psf[a:b] = r['psf'][0]
            fit[a:b] = r['fit'][0]
    except MpsfrError as e:
        if e.code == E_GRID:
            raise ValueError(str(e)) from None
        raise
    if circular:
        cols = _field_columns(lbda, pos, fit, pixscale)
    else:
        cols = _field_columns(lbda, pos, ctx.fit_stamps_elliptical(psf), pixscale, _fit_columns_ell)
    n = len(pos) * nl
    cols['SEEING'] = np.full(n, seeing)
    cols['GL'] = np.full(n, GL)
    cols['L0'] = np.full(n, L0)
    if mreq is not None:
        _append_metrics(cols, psf, mreq, ctx, pixscale)
    return _make_table(cols, {'SEEING': seeing, 'GL': GL, 'L0': L0}), psf


def _hat_integrals(lb, tfun, breaks):
    """w_l = int phi_l(x) T(x) dx over the grid lb, with phi_l the hat function of node l (1 at lb[l], 0 at its
    neighbours) and T linear between consecutive `breaks` (its own nodes, where it may also jump).  Each piece between
    two consecutive points of lb + breaks is integrated exactly (Simpson on a product of two linear functions); T is
    evaluated inside the piece only, so a jump at a break is one-sided on either side."""
    inner = np.asarray(breaks, dtype=float)
    pts = np.union1d(lb, inner[(inner > lb[0]) & (inner < lb[-1])])
    a, b = pts[:-1], pts[1:]
    k = np.searchsorted(lb, a, side='right') - 1          # the grid interval of each piece
    d = lb[k + 1] - lb[k]
    t1, t2 = tfun(a + (b - a) / 3), tfun(a + 2 * (b - a) / 3)
    ta, tb, tm = 2 * t1 - t2, 2 * t2 - t1, (t1 + t2) / 2
    ua, ub = (a - lb[k]) / d, (b - lb[k]) / d             # the hat of node k + 1 on the piece
    h = (b - a) / 6
    right = h * (ua * ta + 2 * (ua + ub) * tm + ub * tb)
    total = h * (ta + 4 * tm + tb)
    w = np.zeros(lb.size)
    np.add.at(w, k, total - right)
    np.add.at(w, k + 1, right)
    return w


def _curve(pair, what):
    """(wave_nm, values) of a throughput curve or an SED: 1-D, equal lengths >= 2, finite, wave strictly increasing,
    values >= 0."""
    try:
        x = np.asarray(pair[0], dtype=float)
        y = np.asarray(pair[1], dtype=float)
    except (TypeError, ValueError, IndexError):
        raise ValueError('%s must be a (wave_nm, values) pair of arrays' % what) from None
    if x.ndim != 1 or y.shape != x.shape or x.size < 2:
        raise ValueError('%s must be two 1-D arrays of equal length >= 2' % what)
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        raise ValueError('%s must be finite' % what)
    if np.any(np.diff(x) <= 0):
        raise ValueError('the wavelengths of %s must be strictly increasing' % what)
    if np.any(y < 0):
        raise ValueError('%s must not be negative' % what)
    return x, y


def band_weights(lbda, bands, sed=None):
    """Quadrature weights (nband, nl) of band-integrated PSFs on the wavelength grid ``lbda`` (nm, strictly
    increasing, at least two nodes).  Normalised per band (as the library does), they give the PSF of a cube in
    f_lambda units integrated over the band, int T f PSF dlambda / int T f dlambda, with T_b the throughput of band b
    and f the source's f_lambda:

        w_bl = f(lbda_l) int T_b(lambda) phi_l(lambda) dlambda

    where phi_l is the hat function of node l (1 at lbda_l, falling linearly to 0 at its neighbours): the integral of
    T_b times the PSF interpolated linearly between the grid's wavelengths, evaluated exactly.  Only where a band has
    throughput does it give weight: a grid interval outside the band (a gap between two bands on a union grid, say)
    contributes nothing.  Where T_b is constant over the intervals round a node this is the trapezoid rule D_l T_b(lbda_l)
    (D_l the trapezoid weights of the grid): a top-hat over the whole grid gives exactly the trapezoid weights, and a
    top-hat whose edges lie on nodes gives the trapezoid weights of the band's own nodes (its edge nodes half an
    interval).  An edge between two nodes shares its interval between them linearly, so lbda_min / lbda_max (the nodes
    with weight) may then lie just outside (lo, hi).

    ``bands``: a sequence of bands (or one band), each either a top-hat ``(lo, hi)`` in nm (T = 1 on [lo, hi]) or a
    curve ``(wave_nm, throughput)`` (linear interpolation, zero outside its range).  ``sed``: None (a flat f_lambda) or
    ``(wave_nm, f_lambda)``, linearly interpolated; it must cover every grid node where a band has weight.
    Raises ValueError for a grid that is not strictly increasing, a band without weight on the grid, negative values
    and an SED that does not cover a band."""
    lb = np.atleast_1d(np.asarray(lbda, dtype=float))
    if lb.ndim != 1 or lb.size < 2 or not np.all(np.isfinite(lb)) or np.any(lb <= 0):
        raise ValueError('lbda must be a 1-D array of at least two positive wavelengths (nm)')
    if np.any(np.diff(lb) <= 0):
        raise ValueError('lbda must be strictly increasing')
    if isinstance(bands, (str, bytes)):
        raise ValueError('bands must be (lo, hi) pairs or (wave_nm, throughput) curves')
    try:
        bands = list(bands)
    except TypeError:
        raise ValueError('bands must be (lo, hi) pairs or (wave_nm, throughput) curves') from None
    if len(bands) == 2 and all(np.ndim(b) == 0 for b in bands):
        bands = [tuple(bands)]                       # (one top-hat)
    if not bands:
        raise ValueError('need at least one band')
    rows = []
    for k, b in enumerate(bands):
        try:
            ok = len(b) == 2
        except TypeError:
            ok = False
        if not ok:
            raise ValueError('band %d must be (lo, hi) or (wave_nm, throughput)' % k)
        if np.ndim(b[0]) == 0 and np.ndim(b[1]) == 0:
            try:
                lo, hi = float(b[0]), float(b[1])
            except (TypeError, ValueError):
                raise ValueError('band %d: (lo, hi) must be numbers' % k) from None
            if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo < hi):
                raise ValueError('band %d: need finite 0 <= lo < hi, got (%g, %g)' % (k, lo, hi))
            rows.append(_hat_integrals(lb, lambda v, lo=lo, hi=hi: ((v >= lo) & (v <= hi)).astype(float), [lo, hi]))
        else:
            x, y = _curve(b, 'band %d' % k)
            rows.append(_hat_integrals(lb, lambda v, x=x, y=y: np.interp(v, x, y, left=0.0, right=0.0), x))
    w = np.array(rows)
    if sed is not None:
        x, f = _curve(sed, 'sed')
        for k in range(len(w)):
            nodes = lb[w[k] > 0]
            if nodes.size and (nodes[0] < x[0] or nodes[-1] > x[-1]):
                raise ValueError('sed does not cover band %d (%g..%g nm)' % (k, nodes[0], nodes[-1]))
        w = w * np.interp(lb, x, f)[None, :]
    for k in range(len(w)):
        if not w[k].sum() > 0:
            raise ValueError('band %d has no weight on the wavelength grid' % k)
    return w


def _band_columns(lbda, w):
    """lbda_eff (sum of the normalised weights x lbda), lbda_min / lbda_max (of the nodes with weight) per band."""
    w = np.asarray(w, dtype=float)
    lbda = np.asarray(lbda, dtype=float)
    wn = w / w.sum(axis=1, keepdims=True)
    eff = wn @ lbda
    lo = np.array([lbda[r > 0].min() for r in w])
    hi = np.array([lbda[r > 0].max() for r in w])
    return eff, lo, hi


def _band_table_columns(lbda, w, fit, pixscale, circular, pos=None):
    """Columns of a band fit table from fit rows ((npos,) nband, NFIT or NFIT_ELL): rows ordered (position,) band;
    band (0-based), (dir_idx, x, y,) lbda_eff, lbda_min, lbda_max, then the fit columns of compute_psf (or of
    fit_psf_cube(circular=False)) without lbda."""
    eff, lo, hi = _band_columns(lbda, w)
    nb = len(eff)
    npos = 1 if pos is None else len(pos)
    fit = np.asarray(fit).reshape(npos * nb, -1)
    fc = (_fit_columns if circular else _fit_columns_ell)(np.tile(eff, npos), fit, pixscale)
    cols = OrderedDict()
    cols['band'] = np.tile(np.arange(nb), npos)
    if pos is not None:
        pos = np.asarray(pos, dtype=float)
        cols['dir_idx'] = np.repeat(np.arange(npos), nb)
        cols['x'] = np.repeat(pos[:, 0], nb)
        cols['y'] = np.repeat(pos[:, 1], nb)
    cols['lbda_eff'] = np.tile(eff, npos)
    cols['lbda_min'] = np.tile(lo, npos)
    cols['lbda_max'] = np.tile(hi, npos)
    for k, v in fc.items():
        if k != 'lbda':
            cols[k] = v
    return cols


def _band_groups(nband):
    m = _lib.MAX_BANDS
    return [(a, min(a + m, nband)) for a in range(0, nband, m)]


def compute_band_psf(lbda, seeing, GL, L0, bands, sed=None, npsflin=1, positions=None, h=(100, 10000),
                     three_lgs_mode=False, verbose=True, *, dim=1280, dimpsf=40, pixscale=0.2, precision='mixed',
                     cutoff_masks='host', device=0, circular=True, metrics=None):
    """Band-integrated form of compute_psf: the PSF of a broadband image, the spectrum-weighted mean of the
    monochromatic PSFs over each band (band_weights(lbda, bands, sed) on the grid ``lbda``), reduced and fitted on the
    GPU -- not the PSF at the band's central wavelength.

    positions=None: the npsflin directions averaged, ``psf`` (nband, dimpsf, dimpsf); else (npos, 2) arcsec as in
    compute_field_psf, ``psf`` (npos, nband, dimpsf, dimpsf).  Returns ``(table, psf)``; the table has one row per
    (position,) band with the columns band (0-based), (dir_idx, x, y,) lbda_eff (the weighted mean wavelength),
    lbda_min, lbda_max (the band's nodes with weight), the fit columns of compute_psf and SEEING, GL, L0.
    circular=False: the fit columns are those of an elliptical Moffat fitted to ``psf`` (fit_psf_cube(...,
    circular=False)); ``psf`` is the same.  ``metrics``: as compute_psf -- the columns ee, sqe, r_ee of every band stamp.
    Every refusal is a ValueError, raised before any GPU context exists."""
    circular = _check_circular(circular)
    mreq = _metrics_request(metrics, pixscale, dimpsf)
    lbda = np.atleast_1d(np.asarray(lbda, dtype=float))
    w = band_weights(lbda, bands, sed)
    seeing, GL, L0 = _two_layer_atmosphere(seeing, GL, L0, h)
    _check_precision(precision)
    pos = _grid_or_field(npsflin, positions)
    masks = _resolve_masks(cutoff_masks)
    if verbose:
        logger.info('Compute band PSF for %d band(s) with seeing=%.2f GL=%.2f L0=%.2f', len(w), seeing, GL, L0)
        if three_lgs_mode:
            logger.info('Using three lasers mode')
    ctx = get_context(dim, pixscale, dimpsf, precision, device)
    nb = len(w)
    npos = 1 if pos is None else len(pos)
    psf = np.empty((npos, nb, dimpsf, dimpsf))
    fit = np.empty((npos, nb, _lib.NFIT))
    rows = ([seeing], [GL], [L0], [1 if three_lgs_mode else 0], h)
    try:
        for ba, bb in _band_groups(nb):
            a_ = (lbda, w[ba:bb]) + rows
            if pos is None:
                r = ctx.reconstruct_band(*a_, npsflin=npsflin, masks=masks, want_sum=False)
                psf[0, ba:bb] = r['psf'][0]
                fit[0, ba:bb] = r['fit'][0]
            else:
                for a, b in _field_groups(npos):
                    r = ctx.reconstruct_band(*a_, npsflin=0, positions=pos[a:b], masks=masks, want_sum=False)
                    psf[a:b, ba:bb] = r['psf'][0]
                    fit[a:b, ba:bb] = r['fit'][0]
    except MpsfrError as e:
        if e.code == E_GRID:
            raise ValueError(str(e)) from None
        raise
    if not circular:
        fit = ctx.fit_stamps_elliptical(psf).reshape(npos, nb, -1)
    cols = _band_table_columns(lbda, w, fit, pixscale, circular, pos)
    n = len(cols['band'])
    cols['SEEING'] = np.full(n, seeing)
    cols['GL'] = np.full(n, GL)
    cols['L0'] = np.full(n, L0)
    if mreq is not None:
        _append_metrics(cols, psf, mreq, ctx, pixscale)
    if pos is None:
        psf = psf[0]
    return _make_table(cols, {'SEEING': seeing, 'GL': GL, 'L0': L0}), psf


def compute_profile_psf(lbda, seeing, L0, cn2, h, wind_speed=12.5, wind_dir=None, GL=None, npsflin=1, positions=None,
                        three_lgs_mode=False, verbose=True, *, dim=1280, dimpsf=40, pixscale=0.2, precision='mixed',
                        cutoff_masks='host', device=0, circular=True, metrics=None):
    """compute_psf / compute_field_psf for a Cn2 profile instead of the fixed two-layer atmosphere.

    ``cn2``, ``h``, ``wind_speed``, ``wind_dir``: the layers' weights (normalised here, psfrec.py:57-58), altitudes
    [m, 0..50000], wind speeds [m/s, 0..100; a scalar applies to every layer] and directions [rad] -- the
    reference's Cn2, hh, vent and arg_v of dsp4muse (psfrec.py:531-613), 1 to 8 layers.  ``wind_dir`` may be
    omitted for two layers only: the reference's directions (0.628163, -0.326497).  ``GL`` only sets the tip-tilt
    kernel (psfrec.py:881-883); by default it is the normalised weight of the lowest layer, so cn2=[GL, 1 - GL]
    with h=(100, 10000) is what compute_psf means by GL.

    positions=None: ``(table, psf)`` as compute_psf (the npsflin directions averaged, psf (nl, dimpsf, dimpsf));
    else (npos, 2) arcsec: as compute_field_psf (psf (npos, nl, dimpsf, dimpsf), table with dir_idx, x, y).
    circular=False: the fit columns are those of an elliptical Moffat fitted to ``psf`` (fit_psf_cube(...,
    circular=False)); ``psf`` is the same.  ``metrics``: as compute_psf -- the columns ee, sqe, r_ee of every stamp.
    Every refusal is a ValueError, raised before any GPU context exists."""
    circular = _check_circular(circular)
    mreq = _metrics_request(metrics, pixscale, dimpsf)
    lbda = np.atleast_1d(np.asarray(lbda, dtype=float))
    if lbda.ndim != 1 or lbda.size < 1 or not np.all(np.isfinite(lbda)) or np.any(lbda <= 0):
        raise ValueError('lbda must be a non-empty 1-D array of positive wavelengths (nm)')
    try:
        seeing, L0 = float(seeing), float(L0)
    except (TypeError, ValueError):
        raise ValueError('seeing and L0 must be scalars') from None
    if not (seeing > 0 and L0 > 0):
        raise ValueError('need seeing > 0 and L0 > 0')
    if wind_dir is None:
        if np.size(h) != 2:
            raise ValueError('wind_dir may only be omitted for two layers (the reference\'s directions)')
        wind_dir = _lib.REF_WIND_DIR
    hh, ws, wd = _lib.profile_layers(h, wind_speed, wind_dir)
    if np.ndim(cn2) != 1:
        raise ValueError('cn2 must be one weight per layer')
    w = _lib.profile_weights(cn2, 1, hh.size)[0]
    if GL is None:
        GL = float(w[np.argmin(hh)] / w.sum())
    try:
        GL = float(GL)
    except (TypeError, ValueError):
        raise ValueError('GL must be a scalar') from None
    if not 0 <= GL <= 1:
        raise ValueError('need 0 <= GL <= 1')
    _check_precision(precision)
    pos = _grid_or_field(npsflin, positions)
    masks = _resolve_masks(cutoff_masks)
    if verbose:
        logger.info('Compute PSF for a %d-layer profile with seeing=%.2f L0=%.2f', hh.size, seeing, L0)
        if three_lgs_mode:
            logger.info('Using three lasers mode')
    ctx = get_context(dim, pixscale, dimpsf, precision, device)
    nl = lbda.size
    args = (lbda, [seeing], [GL], [L0], w, hh, ws, wd, [1 if three_lgs_mode else 0])
    try:
        if pos is None:
            r = ctx.reconstruct_profile(*args, npsflin=npsflin, masks=masks, want_sum=False)
            psf, fit = r['psf'][0], r['fit'][0]
            cols = (_fit_columns(lbda, fit, pixscale) if circular else
                    _fit_columns_ell(lbda, ctx.fit_stamps_elliptical(psf), pixscale))
        else:
            psf = np.empty((len(pos), nl, dimpsf, dimpsf))
            fit = np.empty((len(pos), nl, _lib.NFIT))
            for a, b in _field_groups(len(pos)):
                r = ctx.reconstruct_profile(*args, npsflin=0, positions=pos[a:b], masks=masks, want_sum=False)
                psf[a:b] = r['psf'][0]
                fit[a:b] = r['fit'][0]
            cols = (_field_columns(lbda, pos, fit, pixscale) if circular else
                    _field_columns(lbda, pos, ctx.fit_stamps_elliptical(psf), pixscale, _fit_columns_ell))
    except MpsfrError as e:
        if e.code == E_GRID:
            raise ValueError(str(e)) from None
        raise
    n = len(cols['lbda'])
    cols['SEEING'] = np.full(n, seeing)
    cols['GL'] = np.full(n, GL)
    cols['L0'] = np.full(n, L0)
    if mreq is not None:
        _append_metrics(cols, psf, mreq, ctx, pixscale)
    return _make_table(cols, {'SEEING': seeing, 'GL': GL, 'L0': L0, 'NLAYER': int(hh.size)}), psf


def _field_sum(lbda, stats, three, pos, h, dim, dimpsf, pixscale, precision, cutoff_masks, devs):
    """Sum over the rows of the field stamps (npos, nl, dimpsf, dimpsf): the rows in contiguous balanced shards over
    `devs` (as mpsfr_reconstruct_multi deals them), the positions in groups of at most 25, every (shard, group) an
    asynchronous sums-only call on its context; the shards' sums are added in device order."""
    ntask = len(stats)
    masks = _resolve_masks(cutoff_masks)
    nctx = len(devs) if ntask >= len(devs) else 1
    bounds = [0]
    for k in range(nctx):
        bounds.append(bounds[-1] + ntask // nctx + (1 if k < ntask % nctx else 0))
    replica = [devs[:i].count(d) for i, d in enumerate(devs)]
    ctxs = [get_context(dim, pixscale, dimpsf, precision, d, r) for d, r in zip(devs[:nctx], replica[:nctx])]
    see, gl, l0 = (np.ascontiguousarray(stats[:, k], dtype=float) for k in range(3))
    t3 = np.asarray(three).astype(np.uint8)
    pend = []
    try:
        for k, ctx in enumerate(ctxs):
            a, b = bounds[k], bounds[k + 1]
            pend.append([ctx.reconstruct_field_async(lbda, see[a:b], gl[a:b], l0[a:b], t3[a:b], h, pos[p:q],
                                                     masks=masks, want_psf=False, want_fit=False)
                         for p, q in _field_groups(len(pos))])
        total = np.empty((len(pos), lbda.size, dimpsf, dimpsf))
        for k, parts in enumerate(pend):
            for (p, q), part in zip(_field_groups(len(pos)), parts):
                s = part.wait()['psf_sum']
                total[p:q] = s if k == 0 else total[p:q] + s
    except BaseException as e:
        for ctx in ctxs:
            ctx.abandon()
        if isinstance(e, MpsfrError) and e.code == E_GRID:
            raise ValueError(str(e)) from None
        raise
    return total


def _band_rows(lbda, w, stats, three, npsflin, h, dim, dimpsf, pixscale, precision, cutoff_masks, devs):
    """Band fits of every row (ntask, nband, NFIT) and the sum of the band stamps over the rows (nband, dimpsf,
    dimpsf): the rows in contiguous balanced shards over `devs` (as _field_sum deals them), the bands in groups of at
    most MAX_BANDS, every (shard, group) an asynchronous band call without stamps; the shards' sums are added in
    device order."""
    ntask, nb = len(stats), len(w)
    masks = _resolve_masks(cutoff_masks)
    nctx = len(devs) if ntask >= len(devs) else 1
    bounds = [0]
    for k in range(nctx):
        bounds.append(bounds[-1] + ntask // nctx + (1 if k < ntask % nctx else 0))
    replica = [devs[:i].count(d) for i, d in enumerate(devs)]
    ctxs = [get_context(dim, pixscale, dimpsf, precision, d, r) for d, r in zip(devs[:nctx], replica[:nctx])]
    see, gl, l0 = (np.ascontiguousarray(stats[:, k], dtype=float) for k in range(3))
    t3 = np.asarray(three).astype(np.uint8)
    pend = []
    try:
        for k, ctx in enumerate(ctxs):
            a, b = bounds[k], bounds[k + 1]
            pend.append([ctx.reconstruct_band_async(lbda, w[p:q], see[a:b], gl[a:b], l0[a:b], t3[a:b], h,
                                                    npsflin=npsflin, masks=masks, want_psf=False)
                         for p, q in _band_groups(nb)])
        fit = np.empty((ntask, nb, _lib.NFIT))
        total = np.empty((nb, dimpsf, dimpsf))
        for k, parts in enumerate(pend):
            a, b = bounds[k], bounds[k + 1]
            for (p, q), part in zip(_band_groups(nb), parts):
                r = part.wait()
                fit[a:b, p:q] = r['fit']
                total[p:q] = r['psf_sum'] if k == 0 else total[p:q] + r['psf_sum']
    except BaseException as e:
        for ctx in ctxs:
            ctx.abandon()
        if isinstance(e, MpsfrError) and e.code == E_GRID:
            raise ValueError(str(e)) from None
        raise
    return fit, total


def _table_hdu(cols, meta, name):
    fits, ATable = _astropy()
    if fits is not None:
        t = ATable(cols)
        t.meta.update(meta)
        hdu = fits.table_to_hdu(t)
        hdu.name = name
        return hdu
    hdr = _minifits.Header()
    for k, v in meta.items():
        hdr[k] = v
    return _minifits.BinTableHDU.from_columns(cols, hdr, name)


def compute_psf_from_sparta(filename, extname='SPARTA_ATM_DATA', npsflin=1, lmin=490, lmax=930,
                            nl=35, lbda=None, h=(100, 10000), n_jobs=-1, plot=False,
                            mean_of_lgs=True, verbose=True, *, dim=1280, dimpsf=40, pixscale=0.2,
                            precision='mixed', cutoff_masks='host', device=None, devices=None,
                            field_positions=None, bands=None, band_sed=None, band_lbda=None, metrics=None):
    """Reconstruct a PSF from SPARTA data (psfrec.py:981-1120).

    ``filename`` is a FITS path or an already opened HDUList.  Returns an HDUList with
    PRIMARY, a copy of the SPARTA extension, FIT_ROWS, FIT_MEAN and PSF_MEAN -- or ``None``
    (with a 'No valid values' warning) when no row has a valid laser.  The rows are processed as one
    GPU batch -- or, like the reference's ``n_jobs`` worker processes (psfrec.py:1082-1083), as one
    batch per GPU: with ``device`` and ``devices`` both None every visible GPU is taken when the table
    has at least FANOUT_MIN_TASKS_PER_DEVICE tasks per device (``n_jobs`` = 1 keeps one device,
    ``n_jobs`` > 1 caps their number; a rank of a one-process-per-GPU launch keeps its own);
    ``device=k`` names the one device to use, ``devices=[...]`` several.  The per-row results do not
    depend on the split.

    ``field_positions``: None (the output above), ``'grid'`` (direction_perf(npsflin)) or an (n, 2) array of
    (x, y) in arcsec: then two HDUs follow PSF_MEAN -- PSF_FIELD, the (npos, nl, dimpsf, dimpsf) mean over the
    rows of the stamps at each position (compute_field_psf), and FIT_FIELD, the Moffat fit of each of them with
    dir_idx, x, y and lbda columns (meta: the median SEEING, GL, L0, like FIT_MEAN).

    ``bands`` (with ``band_sed``, see band_weights; ``band_lbda``: the wavelength grid of the bands, by default
    ``lbda``): three more HDUs follow -- FIT_BAND_ROWS, the Moffat fit of each row's band PSF (rows ordered (row,
    band), row_idx / lgs_idx as in FIT_ROWS), PSF_BAND, the (nband, dimpsf, dimpsf) mean over the rows of the band
    PSFs, and FIT_BAND, the fit of each PSF_BAND stamp (as FIT_MEAN is that of PSF_MEAN).  The rows use the devices
    of FIT_ROWS.

    ``metrics`` (None, True or a dict, see compute_psf and psf_metrics): the energy metrics of the mean stamps follow
    all other HDUs -- METRICS_MEAN (of PSF_MEAN, one row per wavelength: lbda, flux, peak, center, ee, sqe, r_ee,
    status), METRICS_FIELD (of PSF_FIELD: dir_idx, x, y, lbda, ...) and METRICS_BAND (of PSF_BAND: band, lbda_eff,
    ...) when those exist; radii, boxes and fractions are in their headers (MRADk, MBOXk, MFRACk; a single radius, box or
    fraction makes a scalar FITS column).  Per-row metrics of
    the SPARTA table are not computed here: Context.reconstruct_device chained into Context.stamp_metrics_device does
    that without downloading a stamp."""
    mreq = _metrics_request(metrics, pixscale, dimpsf)
    bw = blbda = None
    if bands is not None:
        blbda = band_lbda if band_lbda is not None else (lbda if lbda is not None else np.linspace(lmin, lmax, nl))
        blbda = np.atleast_1d(np.asarray(blbda, dtype=float))
        bw = band_weights(blbda, bands, band_sed)
    elif band_sed is not None or band_lbda is not None:
        raise ValueError('band_sed and band_lbda need bands')
    if field_positions is None:
        fpos = None
    elif isinstance(field_positions, str):
        if field_positions != 'grid':
            raise ValueError("field_positions must be None, 'grid' or an (n, 2) array of (x, y) in arcsec")
        fpos = _field_request(None, npsflin)
    else:
        fpos = _field_request(field_positions, npsflin)
    fits, _ = _astropy()
    io_mod = fits if fits is not None else _minifits
    opened = False
    if isinstance(filename, (list, _minifits.HDUList)) or (
            fits is not None and isinstance(filename, fits.HDUList)):
        hdul = filename
    else:
        hdul = io_mod.open(filename)
        opened = True
    try:
        ext = hdul[extname]
        data = np.array(ext.data)
        if fits is not None and isinstance(ext, fits.BinTableHDU):
            out = fits.HDUList([fits.PrimaryHDU(), ext.copy()])
        else:
            out = _minifits.HDUList([_minifits.PrimaryHDU(), ext.copy()])
    finally:
        if opened:
            hdul.close()

    nrows = len(data)
    if nrows == 1:
        n_jobs = 1
    if lbda is None:
        lbda = np.linspace(lmin, lmax, nl)
    lbda = np.atleast_1d(np.asarray(lbda, dtype=float))
    if verbose:
        logger.info('Processing SPARTA table with %d values, njobs=%d ...', nrows, n_jobs)

    # The rows are walked by NumPy, not by a Python loop (a 1000-row table spent as long in that loop
    # as on the GPU): values[row][laser] = (seeing, GL, L0), the outlier rejection of psfrec.py:1049-1051,
    # and the tasks in the reference's order -- rows ascending, lasers ascending inside a row.
    values = np.empty((nrows, 4, 3), dtype=float)
    for k in range(4):
        for j, col in enumerate(('SEEING', 'TUR_GND', 'L0')):
            values[:, k, j] = data['LGS%d_%s' % (k + 1, col)]
    ok = (values[:, :, 1] > 0) & (values[:, :, 2] < MAX_L0) & (values[:, :, 2] > MIN_L0)
    nb_gs = ok.sum(axis=1)
    if verbose:
        for irow in np.nonzero(nb_gs < 4)[0]:
            if nb_gs[irow] == 0:
                logger.info('%d/%d : No valid values, skipping this row', irow + 1, nrows)
            else:
                logger.info('%d/%d : Using only %d values out of 4 after outliers rejection',
                            irow + 1, nrows, nb_gs[irow])
    if mean_of_lgs:
        rows = np.nonzero(nb_gs > 0)[0]
        # the mean over the valid lasers, added in laser order like values[ok].mean(axis=0)
        stats = np.where(ok[rows][:, :, None], values[rows], 0.0).sum(axis=1) / nb_gs[rows][:, None]
        laser_idx = np.full(rows.size, -1)
    else:
        rows, las = np.nonzero(ok)
        stats = values[rows, las]
        laser_idx = las + 1
    three = nb_gs[rows] < 4
    to_compute = (stats, three)

    if len(stats) == 0:
        logger.warning('No valid values')
        return None

    if verbose:
        for (seeing, GL, L0), t3 in zip(stats, three):
            logger.info('Compute PSF with seeing=%.2f GL=%.2f L0=%.2f', seeing, GL, L0)
            if t3:
                logger.info('Using three lasers mode')

    ntask, nlam = len(stats), lbda.size
    devs = _fanout_devices(devices, device, ntask, n_jobs)
    if len(devs) == 1 and ntask >= 2 * PIPELINE_MIN_TASKS:
        # A large table on one device goes through the library as up to four asynchronous host-output
        # calls (mpsfr_reconstruct on_device = 2): the records of one part are assembled while the GPU
        # works on the next ones.  Per-task results do not depend on the split; the stamp sums of the
        # parts are added in order.
        r, rec = _reconstruct_pipelined(lbda, stats, three, laser_idx, npsflin, h, dim, dimpsf, pixscale, precision,
                                        cutoff_masks, devs[0])
        # (with astropy -- the reference's environment -- the same record array becomes an astropy table HDU)
        out.append(_minifits.BinTableHDU(rec, _minifits.Header(), 'FIT_ROWS') if fits is None
                   else fits.BinTableHDU(data=rec, name='FIT_ROWS'))
    else:
        r = _reconstruct(lbda, to_compute, npsflin, h, dim, dimpsf, pixscale, precision, cutoff_masks,
                         device, want_psf=False, devices=devices, n_jobs=n_jobs)

    # FIT_ROWS: the per-task tables stacked (psfrec.py:1086-1101)
    if 'rec' in r:
        pass
    elif fits is None:
        out.append(_minifits.BinTableHDU(_fit_rows_records(lbda, r['fit'], pixscale, stats, laser_idx),
                                         _minifits.Header(), 'FIT_ROWS'))
    else:
        cols = _fit_columns(np.tile(lbda, ntask), r['fit'].reshape(ntask * nlam, -1), pixscale)
        cols['SEEING'] = np.repeat(stats[:, 0], nlam)
        cols['GL'] = np.repeat(stats[:, 1], nlam)
        cols['L0'] = np.repeat(stats[:, 2], nlam)
        cols['row_idx'] = np.repeat(np.arange(1, ntask + 1), nlam)
        cols['lgs_idx'] = np.repeat(np.asarray(laser_idx), nlam)
        out.append(_table_hdu(cols, {}, 'FIT_ROWS'))

    # mean PSF over the tasks and its fit (psfrec.py:1104-1113)
    psftot = r['psf_sum'] / ntask
    ctx = get_context(dim, pixscale, dimpsf, precision, r.get('devices', [device or 0])[0])
    mcols = _fit_columns(lbda, ctx.fit_stamps(psftot), pixscale)
    seeing, GL, L0 = np.median(stats, axis=0)
    out.append(_table_hdu(mcols, {'SEEING': float(seeing), 'GL': float(GL), 'L0': float(L0)},
                          'FIT_MEAN'))
    if fits is not None and isinstance(out, fits.HDUList):
        out.append(fits.ImageHDU(data=psftot, name='PSF_MEAN'))
    else:
        out.append(_minifits.ImageHDU(data=psftot, name='PSF_MEAN'))

    if fpos is not None:
        # the field-resolved mean: the same rows, on the devices the batch ran on, sums only (psf_out = fit_out = NULL)
        devs = r.get('devices', [device or 0])
        psf_field = _field_sum(lbda, stats, three, fpos, h, dim, dimpsf, pixscale, precision, cutoff_masks,
                               devs) / ntask
        if fits is not None and isinstance(out, fits.HDUList):
            out.append(fits.ImageHDU(data=psf_field, name='PSF_FIELD'))
        else:
            out.append(_minifits.ImageHDU(data=psf_field, name='PSF_FIELD'))
        ffit = ctx.fit_stamps(psf_field.reshape(-1, dimpsf, dimpsf))
        out.append(_table_hdu(_field_columns(lbda, fpos, ffit, pixscale),
                              {'SEEING': float(seeing), 'GL': float(GL), 'L0': float(L0)}, 'FIT_FIELD'))

    if bw is not None:
        devs = r.get('devices', [device or 0])
        bfit, bsum = _band_rows(blbda, bw, stats, three, npsflin, h, dim, dimpsf, pixscale, precision, cutoff_masks,
                                devs)
        nb = len(bw)
        eff, lo, hi = _band_columns(blbda, bw)
        rcols = OrderedDict(band=np.tile(np.arange(nb), ntask), lbda_eff=np.tile(eff, ntask),
                            lbda_min=np.tile(lo, ntask), lbda_max=np.tile(hi, ntask))
        rcols.update((k, v) for k, v in _fit_columns(np.tile(eff, ntask), bfit.reshape(ntask * nb, -1),
                                                     pixscale).items() if k != 'lbda')
        rcols['SEEING'] = np.repeat(stats[:, 0], nb)
        rcols['GL'] = np.repeat(stats[:, 1], nb)
        rcols['L0'] = np.repeat(stats[:, 2], nb)
        rcols['row_idx'] = np.repeat(np.arange(1, ntask + 1), nb)
        rcols['lgs_idx'] = np.repeat(np.asarray(laser_idx), nb)
        out.append(_table_hdu(rcols, {}, 'FIT_BAND_ROWS'))
        psf_band = bsum / ntask
        if fits is not None and isinstance(out, fits.HDUList):
            out.append(fits.ImageHDU(data=psf_band, name='PSF_BAND'))
        else:
            out.append(_minifits.ImageHDU(data=psf_band, name='PSF_BAND'))
        out.append(_table_hdu(_band_table_columns(blbda, bw, ctx.fit_stamps(psf_band), pixscale, True),
                              {'SEEING': float(seeing), 'GL': float(GL), 'L0': float(L0)}, 'FIT_BAND'))

    if mreq is not None:
        med = {'SEEING': float(seeing), 'GL': float(GL), 'L0': float(L0)}
        out.append(_metrics_hdu(OrderedDict(lbda=lbda), psftot, mreq, ctx, pixscale, med, 'METRICS_MEAN'))
        if fpos is not None:
            lead = OrderedDict(dir_idx=np.repeat(np.arange(len(fpos)), nlam), x=np.repeat(fpos[:, 0], nlam),
                               y=np.repeat(fpos[:, 1], nlam), lbda=np.tile(lbda, len(fpos)))
            out.append(_metrics_hdu(lead, psf_field, mreq, ctx, pixscale, med, 'METRICS_FIELD'))
        if bw is not None:
            eff = _band_columns(blbda, bw)[0]
            lead = OrderedDict(band=np.arange(len(bw)), lbda_eff=eff)
            out.append(_metrics_hdu(lead, psf_band, mreq, ctx, pixscale, med, 'METRICS_BAND'))

    if plot:
        import matplotlib.pyplot as plt
        plot_psf(out, npsflin=npsflin)
        plt.show()
    return out


def create_sparta_table(nlines=1, seeing=1, L0=25, GL=0.7, bad_l0=False, outfile=None):
    """Helper to create a SPARTA table with the given seeing, L0, and GL values for the 4 LGS
    (psfrec.py:1123-1141).  Returns the table HDU named SPARTA_ATM_DATA."""
    cols = OrderedDict()
    for k in range(1, 5):
        for col, v in (('SEEING', seeing), ('TUR_GND', GL), ('L0', L0)):
            cols['LGS%d_%s' % (k, col)] = np.full(nlines, float(v))
    if bad_l0:
        cols['LGS4_L0'] = np.full(nlines, 150.0)
    hdu = _table_hdu(cols, {}, 'SPARTA_ATM_DATA')
    if outfile is not None:
        fits, _ = _astropy()
        if fits is not None:
            hdu.writeto(outfile, overwrite=True)
        else:
            _minifits.HDUList([_minifits.PrimaryHDU(), hdu]).writeto(outfile, overwrite=True)
    return hdu


def muse_intrinsic_psf(lbda):
    """MUSE PSF polynomial approximation (psfrec.py:1144-1171): fwhm, beta, fwhm_std, beta_std."""
    pol_beta = [-0.83704697, 1.1337153, 0.0609222, -1.35581762, 1.15237178, 2.2106042]
    pol_fwhm = [0.60467385, -1.58905792, 1.75293264, -1.0368302, 0.21487023, 0.34851139]
    pol_beta_std = [0.18187424, -0.17841793, 0.30962616]
    pol_fwhm_std = [0.00707504, -0.0303464, 0.04596354]
    lb = (10 * np.asarray(lbda, dtype=float) - 4750) / (9350 - 4750)
    return (np.polyval(pol_fwhm, lb), np.polyval(pol_beta, lb), np.polyval(pol_fwhm_std, lb),
            np.polyval(pol_beta_std, lb))


def fit_psf_with_polynom(lbda, fwhm, beta, deg=(5, 5), output=0):
    """Fit MUSE PSF fwhm and beta with polynoms (psfrec.py:1174-1215)."""
    def norm(x):
        return (np.asarray(x, dtype=float) - 475) / (935 - 475) - 0.5
    fwhm_pol = np.polyfit(norm(lbda), fwhm, deg[0])
    beta_pol = np.polyfit(norm(lbda), beta, deg[1])
    res = dict(fwhm_pol=fwhm_pol, beta_pol=beta_pol, lbda=lbda, lbda_lim=(475, 935))
    if output > 0:
        lbda_fit = np.linspace(475, 935, 50)
        res['lbda_fit'] = lbda_fit
        res['fwhm_fit'] = np.polyval(fwhm_pol, norm(lbda_fit))
        res['beta_fit'] = np.polyval(beta_pol, norm(lbda_fit))
    return res


def direction_perf(npts, field_size=60, plot=False, lgs=None, ngs=None, ax=None):
    """Grid of directions (arcsec) where the PSF is estimated (psfrec.py:154-180): (2, npts^2),
    (mgrid - npts // 2) * field_size / 2.  With ``plot`` the directions (and the guide stars, if
    given) are drawn on ``ax``."""
    gx, gy = (np.mgrid[:npts, :npts] - npts // 2) * field_size / 2
    dirperf = np.array([gx, gy]).reshape(2, -1)
    if plot:
        import matplotlib.pyplot as plt
        if ax is None:
            _, ax = plt.subplots()
        extent = np.max(dirperf)
        ax.scatter(dirperf[0], dirperf[1], marker='o', s=10, label='Reconstruction directions')
        for stars, size, label in ((lgs, 60, 'LGS'), (ngs, 40, 'NGS')):
            if stars is not None:
                extent = max(extent, np.max(stars))
                ax.scatter(stars[0], stars[1], marker='*', s=size, label=label)
        ax.set_xlim((-1.25 * extent, 1.25 * extent))
        ax.set_ylim((-1.25 * extent, 1.25 * extent))
        ax.set_xlabel('arcsecond')
        ax.set_ylabel('arcsecond')
        ax.legend(loc='upper center')
    return dirperf


def radial_profile(arr, binsize=1):
    """Azimuthal mean of ``arr`` in rings of width ``binsize`` around pixel
    (int(n0/2 + .5), int(n1/2 + .5)) (psfrec.py:810-823).  Returns (bin centres, mean per ring);
    empty rings give nan, as in the reference."""
    arr = np.asarray(arr, dtype=float)
    c0, c1 = int(arr.shape[0] / 2 + .5), int(arr.shape[1] / 2 + .5)
    r = np.hypot(np.arange(arr.shape[0])[:, None] - c0, np.arange(arr.shape[1])[None, :] - c1)
    nbins = int(np.round(r.max() / binsize) + 1)
    edges = np.linspace(0, nbins * binsize, nbins + 1)
    count = np.histogram(r, edges)[0]
    total = np.histogram(r, edges, weights=arr)[0]
    with np.errstate(invalid='ignore', divide='ignore'):
        return (edges[1:] + edges[:-1]) / 2, total / count


def plot_psf(filename, npsflin=1):
    """Figure of a reconstruction result (psfrec.py:826-858): 2 x 3 panels -- the second plane of
    PSF_MEAN (log scale), an empty panel, the reconstruction directions with the four LGS at 63
    arcsec; the radial profile of that plane (log), FWHM(lambda) and beta(lambda) from FIT_MEAN.
    ``filename`` is an HDUList (astropy's or this package's) or a path to the FITS file."""
    import matplotlib.pyplot as plt
    from matplotlib.colors import LogNorm
    opened = isinstance(filename, (str, os.PathLike))
    hdul = (_astropy()[0] or _minifits).open(filename) if opened else filename
    try:
        psf = np.array(hdul['PSF_MEAN'].data, dtype=float)
        fit = hdul['FIT_MEAN'].data
        lbda = np.array(fit['lbda'], dtype=float)
        fwhm = np.array(fit['fwhm'], dtype=float)[:, 0]
        beta = np.array(fit['n'], dtype=float)
    finally:
        if opened:
            hdul.close()
    plane = psf[1]
    fig, axes = plt.subplots(2, 3, figsize=(12, 6), tight_layout=True)
    top, bottom = axes
    im = top[0].imshow(plane, origin='lower', norm=LogNorm())
    fig.colorbar(im, ax=top[0])
    top[0].set_title('PSF')
    top[1].axis('off')
    poslgs = 63.0 * np.array([[1, 1], [-1, -1], [-1, 1], [1, -1]], dtype=float).T   # arcsec
    direction_perf(npsflin, plot=True, lgs=poslgs, ax=top[2])
    centers, prof = radial_profile(plane)
    bottom[0].plot(centers[1:], prof[1:], lw=1)
    bottom[0].set_yscale('log')
    bottom[0].set_title('radial profile')
    bottom[1].plot(lbda, fwhm)
    bottom[1].set_title(r'$FWHM(\lambda)$')
    bottom[2].plot(lbda, beta)
    bottom[2].set_title(r'$\beta(\lambda)$')
    return fig
