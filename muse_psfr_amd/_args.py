"""What include/mpsfr.h says about arguments, in NumPy alone: the limits and flag values of the header, four
primitives (integer, number, flag, array; stamp_stack beside array) and the validators of the calls, which are plain
functions that call the primitives top to bottom.  Every refusal is a ValueError raised before the library is touched;
with two bad arguments the one checked first is reported, so the order of the checks is part of the behaviour."""
import numpy as np

NFIT = 16
NFIT_ELL = 24                # elliptical fit rows (MPSFR_NFIT_ELL, include/mpsfr.h)
MAX_METRIC_RADII = 16        # radii, boxes, fractions of one metrics call (MPSFR_MAX_METRIC_RADII)
NMET_HEAD = 8                # leading fields of a metrics row (MPSFR_NMET_HEAD)
FIT_ILL_CONDITIONED = 4      # status bit of fit_out[14] (MPSFR_FIT_ILL_CONDITIONED, include/mpsfr.h)
FIT_BACKGROUND = 1           # flags of mpsfr_fit_stamps_observed (MPSFR_FIT_BACKGROUND, MPSFR_FIT_ELLIPTICAL)
FIT_ELLIPTICAL = 2
NFIT_PSF = 16                # rows of the PSF-model fit (MPSFR_NFIT_PSF)
FIT_FIXED_SHIFT = 4          # flag of mpsfr_fit_stamps_psf (MPSFR_FIT_FIXED_SHIFT), beside FIT_BACKGROUND
FIT_PSF_MAX_SHIFT = 8.0      # |dp|, |dq| bound in pixels (MPSFR_FIT_PSF_MAX_SHIFT)
NFIT_GROUP = 48              # rows of the PSF-model fit of blended groups (MPSFR_NFIT_GROUP)
MAX_GROUP = 4                # sources per stamp (MPSFR_MAX_GROUP)
FIT_COMMON_SHIFT = 8         # flag of mpsfr_fit_groups_psf (MPSFR_FIT_COMMON_SHIFT), beside FIT_BACKGROUND, FIT_FIXED_SHIFT
FIT_DRIFT = 16               # flag of mpsfr_fit_spectra_psf (MPSFR_FIT_DRIFT), beside FIT_BACKGROUND
NFIT_SPEC = 16               # head of a row of mpsfr_fit_spectra_psf (MPSFR_NFIT_SPEC)
NFIT_SPEC_LAYER = 10         # values per layer of such a row (MPSFR_NFIT_SPEC_LAYER)
MAX_SPEC_LAYERS = 4096       # MPSFR_MAX_SPEC_LAYERS
GROUP_MODES = ('free', 'common', 'fixed')
RENDER_SUBTRACT = 1          # flag of mpsfr_render_stars (MPSFR_RENDER_SUBTRACT)
NRENDER = 4                  # doubles per star of its star_out (MPSFR_NRENDER): status, frame pixels in the footprint, 0, 0
MAX_IMAGE_SIDE = 16384       # rows, columns of a frame (MPSFR_MAX_IMAGE_SIDE)
MAX_IMAGE_PIXELS = 1 << 26   # and pixels
MAX_ORIGIN = 1 << 30         # |origin| bound of the frame calls
RENDER_SORT_CHUNK = 256      # stars of one frame tile that the renderer sorts in LDS (MPSFR_RENDER_SORT_CHUNK)
RENDER_APRON = 10            # a star's footprint: its stamp and this many pixels around it
NFIND = 8                    # doubles per star of mpsfr_find_stars (MPSFR_NFIND): Y, X, T, H, b, sharpness, pixels, flags
FIND_MAX_HALF = 8            # half side of the filter core (MPSFR_FIND_MAX_HALF)
FIND_MAX_SEP = 16            # half side of the square a peak dominates (MPSFR_FIND_MAX_SEP)
FIND_MAX_STARS = 1 << 24     # rows of one call
NGROUP = 8                   # int32 per group row of mpsfr_group_stars (MPSFR_NGROUP): n, flags, label, 0, 4 members
GROUP_MAX_CRIT = 16.0        # largest critical separation in pixels (MPSFR_GROUP_MAX_CRIT)
GROUP_OVERSIZE = 1           # group flag: more than MAX_GROUP members (MPSFR_GROUP_OVERSIZE)
GROUP_WIDE = 2               # group flag: a member's |shift| beyond FIT_PSF_MAX_SHIFT (MPSFR_GROUP_WIDE)
GROUP_MAX_STARS = 1 << 24    # stars of one call
GROUP_FILLER_ORIGIN = -(1 << 30)   # origin of filler rows and of oversize groups
NFRAMEFIT = 8                # doubles per star of mpsfr_fit_frame_psf (MPSFR_NFRAMEFIT), and of its head
FRAME_FIT_MAX_RADIUS = 20.0  # largest fit radius in pixels (MPSFR_FRAME_FIT_MAX_RADIUS)
FRAME_FIT_MAX_ITER = 1000    # MPSFR_FRAME_FIT_MAX_ITER
FRAME_FIT_MAX_STARS = 1 << 20
CUBE_FIT_MAX_LAYERS = 4096   # layers of one mpsfr_fit_cube_psf call (MPSFR_CUBE_FIT_MAX_LAYERS)
NFRAMEFREE = 16              # doubles per star of mpsfr_fit_frame_psf_free (MPSFR_NFRAMEFREE)
NFRAMEFREE_HEAD = 12         # doubles of its head (MPSFR_NFRAMEFREE_HEAD)
FRAME_FREE_MAX_OUTER = 16    # most Gauss-Newton steps of one call (MPSFR_FRAME_FREE_MAX_OUTER)
FRAME_FREE_MAX_STEP = 1.0    # largest max_step in pixels (MPSFR_FRAME_FREE_MAX_STEP)
FRAME_FREE_MAX_MOVE = 4.0    # largest max_move in pixels (MPSFR_FRAME_FREE_MAX_MOVE)
FRAME_FREE_HELD = 1          # flag in column 14: held in the last outer step (MPSFR_FRAME_FREE_HELD)
FRAME_FREE_BOUND = 2         # resting on max_move or on the +-8 bound (MPSFR_FRAME_FREE_BOUND)
FRAME_FREE_CLIPPED = 4       # the last step was clipped by max_step (MPSFR_FRAME_FREE_CLIPPED)
NCUBEFREE_POS = 8            # doubles per star of pos_out of mpsfr_fit_cube_psf_free (MPSFR_NCUBEFREE_POS)
NCUBEFREE_CALL = 8           # doubles of its call_out (MPSFR_NCUBEFREE_CALL)
CUBE_FREE_WORK_BYTES = 4 << 30   # budget of work memory of one such call (MPSFR_CUBE_FREE_WORK_BYTES)
NBACK = 8                    # doubles per mesh cell of mpsfr_frame_background (MPSFR_NBACK)
NBACK_HEAD = 4               # doubles per layer of its head (MPSFR_NBACK_HEAD)
BACKGROUND_MIN_BOX = 8       # side of a mesh cell in pixels (MPSFR_BACKGROUND_MIN_BOX, MPSFR_BACKGROUND_MAX_BOX)
BACKGROUND_MAX_BOX = 64
BACKGROUND_MAX_CLIP = 16     # most clipping passes of a cell (MPSFR_BACKGROUND_MAX_CLIP)
BACKGROUND_MAX_KAPPA = 100.0
BACK_FILLED = 1              # cell flag: invalid, level and rms come from neighbours (MPSFR_BACK_FILLED)
BACK_CLIP_CAP = 2            # the clipping ended at max_clip (MPSFR_BACK_CLIP_CAP)
BACK_FLAT = 4                # MAD == 0 at the last pass (MPSFR_BACK_FLAT)
DIM_AO = 80
PREC_MIXED, PREC_F64 = 0, 1
E_GRID = -3
MAX_FIELD_POSITIONS = 25     # AoGeom::dir[2][25]: positions of one mpsfr_reconstruct_field call
MAX_FIELD_ARCSEC = 60.0      # |x|, |y| bound of a field position (twice the WFM half-field)
MAX_LAYERS = 8               # MPSFR_MAX_LAYERS
MAX_LAYER_HEIGHT = 50000.0   # m
MAX_WIND_SPEED = 100.0       # m/s
REF_WIND_DIR = (0.628163, -0.326497)   # the reference's two wind directions [rad] (psfrec.py:61)
MAX_BANDS = 16               # MPSFR_MAX_BANDS
METRIC_CENTER_MAX = 100.0       # kCenterMax of metrics.hip: beyond it the kernel gives status 2
INT_MAX = (1 << 31) - 1      # the largest count a C int carries


# ---- the four primitives

def integer(name, n, lo, hi, msg='%(name)s must be an integer between %(lo)d and %(hi)d'):
    """`n` as an int in lo .. hi: an int or np.integer, not a bool (ValueError).  A caller with words of its own passes
    `msg`, which may name %(name)s, %(n)r, %(lo)d and %(hi)d; it is formatted only when the check fails."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not lo <= n <= hi:
        raise ValueError(msg % dict(name=name, n=n, lo=lo, hi=hi))
    return int(n)


def number(name, v):
    """`v` as a float: a finite int, float, np.integer or np.floating, not a bool and not a 0-d array (ValueError).
    Range tests stay with the caller."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError('%s must be a finite number' % name)
    return float(v)


def flag(name, v):
    """`v` if it is a bool or np.bool_ (ValueError)."""
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError('%s must be True or False' % name)
    return v


def array(name, a, fill=False, unwrap=False):
    """`a` as a float64 array, without a copy where it is one already (ValueError).  fill: the masked pixels of a
    masked array become NaN.  unwrap: an object with a `.data` attribute gives that, which for a masked array that
    is not filled means the values under the mask."""
    try:
        if fill and isinstance(a, np.ma.MaskedArray):
            return np.ma.filled(a.astype(np.float64), np.nan)
        return np.asarray(getattr(a, 'data', a) if unwrap else a, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('%s must be a numeric array' % name) from None


def stamp_stack(name, a, dimpsf, fill=False, unwrap=False):
    """`a`, a non-empty (..., dimpsf, dimpsf) array of `array`, as C-contiguous (n, dimpsf, dimpsf) float64 (ValueError)."""
    st = array(name, a, fill, unwrap)
    if st.ndim < 2 or st.shape[-2:] != (dimpsf, dimpsf) or st.size == 0:
        raise ValueError('%s must have the shape (..., %d, %d)' % (name, dimpsf, dimpsf))
    return np.ascontiguousarray(st).reshape(-1, dimpsf, dimpsf)


# ---- counts and pointers of the device forms

def _positive_int(name, n):
    # (no upper end: np.inf needs a message of its own, since %(hi)d of the usual one cannot format it)
    integer(name, n, 1, np.inf, '%(name)s must be a positive integer')


def _device_pointers(**ptrs):
    """ValueError unless every named raw device pointer is set."""
    if not all(ptrs.values()):
        names = list(ptrs)
        raise ValueError('%s and %s must be device pointers' % (', '.join(names[:-1]), names[-1]))


def _model_per_star(npsf, n, psf_index_ptr, what='nstar'):
    """ValueError unless a device call without psf_index_ptr brings one model per star."""
    if not psf_index_ptr and npsf != n:
        raise ValueError('without psf_index_ptr, npsf must equal %s' % what)


def _frame_fit_device(ny, nx, nstar, npsf, psf_index_ptr, **ptrs):
    """What the device forms of the frame and cube fits check first, in this order: the frame, the stars, the models,
    the pointers that must be set.  Returns nstar."""
    frame_shape(ny, nx)
    nstar = frame_fit_stars(nstar)
    _positive_int('npsf', npsf)
    _device_pointers(**ptrs)
    _model_per_star(npsf, nstar, psf_index_ptr)
    return nstar


def _group_size(nsrc):
    integer('nsrc', nsrc, 2, MAX_GROUP, 'a group has %(lo)d to %(hi)d sources (one source is fit_stamps_psf), not %(n)r')


def _spec_layers(nl):
    integer('nl', nl, 1, MAX_SPEC_LAYERS, 'a star cube has %(lo)d to %(hi)d layers, not %(n)r')


# ---- the reconstruct calls

def field_positions(positions, max_n=MAX_FIELD_POSITIONS):
    """Validated (npos, 2) float64 C-contiguous array of field positions (x, y) in arcsec, in the convention of
    direction_perf (x = dirperf[0]).  Raises ValueError for a wrong shape, no position, more than `max_n`, a
    non-finite coordinate or one beyond MAX_FIELD_ARCSEC."""
    try:
        pos = np.array(positions, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('positions must be an (n, 2) array of (x, y) in arcsec') from None
    if pos.ndim != 2 or pos.shape[1] != 2:
        raise ValueError('positions must be an (n, 2) array of (x, y) in arcsec, got shape %s' % (pos.shape,))
    if pos.shape[0] < 1:
        raise ValueError('positions must not be empty')
    if max_n is not None and pos.shape[0] > max_n:
        raise ValueError('at most %d positions per call, got %d' % (max_n, pos.shape[0]))
    if not np.all(np.isfinite(pos)):
        raise ValueError('positions must be finite')
    if np.any(np.abs(pos) > MAX_FIELD_ARCSEC):
        raise ValueError('positions must satisfy |x|, |y| <= %g arcsec' % MAX_FIELD_ARCSEC)
    return np.ascontiguousarray(pos)


def grid_side(npsflin):
    """npsflin of a call that evaluates the npsflin x npsflin grid (ValueError), for _grid_or_positions here and the
    compute_* calls of psfrec.py."""
    # (the message is what `integer` would say by itself; it is spelled out so that a search for the words a caller
    # sees finds this line, the one place the rule is stated)
    return integer('npsflin', npsflin, 1, 5, 'npsflin must be an integer between 1 and 5')


def _grid_or_positions(npsflin, positions):
    """What a call evaluates: the npsflin x npsflin grid (positions None; npsflin None means 1) or the caller's
    positions, which take npsflin None or 0.  Returns (npsflin as C takes it, npos, pos or None); ValueError for
    anything else."""
    if positions is None:
        return grid_side(1 if npsflin is None else npsflin), 0, None
    if npsflin not in (0, None):
        raise ValueError('a call with positions takes npsflin = 0')
    pos = field_positions(positions)
    return 0, pos.shape[0], pos


def profile_layers(h, wind_speed, wind_dir):
    """Validated float64 arrays (h, wind_speed, wind_dir) of a Cn2 profile: 1..MAX_LAYERS layers, altitudes in
    [0, MAX_LAYER_HEIGHT] m, speeds in [0, MAX_WIND_SPEED] m/s (a scalar speed applies to every layer), directions
    in radians, all finite.  Raises ValueError otherwise -- the refusals of mpsfr_reconstruct_profile."""
    try:
        hh = np.array(h, dtype=np.float64).reshape(-1)
        ws = np.array(wind_speed, dtype=np.float64)
        wd = np.array(wind_dir, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError('h, wind_speed and wind_dir must be numeric') from None
    n = hh.size
    if not 1 <= n <= MAX_LAYERS:
        raise ValueError('a profile has 1 to %d layers, got %d' % (MAX_LAYERS, n))
    ws = np.full(n, float(ws)) if ws.ndim == 0 else ws.reshape(-1)
    if ws.size != n or wd.size != n:
        raise ValueError('h, wind_speed and wind_dir need one value per layer (%d)' % n)
    if not (np.all(np.isfinite(hh)) and np.all(np.isfinite(ws)) and np.all(np.isfinite(wd))):
        raise ValueError('altitudes and winds must be finite')
    if np.any(hh < 0) or np.any(hh > MAX_LAYER_HEIGHT):
        raise ValueError('layer altitudes must lie in [0, %g] m' % MAX_LAYER_HEIGHT)
    if np.any(ws < 0) or np.any(ws > MAX_WIND_SPEED):
        raise ValueError('wind speeds must lie in [0, %g] m/s' % MAX_WIND_SPEED)
    return (np.ascontiguousarray(hh), np.ascontiguousarray(ws), np.ascontiguousarray(wd))


def profile_weights(cn2, nrow, nlayer):
    """Validated (nrow, nlayer) float64 weights: one row (1-D) applies to every row.  Refuses negative or
    non-finite weights and rows that sum to 0 (ValueError)."""
    try:
        w = np.array(cn2, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('cn2 must be numeric') from None
    if w.ndim == 1:
        w = np.broadcast_to(w, (nrow, w.size))
    if w.ndim != 2 or w.shape != (nrow, nlayer):
        raise ValueError('cn2 must be (%d,) or (%d, %d), got shape %s' % (nlayer, nrow, nlayer, np.shape(cn2)))
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError('Cn2 weights must be finite and >= 0')
    if np.any(w.sum(axis=1) <= 0):
        raise ValueError('every row of Cn2 weights needs a positive sum')
    return np.ascontiguousarray(w)


def band_weight_matrix(weights, nl):
    """Validated (nband, nl) float64 C-contiguous band weights (one band may be given 1-D): 1..MAX_BANDS bands,
    finite, >= 0, each band with a positive sum.  Raises ValueError otherwise -- the refusals of
    mpsfr_reconstruct_band."""
    try:
        w = np.array(weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('band weights must be numeric') from None
    if w.ndim == 1:
        w = w[None, :]
    if w.ndim != 2 or w.shape[1] != nl:
        raise ValueError('band weights must be (nband, %d), got shape %s' % (nl, np.shape(weights)))
    if not 1 <= w.shape[0] <= MAX_BANDS:
        raise ValueError('1 to %d bands per call, got %d' % (MAX_BANDS, w.shape[0]))
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError('band weights must be finite and >= 0')
    if np.any(w.sum(axis=1) <= 0):
        raise ValueError('every band needs a positive sum of weights')
    return np.ascontiguousarray(w)


# ---- the stamp family

def elliptical_stamps(stamps, dimpsf=40):
    """Stamps for the elliptical fit as a C-contiguous (n, dimpsf, dimpsf) float64 array; ValueError unless
    `stamps` is a non-empty array of shape (..., dimpsf, dimpsf) with finite values.  `.data` is unwrapped and a
    masked array is not filled: the values under the mask are fitted."""
    st = stamp_stack('stamps', stamps, dimpsf, unwrap=True)
    if not np.all(np.isfinite(st)):
        raise ValueError('stamps must be finite')
    return st


def observed_flags(background, circular):
    """The flags of mpsfr_fit_stamps_observed from two booleans (ValueError for anything else)."""
    flag('background', background)
    flag('circular', circular)
    return (FIT_BACKGROUND if background else 0) | (0 if circular else FIT_ELLIPTICAL)


def observed_stamps(stamps, var=None, dimpsf=40):
    """(stamps, var) for the weighted fit as C-contiguous (n, dimpsf, dimpsf) float64 arrays (var: None for unit
    weights); ValueError unless `stamps` is a non-empty numeric array of shape (..., dimpsf, dimpsf) and `var` has
    the same shape.  A masked array is accepted: masked pixels become NaN; `.data` is not unwrapped.  Non-finite
    pixels and variances that are not finite and > 0 are the mask of the fit, not an error."""
    st = stamp_stack('stamps', stamps, dimpsf, fill=True)
    if var is None:
        return st, None
    va = array('var', var, fill=True)
    if va.size != st.size or va.shape[-2:] != (dimpsf, dimpsf):
        raise ValueError('var must have the shape of stamps')
    return st, np.ascontiguousarray(va).reshape(-1, dimpsf, dimpsf)


def psf_fit_flags(background, fixed_shift):
    """The flags of mpsfr_fit_stamps_psf from two booleans (ValueError for anything else)."""
    flag('background', background)
    flag('fixed_shift', fixed_shift)
    return (FIT_BACKGROUND if background else 0) | (FIT_FIXED_SHIFT if fixed_shift else 0)


def psf_fit_arguments(nstamp, psf, psf_index, shift, background, fixed_shift, dimpsf=40):
    """(psf, psf_index, shift, flags) of a PSF-model fit of `nstamp` stars, validated as mpsfr_fit_stamps_psf validates
    host arguments (ValueError): psf a non-empty numeric array (..., dimpsf, dimpsf) -> (npsf, dimpsf, dimpsf) float64
    (`.data` unwrapped, a masked array not filled); psf_index None (then npsf == nstamp) or nstamp integers in
    0..npsf-1 -> int32, refused by dtype kind, not by value: a float array of whole numbers is refused; shift None or
    (nstamp, 2) finite values within FIT_PSF_MAX_SHIFT pixels, required under fixed_shift."""
    flags = psf_fit_flags(background, fixed_shift)
    ps = stamp_stack('psf', psf, dimpsf, unwrap=True)
    ix = None
    if psf_index is None:
        if ps.shape[0] != nstamp:
            raise ValueError('without psf_index there must be one model stamp per star (%d), got %d'
                             % (nstamp, ps.shape[0]))
    else:
        try:
            raw = np.asarray(psf_index)
            ix = raw.astype(np.int64).ravel()
        except (TypeError, ValueError):
            raise ValueError('psf_index must be an integer array') from None
        if raw.dtype.kind not in 'iu' or ix.size != nstamp:
            raise ValueError('psf_index must hold one integer per star')
        if np.any(ix < 0) or np.any(ix >= ps.shape[0]):
            raise ValueError('psf_index must lie in 0..%d' % (ps.shape[0] - 1))
        ix = np.ascontiguousarray(ix, dtype=np.int32)
    sh = None
    if shift is None:
        if fixed_shift:
            raise ValueError('fixed_shift needs the shift array')
    else:
        sh = array('shift', shift)
        if sh.size != 2 * nstamp or sh.shape[-1:] != (2,):
            raise ValueError('shift must have the shape (%d, 2)' % nstamp)
        if not np.all(np.abs(sh) <= FIT_PSF_MAX_SHIFT):           # (NaN fails)
            raise ValueError('shift must be finite and within %g pixels' % FIT_PSF_MAX_SHIFT)
        sh = np.ascontiguousarray(sh).reshape(nstamp, 2)
    return ps, ix, sh, flags


def group_fit_flags(background, mode):
    """The flags of mpsfr_fit_groups_psf from a boolean and the mode 'free' | 'common' | 'fixed' (ValueError for
    anything else)."""
    flag('background', background)
    if not isinstance(mode, str) or mode not in GROUP_MODES:
        raise ValueError("mode must be 'free', 'common' or 'fixed'")
    return (FIT_BACKGROUND if background else 0) | {'free': 0, 'common': FIT_COMMON_SHIFT, 'fixed': FIT_FIXED_SHIFT}[mode]


def group_fit_arguments(nstamp, psf, psf_index, shift, background, mode, dimpsf=40):
    """(psf, psf_index, shift, flags) of a PSF-model fit of `nstamp` blended groups, validated as mpsfr_fit_groups_psf
    validates host arguments (ValueError): psf and psf_index as psf_fit_arguments; shift required, (nstamp, K, 2) with
    K = 2 .. MAX_GROUP, finite values within FIT_PSF_MAX_SHIFT pixels."""
    flags = group_fit_flags(background, mode)
    ps, ix, _, _ = psf_fit_arguments(nstamp, psf, psf_index, None, True, False, dimpsf)
    if shift is None:
        raise ValueError('a group fit needs the positions of its sources (shift)')
    sh = array('shift', shift)
    if sh.ndim < 2 or sh.shape[-1] != 2 or sh.size != nstamp * sh.shape[-2] * 2:
        raise ValueError('shift must have the shape (%d, K, 2)' % nstamp)
    _group_size(int(sh.shape[-2]))
    if not np.all(np.abs(sh) <= FIT_PSF_MAX_SHIFT):           # (NaN fails)
        raise ValueError('the positions must be finite and within %g pixels' % FIT_PSF_MAX_SHIFT)
    return ps, ix, np.ascontiguousarray(sh).reshape(nstamp, sh.shape[-2], 2), flags


def spectra_fit_flags(background, x, nl):
    """(flags, x) of mpsfr_fit_spectra_psf: `x` None (no drift) or nl finite values in [-1, 1] of which at least two
    differ -> contiguous float64 and the drift flag (ValueError for anything else)."""
    flag('background', background)
    flags = FIT_BACKGROUND if background else 0
    if x is None:
        return flags, None
    xx = np.ascontiguousarray(array('x', x).ravel())
    if nl < 2 or xx.size != nl:
        raise ValueError('the drift needs at least two layers and one x per layer (%d)' % nl)
    if not np.all(np.abs(xx) <= 1.0):            # (NaN fails)
        raise ValueError('x must be finite and lie in [-1, 1]')
    if np.all(xx == xx[0]):
        raise ValueError('at least two values of x must differ')
    return flags | FIT_DRIFT, xx


def spectra_fit_arguments(cubes, var, psf, psf_index, shift, background, x, dimpsf=40):
    """(cubes, var, psf, psf_index, shift, x, flags) of a PSF-model fit of star cubes, validated as
    mpsfr_fit_spectra_psf validates host arguments (ValueError): cubes (n, nl, dimpsf, dimpsf) (one cube (nl, dimpsf,
    dimpsf) is one star), var None or of the same shape, psf (npsf, nl, dimpsf, dimpsf) (or one cube); psf_index and
    shift as psf_fit_arguments, per star; x as spectra_fit_flags."""
    try:
        nd = np.ndim(cubes)
    except (TypeError, ValueError):
        nd = 0
    if nd not in (3, 4):
        raise ValueError('cubes must have the shape (n, nl, %d, %d)' % (dimpsf, dimpsf))
    shape = np.shape(cubes)
    n = shape[0] if nd == 4 else 1
    nl = shape[-3]
    st, va = observed_stamps(cubes, var, dimpsf)          # (non-empty, so n >= 1, and n * nl stamps)
    _spec_layers(int(nl))
    flags, xx = spectra_fit_flags(background, x, nl)
    try:
        pnd = np.ndim(getattr(psf, 'data', psf))
        pshape = np.shape(getattr(psf, 'data', psf))
    except (TypeError, ValueError):
        raise ValueError('psf must be a numeric array') from None
    if pnd not in (3, 4) or pshape[-3] != nl:
        raise ValueError('psf must have the shape (npsf, %d, %d, %d)' % (nl, dimpsf, dimpsf))
    npsf = pshape[0] if pnd == 4 else 1
    ps, _, _, _ = psf_fit_arguments(npsf * nl, psf, None, None, True, False, dimpsf)
    ps = ps.reshape(npsf, nl, dimpsf, dimpsf)
    # index and start: one per star, checked against the number of model cubes
    _, ix, sh, _ = psf_fit_arguments(n, np.zeros((npsf, dimpsf, dimpsf)), psf_index, shift, True, False, dimpsf)
    return (st.reshape(n, nl, dimpsf, dimpsf), None if va is None else va.reshape(n, nl, dimpsf, dimpsf), ps, ix, sh,
            xx, flags)


def metric_stamps(stamps, dimpsf=40):
    """Stamps for the metrics as a C-contiguous (n, dimpsf, dimpsf) float64 array; ValueError unless `stamps` is a
    non-empty numeric array of shape (..., dimpsf, dimpsf).  `.data` is unwrapped and a masked array is not filled.
    (Non-finite pixels are the kernel's business: such a stamp gets status 2.)"""
    return stamp_stack('stamps', stamps, dimpsf, unwrap=True)


def metric_parameters(radii_px, boxes_px, fractions, dimpsf=40):
    """The three parameter arrays of a metrics call (pixels, pixels, fractions) as contiguous float64, validated as
    mpsfr_stamp_metrics validates them (ValueError): 0..MAX_METRIC_RADII of each and at least one in all, radii and
    box sides finite, > 0 and <= 2 dimpsf, fractions in (0, 1)."""
    res = []
    for name, v in (('radii', radii_px), ('boxes', boxes_px), ('fractions', fractions)):
        try:
            a = np.atleast_1d(np.asarray(() if v is None else v, dtype=np.float64))
        except (TypeError, ValueError):
            raise ValueError('%s must be numbers' % name) from None
        if a.ndim != 1 or a.size > MAX_METRIC_RADII:
            raise ValueError('%s must be a 1-D sequence of at most %d values' % (name, MAX_METRIC_RADII))
        res.append(np.ascontiguousarray(a))
    rad, box, frac = res
    if rad.size + box.size + frac.size == 0:
        raise ValueError('need at least one radius, box or fraction')
    for name, a in (('radii', rad), ('boxes', box)):
        if not np.all(np.isfinite(a) & (a > 0) & (a <= 2 * dimpsf)):
            raise ValueError('%s must be finite, > 0 and at most %d pixels' % (name, 2 * dimpsf))
    if not np.all((frac > 0) & (frac < 1)):
        raise ValueError('fractions must lie in (0, 1)')
    return rad, box, frac


def metric_centers(centers, n):
    """(n, 2) centres (p, q) in pixels as contiguous float64; ValueError unless finite, within METRIC_CENTER_MAX and of
    that shape."""
    try:
        ce = np.asarray(centers, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('centers must be an (n, 2) array of (p, q) in pixels') from None
    if ce.shape != (n, 2):
        raise ValueError('centers must have the shape (%d, 2): one (p, q) per stamp' % n)
    if not np.all(np.isfinite(ce)) or np.any(np.abs(ce) > METRIC_CENTER_MAX):
        raise ValueError('centers must be finite, with |p| and |q| at most %g pixels' % METRIC_CENTER_MAX)
    return np.ascontiguousarray(ce)


# ---- the frame calls

def frame_shape(ny, nx):
    """ValueError unless (ny, nx) is the shape of a frame: 1 .. MAX_IMAGE_SIDE each way, at most 2^26 pixels."""
    ny = integer('ny', ny, 1, MAX_IMAGE_SIDE)
    nx = integer('nx', nx, 1, MAX_IMAGE_SIDE)
    if ny * nx > MAX_IMAGE_PIXELS:
        raise ValueError('a frame holds at most 2^26 pixels')
    return ny, nx


def frame_images(image, var=None):
    """(image, var) of a frame call as C-contiguous (ny, nx) float64 arrays (var: None if absent); ValueError unless
    `image` is a numeric 2-D array with the shape of a frame and `var` has the same shape.  A masked array is
    accepted: masked pixels become NaN; `.data` is not unwrapped.  Non-finite pixels are data, not an error."""
    im = array('image', image, fill=True)
    if im.ndim != 2 or im.size == 0:
        raise ValueError('image must have the shape (ny, nx)')
    frame_shape(*im.shape)
    if var is None:
        return np.ascontiguousarray(im), None
    va = array('var', var, fill=True)
    if va.shape != im.shape:
        raise ValueError('var must have the shape of image')
    return np.ascontiguousarray(im), np.ascontiguousarray(va)


def star_origins(origin, n=None):
    """The (n, 2) int32 origins of a frame call; ValueError unless `origin` is a non-empty integer array of that shape
    (of `n` rows if given) with |origin| <= MAX_ORIGIN.  Refused by dtype kind, not by value, as psf_index is."""
    try:
        raw = np.asarray(origin)
        og = raw.astype(np.int64)
    except (TypeError, ValueError):
        raise ValueError('origin must be an integer array') from None
    if raw.dtype.kind not in 'iu' or og.ndim != 2 or og.shape[1] != 2 or og.shape[0] < 1:
        raise ValueError('origin must be an integer array of shape (n, 2)')
    if n is not None and og.shape[0] != n:
        raise ValueError('origin must have the shape (%d, 2)' % n)
    if np.any(np.abs(og) > MAX_ORIGIN):
        raise ValueError('origin must lie within 2^30 pixels')
    return np.ascontiguousarray(og, dtype=np.int32)


def render_flags(subtract):
    """The flags of mpsfr_render_stars from a boolean (ValueError for anything else)."""
    return RENDER_SUBTRACT if flag('subtract', subtract) else 0


def star_scales(name, scale, n):
    """`scale` (the argument `name`) as n finite float64 values, one per star (ValueError)."""
    sc = array(name, scale)
    if sc.size != n or sc.ndim > 1:
        raise ValueError('%s must hold one value per star (%d)' % (name, n))
    if not np.all(np.isfinite(sc)):
        raise ValueError('%s must be finite' % name)
    return np.ascontiguousarray(sc).reshape(n)


def render_arguments(psf, origin, scale, shift, psf_index, image, shape, subtract, dimpsf=40):
    """(image or None, ny, nx, psf, psf_index, origin, shift, scale, flags) of a render call, validated as
    mpsfr_render_stars validates host arguments (ValueError): origin as star_origins; psf, psf_index and shift as
    psf_fit_arguments; scale n finite values; `image` a frame or None with `shape` = (ny, nx) (both: they must agree);
    subtract needs the image."""
    flags = render_flags(subtract)
    og = star_origins(origin)
    n = og.shape[0]
    ps, ix, sh, _ = psf_fit_arguments(n, psf, psf_index, shift, True, False, dimpsf)
    sc = star_scales('scale', scale, n)
    if image is None:
        if subtract:
            raise ValueError('subtract needs the image')
        if shape is None:
            raise ValueError('give the image or the shape of the frame')
        try:
            ny, nx = shape
        except (TypeError, ValueError):
            raise ValueError('shape must be (ny, nx)') from None
        ny, nx = frame_shape(ny, nx)
        im = None
    else:
        im, _ = frame_images(image)
        ny, nx = im.shape
        if shape is not None and tuple(shape) != (ny, nx):
            raise ValueError('shape differs from the shape of image')
    return im, ny, nx, ps, ix, og, sh, sc, flags


def find_parameters(half, sep, threshold, max_stars, dimpsf=40):
    """(half, sep, threshold, max_stars) of a find call, validated as mpsfr_find_stars validates them (ValueError)."""
    half = integer('half', half, 1, min(FIND_MAX_HALF, dimpsf // 2))
    sep = integer('sep', sep, 1, FIND_MAX_SEP)
    max_stars = integer('max_stars', max_stars, 1, FIND_MAX_STARS)
    return half, sep, number('threshold', threshold), max_stars


def find_arguments(image, var, psf, half, sep, threshold, max_stars, dimpsf=40):
    """(image, var or None, psf, half, sep, threshold, max_stars) of a host find call, validated as mpsfr_find_stars
    validates host arguments (ValueError): the frame as frame_images, `psf` one numeric (dimpsf, dimpsf) stamp whose
    (2 half + 1)^2 core is finite and not constant.  `psf` is neither filled nor unwrapped."""
    im, va = frame_images(image, var)
    half, sep, threshold, max_stars = find_parameters(half, sep, threshold, max_stars, dimpsf)
    ps = np.ascontiguousarray(array('psf', psf))
    if ps.shape != (dimpsf, dimpsf):
        raise ValueError('psf must be one model stamp of shape (%d, %d)' % (dimpsf, dimpsf))
    c = dimpsf // 2
    core = ps[c - half:c + half + 1, c - half:c + half + 1]
    if not np.all(np.isfinite(core)):
        raise ValueError('psf must be finite over its core')
    if np.all(core == core[0, 0]):
        raise ValueError('psf must not be constant over its core')
    return im, va, ps, half, sep, threshold, max_stars


def background_parameters(box, filter, kappa, max_clip, min_frac):
    """(box, filter, kappa, max_clip, min_frac) of a background call, validated as mpsfr_frame_background validates them
    (ValueError)."""
    box = integer('box', box, BACKGROUND_MIN_BOX, BACKGROUND_MAX_BOX)
    if integer('filter', filter, 1, 5, 'filter must be 1, 3 or 5') % 2 == 0:
        raise ValueError('filter must be 1, 3 or 5')
    max_clip = integer('max_clip', max_clip, 0, BACKGROUND_MAX_CLIP)
    kappa = number('kappa', kappa)
    if not 1.0 <= kappa <= BACKGROUND_MAX_KAPPA:
        raise ValueError('kappa must lie between 1 and %g' % BACKGROUND_MAX_KAPPA)
    min_frac = number('min_frac', min_frac)
    if not 0.0 < min_frac <= 1.0:
        raise ValueError('min_frac must lie in (0, 1]')
    return box, int(filter), kappa, max_clip, min_frac


def background_shape(nl, ny, nx):
    """ValueError unless (nl, ny, nx) is the shape of a background call: layers that are frames, 2^26 pixels in all."""
    _positive_int('nl', nl)
    ny, nx = frame_shape(ny, nx)
    if int(nl) * ny * nx > MAX_IMAGE_PIXELS:
        raise ValueError('a background call holds at most 2^26 pixels')
    return int(nl), ny, nx


def background_arguments(image, var, apply_to, box, filter, kappa, max_clip, min_frac):
    """(image, var or None, apply_to or None, box, filter, kappa, max_clip, min_frac) of a host background call,
    validated as mpsfr_frame_background validates host arguments (ValueError): `image` a frame of frame_images or a
    numeric (nl, ny, nx) cube of such frames with at most 2^26 pixels (masked pixels become NaN; `.data` is not
    unwrapped); var and apply_to None or of its shape."""
    im = array('image', image, fill=True)
    if im.ndim not in (2, 3) or im.size == 0:
        raise ValueError('image must have the shape (ny, nx) or (nl, ny, nx)')
    background_shape(*((1,) * (3 - im.ndim) + im.shape))
    others = []
    for a, what in ((var, 'var'), (apply_to, 'apply_to')):
        if a is not None:
            a = array(what, a, fill=True)
            if a.shape != im.shape:
                raise ValueError('%s must have the shape of image' % what)
            a = np.ascontiguousarray(a)
        others.append(a)
    return (np.ascontiguousarray(im), others[0], others[1]) + background_parameters(box, filter, kappa, max_clip, min_frac)


def group_parameters(nstar, stride, crit, max_groups):
    """(nstar, stride, crit, max_groups) of a group call, validated as mpsfr_group_stars validates them (ValueError);
    max_groups=None stands for nstar."""
    nstar = integer('nstar', nstar, 1, GROUP_MAX_STARS)
    stride = integer('stride', stride, 2, INT_MAX)
    max_groups = nstar if max_groups is None else integer('max_groups', max_groups, 1, INT_MAX)
    # (crit keeps one message for type and range, so it is not a `number`; NaN fails the comparison)
    if isinstance(crit, bool) or not isinstance(crit, (int, float, np.integer, np.floating)) \
            or not 0.0 < crit <= GROUP_MAX_CRIT:
        raise ValueError('crit must be a number above 0 and at most %g pixels' % GROUP_MAX_CRIT)
    return nstar, stride, float(crit), max_groups


def group_arguments(pos, crit, shape, max_groups=None):
    """(pos, ny, nx, crit, max_groups) of a host group call, validated as mpsfr_group_stars validates host arguments
    (ValueError): `pos` a numeric (nstar, stride >= 2) array whose first two columns are (row, column); a row with a NaN
    in either is a filler, every other row lies within [-1, ny] x [-1, nx]; `shape` = (ny, nx) the shape of a frame."""
    try:
        ny, nx = shape
    except (TypeError, ValueError):
        raise ValueError('shape must be (ny, nx)') from None
    ny, nx = frame_shape(ny, nx)
    po = np.ascontiguousarray(array('pos', pos))
    if po.ndim != 2 or po.shape[0] < 1 or po.shape[1] < 2:
        raise ValueError('pos must have the shape (nstar, stride) with nstar >= 1 and stride >= 2')
    nstar, stride, crit, max_groups = group_parameters(po.shape[0], po.shape[1], crit, max_groups)
    y, x = po[:, 0], po[:, 1]
    star = ~(np.isnan(y) | np.isnan(x))
    with np.errstate(invalid='ignore'):
        inside = (y >= -1.0) & (y <= ny) & (x >= -1.0) & (x <= nx)
    if np.any(star & ~inside):
        raise ValueError('a position lies outside [-1, ny] x [-1, nx]')
    return po, ny, nx, crit, max_groups


def group_offsets(counts):
    """The first row of every class in the tables of mpsfr_group_stars, from its six counts: offsets[k - 1] for the
    groups of k = 1 .. MAX_GROUP stars, offsets[MAX_GROUP] for the oversize ones, offsets[MAX_GROUP + 1] the total."""
    c = np.asarray(counts, dtype=np.int64)
    if c.shape != (MAX_GROUP + 2,):
        raise ValueError('counts must hold the %d counts of a group call' % (MAX_GROUP + 2))
    return np.concatenate(([0], np.cumsum(c[1:])))


def group_shift_rows(shift, counts):
    """The shifts of mpsfr_group_stars one group per row: (max_groups, MAX_GROUP, 2), zero beyond a group's members,
    from the buffer `shift` of max_groups * MAX_GROUP * 2 doubles, in which the shifts of the groups of k stars lie at
    a pitch of 2 k doubles from 8 offset_k on."""
    buf = np.asarray(shift, dtype=np.float64).reshape(-1)
    rows = buf.size // (2 * MAX_GROUP)
    out = np.zeros((rows, MAX_GROUP, 2))
    off = group_offsets(counts)
    for k in range(1, MAX_GROUP + 1):
        lo = int(min(off[k - 1], rows))
        n = int(min(off[k], rows)) - lo
        if n > 0:
            out[lo:lo + n, :k] = buf[8 * lo:8 * lo + 2 * k * n].reshape(n, k, 2)
    return out


# ---- the crowded-field fits of frames and cubes

def frame_fit_stars(nstar):
    """The number of stars of a frame fit: an integer in 1 .. FRAME_FIT_MAX_STARS (ValueError)."""
    return integer('nstar', nstar, 1, FRAME_FIT_MAX_STARS)


def frame_fit_parameters(radius, background, max_iter, tol):
    """(radius, flags, max_iter, tol) of a frame fit, validated as mpsfr_fit_frame_psf validates them (ValueError)."""
    radius = number('radius', radius)
    if not 1.0 <= radius <= FRAME_FIT_MAX_RADIUS:
        raise ValueError('radius must lie between 1 and %g pixels' % FRAME_FIT_MAX_RADIUS)
    tol = number('tol', tol)
    if not 0.0 < tol < 1.0:
        raise ValueError('tol must lie in (0, 1)')
    max_iter = integer('max_iter', max_iter, 1, FRAME_FIT_MAX_ITER)
    return radius, FIT_BACKGROUND if flag('background', background) else 0, max_iter, tol


def frame_free_parameters(max_outer, pos_tol, max_step, max_move, min_snr):
    """(max_outer, pos_tol, max_step, max_move, min_snr) of a frame fit with free positions, validated as
    mpsfr_fit_frame_psf_free validates them (ValueError)."""
    max_outer = integer('max_outer', max_outer, 0, FRAME_FREE_MAX_OUTER)
    pos_tol = number('pos_tol', pos_tol)
    if not pos_tol > 0.0:
        raise ValueError('pos_tol must be > 0')
    max_step = number('max_step', max_step)
    if not 0.0 < max_step <= FRAME_FREE_MAX_STEP:
        raise ValueError('max_step must lie in (0, %g] pixels' % FRAME_FREE_MAX_STEP)
    max_move = number('max_move', max_move)
    if not 0.0 < max_move <= FRAME_FREE_MAX_MOVE:
        raise ValueError('max_move must lie in (0, %g] pixels' % FRAME_FREE_MAX_MOVE)
    min_snr = number('min_snr', min_snr)
    if not min_snr >= 0.0:
        raise ValueError('min_snr must be >= 0')
    return max_outer, pos_tol, max_step, max_move, min_snr


def frame_fit_arguments(image, var, psf, psf_index, origin, shift, scale0, radius, background, max_iter, tol, dimpsf=40):
    """(image, var or None, psf, psf_index, origin, shift, scale0 or None, radius, flags, max_iter, tol) of a host frame
    fit, validated as mpsfr_fit_frame_psf validates host arguments (ValueError), in this order: the frame as
    frame_images, origin as star_origins, the star count, psf, psf_index and shift as psf_fit_arguments, the
    parameters, scale0 n finite values or None."""
    im, va = frame_images(image, var)
    og = star_origins(origin)
    n = frame_fit_stars(og.shape[0])
    ps, ix, sh, _ = psf_fit_arguments(n, psf, psf_index, shift, True, False, dimpsf)
    radius, flags, max_iter, tol = frame_fit_parameters(radius, background, max_iter, tol)
    s0 = None if scale0 is None else star_scales('scale0', scale0, n)
    return im, va, ps, ix, og, sh, s0, radius, flags, max_iter, tol


def cube_fit_layers(nl):
    """The number of layers of a cube fit: an integer in 1 .. CUBE_FIT_MAX_LAYERS (ValueError)."""
    return integer('nl', nl, 1, CUBE_FIT_MAX_LAYERS, 'a cube has %(lo)d to %(hi)d layers, not %(n)r')


def cube_fit_batch(layer_batch):
    """layer_batch of a cube fit: an integer >= 0 (ValueError)."""
    return integer('layer_batch', layer_batch, 0, INT_MAX, 'layer_batch must be an integer, 0 or above')


def cube_fit_arguments(cube, var, psf, psf_index, origin, shift, layer_shift, scale0, radius, background, max_iter, tol,
                       layer_batch, dimpsf=40):
    """(cube, var or None, psf, psf_index, origin, shift, layer_shift or None, scale0 or None, radius, flags, max_iter,
    tol, layer_batch) of a host cube fit, validated as mpsfr_fit_cube_psf validates host arguments (ValueError): every
    layer of cube and var a frame of frame_images (a masked array is filled with NaN, anything else with `.data` is
    unwrapped), 1 .. CUBE_FIT_MAX_LAYERS of them; psf a numeric (npsf, nl, dimpsf, dimpsf) array (`.data` unwrapped,
    not filled); origin, psf_index, shift, radius, background, max_iter and tol as frame_fit_arguments takes them;
    layer_shift None or (nl, 2) finite values that keep every shift[k] + layer_shift[l] within FIT_PSF_MAX_SHIFT;
    scale0 None or (nl, n) finite values; layer_batch an integer >= 0."""
    cu = array('cube', cube, fill=True, unwrap=True)
    if cu.ndim != 3 or cu.size == 0:
        raise ValueError('cube must have the shape (nl, ny, nx)')
    nl = cube_fit_layers(cu.shape[0])
    va = None
    if var is not None:
        va = array('var', var, fill=True, unwrap=True)
        if va.shape != cu.shape:
            raise ValueError('var must have the shape of cube')
    ps = array('psf', psf, unwrap=True)
    if ps.ndim != 4 or ps.shape[1:] != (nl, dimpsf, dimpsf) or ps.size == 0:
        raise ValueError('psf must have the shape (npsf, %d, %d, %d)' % (nl, dimpsf, dimpsf))
    # one layer through the frame fit's own validation: the frame, the stars, the model list, the parameters
    _, _, _, ix, og, sh, _, radius, flags, max_iter, tol = frame_fit_arguments(
        cu[0], None if va is None else va[0], ps[:, 0], psf_index, origin, shift, None, radius, background, max_iter, tol,
        dimpsf)
    n = og.shape[0]
    ls = None
    if layer_shift is not None:
        ls = array('layer_shift', layer_shift)
        if ls.shape != (nl, 2):
            raise ValueError('layer_shift must have the shape (%d, 2)' % nl)
        if not np.all(np.isfinite(ls)):
            raise ValueError('layer_shift must be finite')
        total = ls[:, None, :] if sh is None else sh[None, :, :] + ls[:, None, :]
        if not np.all(np.abs(total) <= FIT_PSF_MAX_SHIFT):
            raise ValueError('shift + layer_shift must stay within %g pixels' % FIT_PSF_MAX_SHIFT)
        ls = np.ascontiguousarray(ls)
    s0 = None
    if scale0 is not None:
        s0 = array('scale0', scale0)
        if s0.shape != (nl, n):
            raise ValueError('scale0 must have the shape (%d, %d)' % (nl, n))
        if not np.all(np.isfinite(s0)):
            raise ValueError('scale0 must be finite')
        s0 = np.ascontiguousarray(s0)
    layer_batch = cube_fit_batch(layer_batch)
    return (np.ascontiguousarray(cu), None if va is None else np.ascontiguousarray(va), np.ascontiguousarray(ps), ix, og,
            sh, ls, s0, radius, flags, max_iter, tol, layer_batch)


def cube_free_work(nl, ny, nx, nstar):
    """The bytes of work memory of a cube fit with free positions, as mpsfr_fit_cube_psf_free counts them (include/
    mpsfr.h): render's lists once, per layer two frames and the per-layer vectors, the joint ones once.  Above
    CUBE_FREE_WORK_BYTES: ValueError, as C refuses the call."""
    def up(at, align):
        return (at + align - 1) // align * align
    nl, ny, nx, n = int(nl), int(ny), int(nx), int(nstar)
    nt = ((ny + 31) // 32) * ((nx + 31) // 32)
    npix, nchunk = ny * nx, (ny * nx + 4095) // 4096
    at = 4 * (nt + nt + nt + 1 + n + 9 * n)                                   # the renderer's lists (int32)
    at = up(at, 8) + 8 * (nl * (2 * npix + 25 * n + 8 * nchunk + 17) + 14 * n + 10)
    at += 4 * (nl * (4 * n + 5) + 5 * n + 11)
    if at > CUBE_FREE_WORK_BYTES:
        raise ValueError('%d layers of %d x %d pixels and %d stars need %d bytes of work memory, above the budget of '
                         '%d: take the positions from fewer layers' % (nl, ny, nx, n, at, CUBE_FREE_WORK_BYTES))
    return at


def cube_free_arguments(cube, var, psf, psf_index, origin, shift, layer_shift, scale0, radius, background, max_iter, tol,
                        max_outer, pos_tol, max_step, max_move, min_snr, dimpsf=40):
    """(cube, var or None, psf, psf_index, origin, shift, layer_shift or None, scale0 or None, radius, flags, max_iter,
    tol, (max_outer, pos_tol, max_step, max_move, min_snr)) of a host cube fit with free positions, validated as
    mpsfr_fit_cube_psf_free validates host arguments (ValueError): the arrays as cube_fit_arguments, the outer loop as
    frame_free_parameters, the work memory as cube_free_work, counted from the shapes before any array is made."""
    shape, nstar = np.shape(getattr(cube, 'data', cube)), np.shape(origin)[:1]
    if len(shape) == 3 and nstar and all(0 < v < 1 << 24 for v in shape + nstar):
        cube_free_work(shape[0], shape[1], shape[2], nstar[0])               # (before any array of that size is made)
    cu, va, ps, ix, og, sh, ls, s0, radius, flags, max_iter, tol, _ = cube_fit_arguments(
        cube, var, psf, psf_index, origin, shift, layer_shift, scale0, radius, background, max_iter, tol, 0, dimpsf)
    free = frame_free_parameters(max_outer, pos_tol, max_step, max_move, min_snr)
    cube_free_work(cu.shape[0], cu.shape[1], cu.shape[2], og.shape[0])
    return cu, va, ps, ix, og, sh, ls, s0, radius, flags, max_iter, tol, free


# What `from ._args import *` hands to _lib.py, where every limit, validator and helper stays reachable as _lib.NAME
# (the helpers with a leading underscore too): not NumPy, and not the primitives, which a user of them imports by name.
__all__ = [n for n in dir() if not n.startswith('__') and n not in ('np', 'integer', 'number', 'flag', 'array',
                                                                    'stamp_stack')]
