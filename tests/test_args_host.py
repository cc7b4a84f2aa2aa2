"""Host: the argument rules of muse_psfr_amd/_args.py, of the Context methods in front of them and of the checks of
psfrec.py that use the same primitives, as two tables.

REFUSALS: (callable, args, keyword args, the exact message); every `raise` of _args.py, every ValueError a Context
method raises itself and every check of psfrec.py built on the primitives has at least one row, the ends of every
range a value inside and one outside, and the rows marked `order` give two bad arguments and pin which is reported.
ACCEPTED / EXPECTED: (callable, args, keyword args) and the full result as literals -- describe() below: arrays as
(dtype, shape, C-contiguous, values), scalars with their Python type.  A Context is the stub of test_lib_calls_host.py
(no library, no GPU).

Where the expectations come from.  Every row that calls a name the package had before the argument rules moved into
_args.py -- the validators, the Context methods, the public functions of psfrec.py, _positive_int, _device_pointers,
_group_size, _spec_layers, _grid_or_positions, _shift_pixels, _sky_parameters, _check_circular -- was recorded from
those modules as they were, not from _args.py, and passes against them unchanged.  The rows that call a name which is
new cannot have been: integer, number, flag, array, stamp_stack, grid_side, _model_per_star and _frame_fit_device of
_args.py, _check_precision, _grid_or_field and _two_layer_atmosphere of psfrec.py, and test_no_copy, which begins with
array.  Their messages are the existing ones the primitives took over, letter for letter, and their accepted results
were written from what the replaced in-line code returned (int, float, the flag itself, a float64 array)."""
import numpy as np
import pytest

from muse_psfr_amd import _args as A
from muse_psfr_amd import psfrec as P
from test_lib_calls_host import make_ctx

NAN, INF = float('nan'), float('inf')
ST = np.array([[1.0, 2.0], [3.0, 4.0]])                       # one stamp of dimpsf = 2
ST2 = np.arange(8.0).reshape(2, 2, 2)
MASKED = np.ma.array([[1.0, 2.0], [3.0, 4.0]], mask=[[False, True], [False, False]])
BIG = np.arange(1600.0).reshape(40, 40)                       # a single (40, 40) stamp
Z40 = np.zeros((1, 40, 40))
FRAME = np.arange(12.0).reshape(3, 4)
CUBE = np.arange(18.0).reshape(2, 3, 3)
CPSF = np.ones((1, 2, 2, 2))                                  # (npsf, nl, 2, 2) models of CUBE
CORE = np.arange(16.0).reshape(4, 4)                          # a model stamp of dimpsf = 4
HUGE = np.broadcast_to(np.zeros(1), (600, 4096, 4096))        # 80 GB if it were ever copied
LB3 = [500.0, 600.0, 700.0]


class Holder:
    """An object with a .data attribute (an mpdaf-style cube)."""

    def __init__(self, data):
        self.data = data


def C(name):
    """The method `name` of a fresh stub Context."""
    def call(*args, **kwargs):
        return getattr(make_ctx(), name)(*args, **kwargs)
    call.__name__ = 'Context.' + name
    return call


def R(fn, message, *args, **kwargs):
    return fn, args, kwargs, message


def frame_fit(image=FRAME, var=None, psf=ST, psf_index=None, origin=((0, 0),), shift=None, scale0=None, radius=8.0,
              background=True, max_iter=100, tol=1e-10):
    return A.frame_fit_arguments(image, var, psf, psf_index, origin, shift, scale0, radius, background, max_iter, tol, 2)


def cube_fit(cube=CUBE, var=None, psf=CPSF, psf_index=None, origin=((0, 0),), shift=None, layer_shift=None, scale0=None,
             layer_batch=0):
    return A.cube_fit_arguments(cube, var, psf, psf_index, origin, shift, layer_shift, scale0, 8.0, True, 100, 1e-10,
                                layer_batch, 2)


def cube_free(cube=CUBE, origin=((0, 0),), max_outer=8):
    return A.cube_free_arguments(cube, None, CPSF, None, origin, None, None, None, 8.0, True, 100, 1e-10, max_outer,
                                 1e-3, 0.5, 2.0, 3.0, 2)


def frame_dev(ny=8, nx=8, image_ptr=1, nstar=2, npsf=2, psf_ptr=2, origin_ptr=3, star_out_ptr=4, head_ptr=5, **kw):
    return C('fit_frame_psf_device')(ny, nx, image_ptr, nstar, npsf, psf_ptr, origin_ptr, star_out_ptr, head_ptr, **kw)


def free_dev(nstar=2, npsf=2, shift_out_ptr=6, **kw):
    return C('fit_frame_psf_free_device')(8, 8, 1, nstar, npsf, 2, 3, 4, shift_out_ptr, 5, **kw)


def cube_dev(nl=2, nstar=2, npsf=2, head_ptr=5, **kw):
    return C('fit_cube_psf_device')(nl, 8, 8, 1, nstar, npsf, 2, 3, 4, head_ptr, **kw)


def cube_free_dev(nl=2, ny=8, nx=8, nstar=2, npsf=2, call_ptr=8, **kw):
    return C('fit_cube_psf_free_device')(nl, ny, nx, 1, nstar, npsf, 2, 3, 4, 5, 6, 7, call_ptr, **kw)


def crowded(psf=Z40, positions=((5.0, 5.0),), **kw):
    return P.fit_crowded_stars(np.zeros((8, 8)), psf, positions, **kw)


def crowded_spectra(psf=np.zeros((2, 40, 40)), **kw):
    return P.fit_crowded_spectra(np.zeros((2, 8, 8)), psf, ((5.0, 5.0),), **kw)


def found_stars(psf=BIG, **kw):
    return P.fit_found_stars(np.zeros((8, 8)), psf, ((5.0, 5.0),), crit=2.0, **kw)


def field_psf(seeing=1.0, GL=0.7, L0=25.0, **kw):
    return P.compute_field_psf(LB3, seeing, GL, L0, verbose=False, **kw)


def band_psf(seeing=1.0, GL=0.7, L0=25.0, **kw):
    return P.compute_band_psf(LB3, seeing, GL, L0, [(500.0, 700.0)], verbose=False, **kw)


def profile_psf(**kw):
    return P.compute_profile_psf(LB3, 1.0, 25.0, [0.7, 0.3], (100.0, 10000.0), verbose=False, **kw)


INT15 = 'n must be an integer between 1 and 5'
NUM = 'v must be a finite number'
FLAG = 'f must be True or False'
NPSFLIN = 'npsflin must be an integer between 1 and 5'
PRECISION = "precision must be 'mixed' or 'f64'"
SCALARS = 'seeing, GL and L0 must be scalars'
GROUP1 = 'a group has 2 to 4 sources (one source is fit_stamps_psf), not 1'
SHIFT8 = 'shift must be finite and within 8 pixels'
RADIUS = 'radius must lie between 1 and 20 pixels'
CRIT = 'crit must be a number above 0 and at most 16 pixels'
FILTER = 'filter must be 1, 3 or 5'
NSTAR_EQ = 'without psf_index_ptr, npsf must equal nstar'
NSTAMP_EQ = 'without psf_index_ptr, npsf must equal nstamp'
WORK = ('600 layers of 4096 x 4096 pixels and 1 stars need 161218980112 bytes of work memory, above the budget of '
        '4294967296: take the positions from fewer layers')

REFUSALS = [
    # ---- the primitives
    R(A.integer, INT15, 'n', True, 1, 5), R(A.integer, INT15, 'n', 0, 1, 5), R(A.integer, INT15, 'n', 6, 1, 5),
    R(A.integer, INT15, 'n', 2.0, 1, 5), R(A.integer, INT15, 'n', '3', 1, 5), R(A.integer, INT15, 'n', np.float64(3), 1, 5),
    R(A.integer, INT15, 'n', np.True_, 1, 5), R(A.integer, INT15, 'n', np.array([3]), 1, 5),
    R(A.integer, 'its own words', 'n', 9, 1, 5, 'its own words'),
    R(A.integer, 'n takes 1 to 5, not 9', 'n', 9, 1, 5, '%(name)s takes %(lo)d to %(hi)d, not %(n)r'),
    R(A.number, NUM, 'v', True), R(A.number, NUM, 'v', np.True_), R(A.number, NUM, 'v', np.array(1.0)),
    R(A.number, NUM, 'v', 'x'), R(A.number, NUM, 'v', None), R(A.number, NUM, 'v', NAN), R(A.number, NUM, 'v', INF),
    R(A.number, NUM, 'v', -INF), R(A.number, NUM, 'v', np.float32('nan')), R(A.number, NUM, 'v', [1.0]),
    R(A.flag, FLAG, 'f', 1), R(A.flag, FLAG, 'f', 0.0), R(A.flag, FLAG, 'f', None), R(A.flag, FLAG, 'f', 'True'),
    R(A.flag, FLAG, 'f', np.array([True])),
    R(A.array, 'a must be a numeric array', 'a', 'abc'), R(A.array, 'a must be a numeric array', 'a', [[1, 2], [3]]),
    R(A.array, 'a must be a numeric array', 'a', [1.0, 'x']), R(A.array, 'a must be a numeric array', 'a', object()),
    R(A.array, 'a must be a numeric array', 'a', Holder('abc'), unwrap=True),
    R(A.stamp_stack, 's must have the shape (..., 2, 2)', 's', np.zeros(3), 2),
    R(A.stamp_stack, 's must have the shape (..., 2, 2)', 's', np.zeros((0, 2, 2)), 2),
    R(A.stamp_stack, 's must have the shape (..., 2, 2)', 's', np.zeros((2, 3)), 2),
    R(A.stamp_stack, 's must be a numeric array', 's', 'abc', 2),
    # ---- counts and pointers
    R(A._positive_int, 'nstamp must be a positive integer', 'nstamp', 0),
    R(A._positive_int, 'nstamp must be a positive integer', 'nstamp', True),
    R(A._positive_int, 'nstamp must be a positive integer', 'nstamp', 1.0),
    R(A._device_pointers, 'a_ptr and b_ptr must be device pointers', a_ptr=1, b_ptr=0),
    R(A._device_pointers, 'a_ptr, b_ptr and c_ptr must be device pointers', a_ptr=None, b_ptr=2, c_ptr=3),
    R(A._model_per_star, NSTAR_EQ, 3, 2, None), R(A._model_per_star, NSTAR_EQ, 3, 2, 0),
    R(A._model_per_star, NSTAMP_EQ, 1, 2, None, 'nstamp'),
    R(A._group_size, GROUP1, 1), R(A._group_size, GROUP1.replace('not 1', 'not 5'), 5),
    R(A._group_size, GROUP1.replace('not 1', 'not True'), True),
    R(A._spec_layers, 'a star cube has 1 to 4096 layers, not 0', 0),
    R(A._spec_layers, 'a star cube has 1 to 4096 layers, not 4097', 4097),
    R(A._spec_layers, 'a star cube has 1 to 4096 layers, not 2.0', 2.0),
    # ---- the reconstruct calls
    R(A.field_positions, 'positions must be an (n, 2) array of (x, y) in arcsec', 'abc'),
    R(A.field_positions, 'positions must be an (n, 2) array of (x, y) in arcsec, got shape (3,)', [1, 2, 3]),
    R(A.field_positions, 'positions must not be empty', np.zeros((0, 2))),
    R(A.field_positions, 'at most 25 positions per call, got 26', np.zeros((26, 2))),
    R(A.field_positions, 'at most 1 positions per call, got 2', np.zeros((2, 2)), 1),
    R(A.field_positions, 'positions must be finite', [[NAN, 0.0]]),
    R(A.field_positions, 'positions must be finite', [[0.0, INF]]),
    R(A.field_positions, 'positions must satisfy |x|, |y| <= 60 arcsec', [[60.5, 0.0]]),
    R(A.field_positions, 'positions must satisfy |x|, |y| <= 60 arcsec', [[0.0, -61.0]]),
    R(A.grid_side, NPSFLIN, True), R(A.grid_side, NPSFLIN, 0), R(A.grid_side, NPSFLIN, 6), R(A.grid_side, NPSFLIN, 2.0),
    R(A._grid_or_positions, NPSFLIN, 0, None),
    R(A._grid_or_positions, 'a call with positions takes npsflin = 0', 2, [[0.0, 0.0]]),
    R(A.profile_layers, 'h, wind_speed and wind_dir must be numeric', 'a', 1.0, 1.0),
    R(A.profile_layers, 'a profile has 1 to 8 layers, got 9', np.zeros(9), 1.0, np.zeros(9)),
    R(A.profile_layers, 'a profile has 1 to 8 layers, got 0', [], 1.0, []),
    R(A.profile_layers, 'h, wind_speed and wind_dir need one value per layer (2)', [0.0, 1.0], [1.0, 2.0, 3.0], [0.0, 0.0]),
    R(A.profile_layers, 'h, wind_speed and wind_dir need one value per layer (2)', [0.0, 1.0], 1.0, [0.0]),
    R(A.profile_layers, 'altitudes and winds must be finite', [NAN], 1.0, [0.0]),
    R(A.profile_layers, 'altitudes and winds must be finite', [0.0], INF, [0.0]),
    R(A.profile_layers, 'altitudes and winds must be finite', [0.0], 1.0, [NAN]),
    R(A.profile_layers, 'layer altitudes must lie in [0, 50000] m', [-1.0], 1.0, [0.0]),
    R(A.profile_layers, 'layer altitudes must lie in [0, 50000] m', [50001.0], 1.0, [0.0]),
    R(A.profile_layers, 'wind speeds must lie in [0, 100] m/s', [0.0], 100.5, [0.0]),
    R(A.profile_layers, 'wind speeds must lie in [0, 100] m/s', [0.0], -0.5, [0.0]),
    R(A.profile_weights, 'cn2 must be numeric', 'a', 1, 1),
    R(A.profile_weights, 'cn2 must be (2,) or (1, 2), got shape (3,)', [1.0, 2.0, 3.0], 1, 2),
    R(A.profile_weights, 'cn2 must be (2,) or (3, 2), got shape (2, 2)', np.ones((2, 2)), 3, 2),
    R(A.profile_weights, 'Cn2 weights must be finite and >= 0', [1.0, -1.0], 1, 2),
    R(A.profile_weights, 'Cn2 weights must be finite and >= 0', [1.0, NAN], 1, 2),
    R(A.profile_weights, 'every row of Cn2 weights needs a positive sum', [0.0, 0.0], 1, 2),
    R(A.band_weight_matrix, 'band weights must be numeric', 'a', 3),
    R(A.band_weight_matrix, 'band weights must be (nband, 3), got shape (2,)', [1.0, 2.0], 3),
    R(A.band_weight_matrix, '1 to 16 bands per call, got 17', np.ones((17, 3)), 3),
    R(A.band_weight_matrix, '1 to 16 bands per call, got 0', np.ones((0, 3)), 3),
    R(A.band_weight_matrix, 'band weights must be finite and >= 0', [[1.0, -1.0, 0.0]], 3),
    R(A.band_weight_matrix, 'band weights must be finite and >= 0', [[1.0, INF, 0.0]], 3),
    R(A.band_weight_matrix, 'every band needs a positive sum of weights', [[0.0, 0.0, 0.0]], 3),
    # ---- the stamp family
    R(A.elliptical_stamps, 'stamps must be a numeric array', 'abc', 2),
    R(A.elliptical_stamps, 'stamps must have the shape (..., 2, 2)', np.zeros((2, 3)), 2),
    R(A.elliptical_stamps, 'stamps must be finite', [[1.0, NAN], [0.0, 0.0]], 2),
    R(A.elliptical_stamps, 'stamps must be finite', [[1.0, INF], [0.0, 0.0]], 2),
    R(A.observed_flags, 'background must be True or False', 1, True),
    R(A.observed_flags, 'circular must be True or False', True, 0),
    R(A.observed_flags, 'background must be True or False', 1, 0),                                  # order
    R(A.observed_stamps, 'stamps must be a numeric array', 'abc', None, 2),
    R(A.observed_stamps, 'stamps must have the shape (..., 2, 2)', np.zeros(4), None, 2),
    R(A.observed_stamps, 'var must be a numeric array', ST, 'abc', 2),
    R(A.observed_stamps, 'var must have the shape of stamps', ST, np.zeros(3), 2),
    R(A.observed_stamps, 'var must have the shape of stamps', ST2, ST, 2),
    R(A.observed_stamps, 'stamps must be a numeric array', Holder(ST), None, 2),       # fills, does not unwrap .data
    R(A.observed_stamps, 'var must be a numeric array', ST, Holder(ST), 2),
    R(A.psf_fit_flags, 'background must be True or False', None, False),
    R(A.psf_fit_flags, 'fixed_shift must be True or False', True, 1),
    R(A.psf_fit_arguments, 'psf must be a numeric array', 1, 'abc', None, None, True, False, 2),
    R(A.psf_fit_arguments, 'psf must have the shape (..., 2, 2)', 1, np.zeros((2, 3)), None, None, True, False, 2),
    R(A.psf_fit_arguments, 'without psf_index there must be one model stamp per star (2), got 1', 2, ST, None, None, True,
      False, 2),
    R(A.psf_fit_arguments, 'psf_index must be an integer array', 1, ST, 'abc', None, True, False, 2),
    R(A.psf_fit_arguments, 'psf_index must hold one integer per star', 2, ST, [0.0, 0.0], None, True, False, 2),
    R(A.psf_fit_arguments, 'psf_index must hold one integer per star', 2, ST, [True, False], None, True, False, 2),
    R(A.psf_fit_arguments, 'psf_index must hold one integer per star', 2, ST, [0], None, True, False, 2),
    R(A.psf_fit_arguments, 'psf_index must lie in 0..0', 2, ST, [0, 1], None, True, False, 2),
    R(A.psf_fit_arguments, 'psf_index must lie in 0..1', 2, ST2, [-1, 0], None, True, False, 2),
    R(A.psf_fit_arguments, 'fixed_shift needs the shift array', 1, ST, None, None, True, True, 2),
    R(A.psf_fit_arguments, 'shift must be a numeric array', 1, ST, None, 'abc', True, False, 2),
    R(A.psf_fit_arguments, 'shift must have the shape (2, 2)', 2, ST2, None, [1.0, 2.0, 3.0], True, False, 2),
    R(A.psf_fit_arguments, 'shift must have the shape (1, 2)', 1, ST, None, [[1.0], [2.0]], True, False, 2),
    R(A.psf_fit_arguments, SHIFT8, 1, ST, None, [[NAN, 0.0]], True, False, 2),
    R(A.psf_fit_arguments, SHIFT8, 1, ST, None, [[0.0, INF]], True, False, 2),
    R(A.psf_fit_arguments, SHIFT8, 1, ST, None, [[0.0, -8.5]], True, False, 2),
    R(A.psf_fit_arguments, 'background must be True or False', 1, 'abc', None, None, 1, False, 2),     # order
    R(A.group_fit_flags, 'background must be True or False', 1, 'free'),
    R(A.group_fit_flags, "mode must be 'free', 'common' or 'fixed'", True, 'x'),
    R(A.group_fit_flags, "mode must be 'free', 'common' or 'fixed'", True, 1),
    R(A.group_fit_arguments, 'a group fit needs the positions of its sources (shift)', 1, ST, None, None, True, 'free', 2),
    R(A.group_fit_arguments, 'shift must be a numeric array', 1, ST, None, 'abc', True, 'free', 2),
    R(A.group_fit_arguments, 'shift must have the shape (1, K, 2)', 1, ST, None, [[1.0, 2.0, 3.0]], True, 'free', 2),
    R(A.group_fit_arguments, GROUP1, 1, ST, None, np.zeros((1, 1, 2)), True, 'free', 2),
    R(A.group_fit_arguments, GROUP1.replace('not 1', 'not 5'), 1, ST, None, np.zeros((1, 5, 2)), True, 'free', 2),
    R(A.group_fit_arguments, 'the positions must be finite and within 8 pixels', 1, ST, None, [[[NAN, 0.0], [0.0, 0.0]]],
      True, 'free', 2),
    R(A.group_fit_arguments, 'the positions must be finite and within 8 pixels', 1, ST, None, [[[8.5, 0.0], [0.0, 0.0]]],
      True, 'free', 2),
    R(A.spectra_fit_flags, 'background must be True or False', 1, None, 2),
    R(A.spectra_fit_flags, 'x must be a numeric array', True, 'abc', 2),
    R(A.spectra_fit_flags, 'the drift needs at least two layers and one x per layer (1)', True, [0.0], 1),
    R(A.spectra_fit_flags, 'the drift needs at least two layers and one x per layer (3)', True, [0.0, 1.0], 3),
    R(A.spectra_fit_flags, 'x must be finite and lie in [-1, 1]', True, [0.0, 1.5], 2),
    R(A.spectra_fit_flags, 'x must be finite and lie in [-1, 1]', True, [0.0, NAN], 2),
    R(A.spectra_fit_flags, 'at least two values of x must differ', True, [0.5, 0.5], 2),
    R(A.spectra_fit_arguments, 'cubes must have the shape (n, nl, 2, 2)', ST, None, ST2, None, None, True, None, 2),
    R(A.spectra_fit_arguments, 'cubes must have the shape (n, nl, 2, 2)', [[1, 2], [3]], None, ST2, None, None, True, None, 2),
    R(A.spectra_fit_arguments, 'psf must be a numeric array', ST2, None, [[1, 2], [3]], None, None, True, None, 2),
    R(A.spectra_fit_arguments, 'psf must have the shape (npsf, 2, 2, 2)', ST2, None, ST, None, None, True, None, 2),
    R(A.spectra_fit_arguments, 'psf must have the shape (npsf, 2, 2, 2)', ST2, None, np.zeros((3, 2, 2)), None, None, True,
      None, 2),
    R(A.metric_stamps, 'stamps must be a numeric array', 'abc', 2),
    R(A.metric_stamps, 'stamps must have the shape (..., 2, 2)', np.zeros((3, 2)), 2),
    R(A.metric_parameters, 'radii must be numbers', 'abc', None, None, 2),
    R(A.metric_parameters, 'boxes must be a 1-D sequence of at most 16 values', None, [[1.0, 2.0]], None, 2),
    R(A.metric_parameters, 'fractions must be a 1-D sequence of at most 16 values', None, None, np.full(17, 0.5), 2),
    R(A.metric_parameters, 'need at least one radius, box or fraction', None, None, None, 2),
    R(A.metric_parameters, 'radii must be finite, > 0 and at most 4 pixels', [0.0], None, None, 2),
    R(A.metric_parameters, 'radii must be finite, > 0 and at most 4 pixels', [4.5], None, None, 2),
    R(A.metric_parameters, 'radii must be finite, > 0 and at most 4 pixels', [INF], None, None, 2),
    R(A.metric_parameters, 'boxes must be finite, > 0 and at most 4 pixels', None, [NAN], None, 2),
    R(A.metric_parameters, 'fractions must lie in (0, 1)', None, None, [1.0], 2),
    R(A.metric_parameters, 'fractions must lie in (0, 1)', None, None, [0.0], 2),
    R(A.metric_parameters, 'fractions must lie in (0, 1)', None, None, [NAN], 2),
    R(A.metric_centers, 'centers must be an (n, 2) array of (p, q) in pixels', 'abc', 1),
    R(A.metric_centers, 'centers must have the shape (2, 2): one (p, q) per stamp', [[1.0, 2.0]], 2),
    R(A.metric_centers, 'centers must be finite, with |p| and |q| at most 100 pixels', [[NAN, 0.0]], 1),
    R(A.metric_centers, 'centers must be finite, with |p| and |q| at most 100 pixels', [[0.0, INF]], 1),
    R(A.metric_centers, 'centers must be finite, with |p| and |q| at most 100 pixels', [[-100.5, 0.0]], 1),
    # ---- the frame calls
    R(A.frame_shape, 'ny must be an integer between 1 and 16384', 0, 1),
    R(A.frame_shape, 'ny must be an integer between 1 and 16384', True, 1),
    R(A.frame_shape, 'ny must be an integer between 1 and 16384', 16385, 1),
    R(A.frame_shape, 'nx must be an integer between 1 and 16384', 1, 16385),
    R(A.frame_shape, 'nx must be an integer between 1 and 16384', 1, 2.0),
    R(A.frame_shape, 'ny must be an integer between 1 and 16384', 0, 0),                                # order
    R(A.frame_shape, 'a frame holds at most 2^26 pixels', 16384, 16384),
    R(A.frame_shape, 'a frame holds at most 2^26 pixels', 8192, 8193),
    R(A.frame_images, 'image must be a numeric array', 'abc'),
    R(A.frame_images, 'image must have the shape (ny, nx)', np.zeros(3)),
    R(A.frame_images, 'image must have the shape (ny, nx)', np.zeros((0, 3))),
    R(A.frame_images, 'var must be a numeric array', FRAME, 'abc'),
    R(A.frame_images, 'var must have the shape of image', FRAME, np.zeros((4, 3))),
    R(A.frame_images, 'image must be a numeric array', Holder(FRAME)),                  # fills, does not unwrap .data
    R(A.frame_images, 'var must be a numeric array', FRAME, Holder(FRAME)),
    R(A.star_origins, 'origin must be an integer array', 'abc'),
    R(A.star_origins, 'origin must be an integer array of shape (n, 2)', [[1.0, 2.0]]),
    R(A.star_origins, 'origin must be an integer array of shape (n, 2)', [1, 2]),
    R(A.star_origins, 'origin must be an integer array of shape (n, 2)', np.zeros((0, 2), dtype=np.int64)),
    R(A.star_origins, 'origin must have the shape (2, 2)', [[1, 2]], 2),
    R(A.star_origins, 'origin must lie within 2^30 pixels', [[(1 << 30) + 1, 0]]),
    R(A.star_origins, 'origin must lie within 2^30 pixels', [[0, -(1 << 30) - 1]]),
    R(A.render_flags, 'subtract must be True or False', 1),
    R(A.star_scales, 'scale must be a numeric array', 'scale', 'abc', 1),
    R(A.star_scales, 'scale must hold one value per star (1)', 'scale', [1.0, 2.0], 1),
    R(A.star_scales, 'scale0 must hold one value per star (1)', 'scale0', [[1.0]], 1),
    R(A.star_scales, 'scale must be finite', 'scale', [NAN], 1),
    R(A.star_scales, 'scale must be finite', 'scale', [-INF], 1),
    R(A.render_arguments, 'subtract needs the image', ST, [[0, 0]], [1.0], None, None, None, (3, 4), True, 2),
    R(A.render_arguments, 'give the image or the shape of the frame', ST, [[0, 0]], [1.0], None, None, None, None, False, 2),
    R(A.render_arguments, 'shape must be (ny, nx)', ST, [[0, 0]], [1.0], None, None, None, 5, False, 2),
    R(A.render_arguments, 'shape must be (ny, nx)', ST, [[0, 0]], [1.0], None, None, None, (1, 2, 3), False, 2),
    R(A.render_arguments, 'ny must be an integer between 1 and 16384', ST, [[0, 0]], [1.0], None, None, None, (0, 3), False, 2),
    R(A.render_arguments, 'shape differs from the shape of image', ST, [[0, 0]], [1.0], None, None, FRAME, (3, 5), False, 2),
    R(A.render_arguments, 'subtract must be True or False', ST, 'abc', [1.0], None, None, None, None, 1, 2),   # order
    R(A.render_arguments, 'origin must be an integer array', ST, 'abc', [NAN], None, None, None, None, False, 2),   # order
    R(A.find_parameters, 'half must be an integer between 1 and 8', 0, 1, 5.0, 10, 40),
    R(A.find_parameters, 'half must be an integer between 1 and 8', 9, 1, 5.0, 10, 40),
    R(A.find_parameters, 'half must be an integer between 1 and 2', 3, 1, 5.0, 10, 4),
    R(A.find_parameters, 'sep must be an integer between 1 and 16', 1, 17, 5.0, 10, 40),
    R(A.find_parameters, 'sep must be an integer between 1 and 16', 1, 0, 5.0, 10, 40),
    R(A.find_parameters, 'max_stars must be an integer between 1 and 16777216', 1, 1, 5.0, 0, 40),
    R(A.find_parameters, 'max_stars must be an integer between 1 and 16777216', 1, 1, 5.0, (1 << 24) + 1, 40),
    R(A.find_parameters, 'threshold must be a finite number', 1, 1, NAN, 10, 40),
    R(A.find_parameters, 'threshold must be a finite number', 1, 1, INF, 10, 40),
    R(A.find_parameters, 'threshold must be a finite number', 1, 1, True, 10, 40),
    R(A.find_parameters, 'threshold must be a finite number', 1, 1, np.array(5.0), 10, 40),
    R(A.find_parameters, 'threshold must be a finite number', 1, 1, '5', 10, 40),
    R(A.find_parameters, 'half must be an integer between 1 and 8', 0, 1, NAN, 10, 40),                 # order
    R(A.find_parameters, 'max_stars must be an integer between 1 and 16777216', 1, 1, NAN, 0, 40),      # order
    R(A.find_arguments, 'psf must be a numeric array', FRAME, None, 'abc', 1, 1, 5.0, 10, 4),
    R(A.find_arguments, 'psf must be one model stamp of shape (4, 4)', FRAME, None, np.zeros((3, 3)), 1, 1, 5.0, 10, 4),
    R(A.find_arguments, 'psf must be one model stamp of shape (4, 4)', FRAME, None, 3.0, 1, 1, 5.0, 10, 4),
    R(A.find_arguments, 'psf must be finite over its core', FRAME, None, np.full((4, 4), NAN), 1, 1, 5.0, 10, 4),
    R(A.find_arguments, 'psf must not be constant over its core', FRAME, None, np.ones((4, 4)), 1, 1, 5.0, 10, 4),
    R(A.background_parameters, 'box must be an integer between 8 and 64', 7, 3, 3.0, 5, 0.25),
    R(A.background_parameters, 'box must be an integer between 8 and 64', 65, 3, 3.0, 5, 0.25),
    R(A.background_parameters, 'box must be an integer between 8 and 64', True, 3, 3.0, 5, 0.25),
    R(A.background_parameters, FILTER, 32, 2, 3.0, 5, 0.25), R(A.background_parameters, FILTER, 32, 4, 3.0, 5, 0.25),
    R(A.background_parameters, FILTER, 32, 0, 3.0, 5, 0.25), R(A.background_parameters, FILTER, 32, 6, 3.0, 5, 0.25),
    R(A.background_parameters, FILTER, 32, 7, 3.0, 5, 0.25), R(A.background_parameters, FILTER, 32, True, 3.0, 5, 0.25),
    R(A.background_parameters, FILTER, 32, 3.0, 3.0, 5, 0.25),
    R(A.background_parameters, 'max_clip must be an integer between 0 and 16', 32, 3, 3.0, -1, 0.25),
    R(A.background_parameters, 'max_clip must be an integer between 0 and 16', 32, 3, 3.0, 17, 0.25),
    R(A.background_parameters, 'kappa must be a finite number', 32, 3, 'x', 5, 0.25),
    R(A.background_parameters, 'kappa must be a finite number', 32, 3, NAN, 5, 0.25),
    R(A.background_parameters, 'kappa must be a finite number', 32, 3, INF, 5, 0.25),
    R(A.background_parameters, 'kappa must lie between 1 and 100', 32, 3, 0.5, 5, 0.25),
    R(A.background_parameters, 'kappa must lie between 1 and 100', 32, 3, 100.5, 5, 0.25),
    R(A.background_parameters, 'min_frac must be a finite number', 32, 3, 3.0, 5, NAN),
    R(A.background_parameters, 'min_frac must be a finite number', 32, 3, 3.0, 5, INF),
    R(A.background_parameters, 'min_frac must lie in (0, 1]', 32, 3, 3.0, 5, 0.0),
    R(A.background_parameters, 'min_frac must lie in (0, 1]', 32, 3, 3.0, 5, 1.5),
    R(A.background_parameters, 'box must be an integer between 8 and 64', 7, 2, NAN, 5, 0.25),                  # order
    R(A.background_parameters, 'max_clip must be an integer between 0 and 16', 32, 3, NAN, 99, 0.25),           # order
    R(A.background_shape, 'nl must be a positive integer', 0, 1, 1),
    R(A.background_shape, 'nx must be an integer between 1 and 16384', 1, 1, 0),
    R(A.background_shape, 'a background call holds at most 2^26 pixels', 2, 8192, 8192),
    R(A.background_arguments, 'image must be a numeric array', 'abc', None, None, 32, 3, 3.0, 5, 0.25),
    R(A.background_arguments, 'image must have the shape (ny, nx) or (nl, ny, nx)', np.zeros(3), None, None, 32, 3, 3.0, 5,
      0.25),
    R(A.background_arguments, 'var must have the shape of image', FRAME, np.zeros((4, 3)), None, 32, 3, 3.0, 5, 0.25),
    R(A.background_arguments, 'apply_to must have the shape of image', FRAME, None, np.zeros(3), 32, 3, 3.0, 5, 0.25),
    R(A.background_arguments, 'apply_to must be a numeric array', FRAME, None, 'abc', 32, 3, 3.0, 5, 0.25),
    R(A.background_arguments, 'image must be a numeric array', Holder(FRAME), None, None, 32, 3, 3.0, 5, 0.25),   # fills only
    R(A.background_arguments, 'var must be a numeric array', FRAME, Holder(FRAME), None, 32, 3, 3.0, 5, 0.25),
    R(A.find_arguments, 'psf must be a numeric array', FRAME, None, Holder(CORE), 1, 1, 5.0, 10, 4),   # neither fills nor unwraps
    R(A.group_parameters, 'nstar must be an integer between 1 and 16777216', 0, 2, 1.0, None),
    R(A.group_parameters, 'nstar must be an integer between 1 and 16777216', (1 << 24) + 1, 2, 1.0, None),
    R(A.group_parameters, 'stride must be an integer between 2 and 2147483647', 1, 1, 1.0, None),
    R(A.group_parameters, 'stride must be an integer between 2 and 2147483647', 1, 1 << 31, 1.0, None),
    R(A.group_parameters, 'max_groups must be an integer between 1 and 2147483647', 1, 2, 1.0, 0),
    R(A.group_parameters, 'max_groups must be an integer between 1 and 2147483647', 1, 2, 1.0, 1 << 31),
    R(A.group_parameters, CRIT, 1, 2, 0.0, None), R(A.group_parameters, CRIT, 1, 2, 16.5, None),
    R(A.group_parameters, CRIT, 1, 2, NAN, None), R(A.group_parameters, CRIT, 1, 2, INF, None),
    R(A.group_parameters, CRIT, 1, 2, True, None), R(A.group_parameters, CRIT, 1, 2, '1', None),
    R(A.group_parameters, CRIT, 1, 2, np.array(1.0), None),
    R(A.group_arguments, 'shape must be (ny, nx)', [[1.0, 1.0]], 1.0, 5),
    R(A.group_arguments, 'pos must be a numeric array', 'abc', 1.0, (4, 4)),
    R(A.group_arguments, 'pos must have the shape (nstar, stride) with nstar >= 1 and stride >= 2', np.zeros(3), 1.0, (4, 4)),
    R(A.group_arguments, 'pos must have the shape (nstar, stride) with nstar >= 1 and stride >= 2', np.zeros((2, 1)), 1.0,
      (4, 4)),
    R(A.group_arguments, 'a position lies outside [-1, ny] x [-1, nx]', [[-2.0, 0.0]], 1.0, (4, 4)),
    R(A.group_arguments, 'a position lies outside [-1, ny] x [-1, nx]', [[0.0, 4.5]], 1.0, (4, 4)),
    R(A.group_arguments, 'a position lies outside [-1, ny] x [-1, nx]', [[0.0, INF]], 1.0, (4, 4)),
    R(A.group_offsets, 'counts must hold the 6 counts of a group call', [1, 2]),
    # ---- the crowded-field fits
    R(A.frame_fit_stars, 'nstar must be an integer between 1 and 1048576', 0),
    R(A.frame_fit_stars, 'nstar must be an integer between 1 and 1048576', (1 << 20) + 1),
    R(A.frame_fit_stars, 'nstar must be an integer between 1 and 1048576', True),
    R(A.frame_fit_parameters, 'radius must be a finite number', NAN, True, 100, 1e-10),
    R(A.frame_fit_parameters, 'radius must be a finite number', INF, True, 100, 1e-10),
    R(A.frame_fit_parameters, 'radius must be a finite number', np.array(8.0), True, 100, 1e-10),
    R(A.frame_fit_parameters, RADIUS, 0.5, True, 100, 1e-10), R(A.frame_fit_parameters, RADIUS, 20.5, True, 100, 1e-10),
    R(A.frame_fit_parameters, 'tol must be a finite number', 8.0, True, 100, NAN),
    R(A.frame_fit_parameters, 'tol must be a finite number', 8.0, True, 100, INF),
    R(A.frame_fit_parameters, 'tol must lie in (0, 1)', 8.0, True, 100, 0.0),
    R(A.frame_fit_parameters, 'tol must lie in (0, 1)', 8.0, True, 100, 1.0),
    R(A.frame_fit_parameters, 'max_iter must be an integer between 1 and 1000', 8.0, True, 0, 1e-10),
    R(A.frame_fit_parameters, 'max_iter must be an integer between 1 and 1000', 8.0, True, 1001, 1e-10),
    R(A.frame_fit_parameters, 'background must be True or False', 8.0, 1, 100, 1e-10),
    R(A.frame_fit_parameters, RADIUS, 0.5, 1, 0, 0.0),                                                   # order
    R(A.frame_fit_parameters, 'tol must lie in (0, 1)', 8.0, 1, 0, 0.0),                                 # order
    R(A.frame_fit_parameters, 'max_iter must be an integer between 1 and 1000', 8.0, 1, 0, 1e-10),       # order
    R(A.frame_free_parameters, 'max_outer must be an integer between 0 and 16', -1, 1e-3, 0.5, 2.0, 3.0),
    R(A.frame_free_parameters, 'max_outer must be an integer between 0 and 16', 17, 1e-3, 0.5, 2.0, 3.0),
    R(A.frame_free_parameters, 'pos_tol must be a finite number', 8, NAN, 0.5, 2.0, 3.0),
    R(A.frame_free_parameters, 'pos_tol must be > 0', 8, 0.0, 0.5, 2.0, 3.0),
    R(A.frame_free_parameters, 'max_step must be a finite number', 8, 1e-3, INF, 2.0, 3.0),
    R(A.frame_free_parameters, 'max_step must lie in (0, 1] pixels', 8, 1e-3, 0.0, 2.0, 3.0),
    R(A.frame_free_parameters, 'max_step must lie in (0, 1] pixels', 8, 1e-3, 1.5, 2.0, 3.0),
    R(A.frame_free_parameters, 'max_move must be a finite number', 8, 1e-3, 0.5, NAN, 3.0),
    R(A.frame_free_parameters, 'max_move must lie in (0, 4] pixels', 8, 1e-3, 0.5, 0.0, 3.0),
    R(A.frame_free_parameters, 'max_move must lie in (0, 4] pixels', 8, 1e-3, 0.5, 4.5, 3.0),
    R(A.frame_free_parameters, 'min_snr must be a finite number', 8, 1e-3, 0.5, 2.0, INF),
    R(A.frame_free_parameters, 'min_snr must be >= 0', 8, 1e-3, 0.5, 2.0, -0.5),
    R(A.frame_free_parameters, 'pos_tol must be a finite number', 8, INF, 0.5, 2.0, 3.0),
    R(A.frame_free_parameters, 'max_step must be a finite number', 8, 1e-3, NAN, 2.0, 3.0),
    R(A.frame_free_parameters, 'max_move must be a finite number', 8, 1e-3, 0.5, INF, 3.0),
    R(A.frame_free_parameters, 'min_snr must be a finite number', 8, 1e-3, 0.5, 2.0, NAN),
    R(frame_fit, 'image must be a numeric array', image='abc', origin='abc'),                            # order
    R(frame_fit, 'origin must be an integer array of shape (n, 2)', origin=[[0.0, 0.0]], psf='abc'),     # order
    R(frame_fit, 'psf must be a numeric array', psf='abc', psf_index=[0.0]),                             # order
    R(frame_fit, 'psf_index must hold one integer per star', psf_index=[0.0], shift=[[NAN, 0.0]]),       # order
    R(frame_fit, SHIFT8, shift=[[NAN, 0.0]], radius=0.5),                                                # order
    R(frame_fit, RADIUS, radius=0.5, scale0=[NAN]),                                                      # order
    R(frame_fit, 'scale0 must be finite', scale0=[NAN]),
    R(frame_fit, 'without psf_index there must be one model stamp per star (2), got 1', origin=[[0, 0], [1, 1]]),
    R(A.cube_fit_layers, 'a cube has 1 to 4096 layers, not 0', 0),
    R(A.cube_fit_layers, 'a cube has 1 to 4096 layers, not 4097', 4097),
    R(A.cube_fit_layers, 'a cube has 1 to 4096 layers, not True', True),
    R(A.cube_fit_batch, 'layer_batch must be an integer, 0 or above', -1),
    R(A.cube_fit_batch, 'layer_batch must be an integer, 0 or above', 1 << 31),
    R(A.cube_fit_batch, 'layer_batch must be an integer, 0 or above', 1.0),
    R(cube_fit, 'cube must be a numeric array', cube='abc'),
    R(cube_fit, 'cube must have the shape (nl, ny, nx)', cube=FRAME),
    R(cube_fit, 'var must have the shape of cube', var=FRAME),
    R(cube_fit, 'psf must be a numeric array', psf='abc'),
    R(cube_fit, 'psf must have the shape (npsf, 2, 2, 2)', psf=np.ones((1, 3, 2, 2))),
    R(cube_fit, 'psf must have the shape (npsf, 2, 2, 2)', psf=ST2),
    R(cube_fit, 'layer_shift must be a numeric array', layer_shift='abc'),
    R(cube_fit, 'layer_shift must have the shape (2, 2)', layer_shift=np.zeros(4)),
    R(cube_fit, 'layer_shift must be finite', layer_shift=[[NAN, 0.0], [0.0, 0.0]]),
    R(cube_fit, 'shift + layer_shift must stay within 8 pixels', layer_shift=[[8.5, 0.0], [0.0, 0.0]]),
    R(cube_fit, 'shift + layer_shift must stay within 8 pixels', shift=[[5.0, 0.0]], layer_shift=[[4.0, 0.0], [0.0, 0.0]]),
    R(cube_fit, 'scale0 must be a numeric array', scale0='abc'),
    R(cube_fit, 'scale0 must have the shape (2, 1)', scale0=np.zeros(2)),
    R(cube_fit, 'scale0 must be finite', scale0=[[INF], [0.0]]),
    R(cube_fit, 'layer_batch must be an integer, 0 or above', layer_batch=-1),
    R(cube_fit, 'cube must have the shape (nl, ny, nx)', cube=FRAME, layer_batch=-1),                     # order
    R(A.cube_free_work, WORK, 600, 4096, 4096, 1),
    R(cube_free, WORK, cube=HUGE),                        # (counted from the shape: HUGE is never copied)
    R(cube_free, 'max_outer must be an integer between 0 and 16', max_outer=17),
    # ---- what the Context methods raise themselves
    R(C('reconstruct'), 'exactly two layers are supported (psfrec.py:66)', LB3, 1.0, 0.7, 25.0, h=(1.0, 2.0, 3.0)),
    R(C('psf_from_psd'), 'the PSD must be 8 x 8 for this context', np.zeros((4, 4)), LB3),
    R(C('psd_to_psf'), 'the PSD must be 8 x 8 for this context', np.zeros((4, 4)), np.ones((4, 4)), 8.0, [5e-7]),
    R(C('psd_to_psf'), 'the pupil must be a square 2-D array', np.zeros((8, 8)), np.ones((4, 3)), 8.0, [5e-7]),
    R(C('psd_to_psf'), 'phase_static must have the shape of the pupil (4, 4), not (3, 3)', np.zeros((8, 8)), np.ones((4, 4)),
      8.0, [5e-7], phase_static=np.zeros((3, 3))),
    R(C('debug_fetch'), 'x: library returned 0 values, expected 4', 'x', (2, 2)),
    R(C('fit_stamps_device'), 'nstamp must be a positive integer', 0, 1, 2),
    R(C('fit_stamps_device'), 'stamps_ptr and fit_ptr must be device pointers', 1, 0, 2),
    R(C('fit_stamps_elliptical_device'), 'nstamp must be a positive integer', True, 1, 2),
    R(C('fit_stamps_elliptical_device'), 'stamps_ptr and fit_ptr must be device pointers', 1, 1, None),
    R(C('fit_stamps_observed_device'), 'nstamp must be a positive integer', 0, 1, 2),
    R(C('fit_stamps_observed_device'), 'stamps_ptr and fit_ptr must be device pointers', 1, None, 2),
    R(C('fit_stamps_observed_device'), 'circular must be True or False', 1, 1, 2, circular=0),
    R(C('fit_stamps_psf_device'), 'npsf must be a positive integer', 2, 1, 0, 2, 3),
    R(C('fit_stamps_psf_device'), 'stamps_ptr, psf_ptr and fit_ptr must be device pointers', 2, 1, 2, 0, 3),
    R(C('fit_stamps_psf_device'), NSTAMP_EQ, 2, 1, 1, 2, 3),
    R(C('fit_stamps_psf_device'), 'fixed_shift must be True or False', 2, 1, 2, 2, 3, fixed_shift=1),
    R(C('fit_stamps_psf_device'), 'fixed_shift needs shift_ptr', 2, 1, 2, 2, 3, fixed_shift=True),
    R(C('fit_stamps_psf_device'), 'nstamp must be a positive integer', 0, 1, 0, 0, 3),                    # order
    R(C('fit_groups_psf_device'), GROUP1, 2, 1, 1, 2, 2, 3, 4),
    R(C('fit_groups_psf_device'), 'stamps_ptr, psf_ptr, shift_ptr and fit_ptr must be device pointers', 2, 2, 1, 2, 2, 0, 4),
    R(C('fit_groups_psf_device'), NSTAMP_EQ, 2, 2, 1, 3, 2, 3, 4),
    R(C('fit_groups_psf_device'), "mode must be 'free', 'common' or 'fixed'", 2, 2, 1, 2, 2, 3, 4, mode='x'),
    R(C('fit_spectra_psf_device'), 'nstar must be a positive integer', 0, 2, 1, 2, 2, 3),
    R(C('fit_spectra_psf_device'), 'a star cube has 1 to 4096 layers, not 0', 2, 0, 1, 2, 2, 3),
    R(C('fit_spectra_psf_device'), 'cubes_ptr, psf_ptr and fit_ptr must be device pointers', 2, 2, 0, 2, 2, 3),
    R(C('fit_spectra_psf_device'), NSTAR_EQ, 2, 2, 1, 1, 2, 3),
    R(C('fit_spectra_psf_device'), 'at least two values of x must differ', 2, 2, 1, 2, 2, 3, x=[0.0, 0.0]),
    R(C('stamp_metrics_device'), 'stamps_ptr and out_ptr must be device pointers', 1, 1, 0, [1.0], None, None),
    R(C('stamp_metrics_device'), 'need at least one radius, box or fraction', 1, 1, 2, None, None, None),
    R(C('cut_stamps_device'), 'nx must be an integer between 1 and 16384', 8, 0, 1, 2, 3, 4),
    R(C('cut_stamps_device'), 'nstar must be a positive integer', 8, 8, 1, 0, 3, 4),
    R(C('cut_stamps_device'), 'image_ptr, origin_ptr and stamps_ptr must be device pointers', 8, 8, 1, 2, 0, 4),
    R(C('cut_stamps_device'), 'var_ptr and var_stamps_ptr must both be given or both be None', 8, 8, 1, 2, 3, 4, var_ptr=5),
    R(C('render_stars'), 'return_status must be True or False', Z40, [[0, 0]], [1.0], shape=(8, 8), return_status=1),
    R(C('render_stars'), 'scale must be finite', Z40, [[0, 0]], [NAN], shape=(8, 8), return_status=1),      # order
    R(C('render_stars_device'), 'npsf must be a positive integer', 8, 8, 2, 0, 1, 2, 3, 4),
    R(C('render_stars_device'), 'psf_ptr, origin_ptr, scale_ptr and image_out_ptr must be device pointers', 8, 8, 2, 2, 1, 2,
      3, 0),
    R(C('render_stars_device'), NSTAR_EQ, 8, 8, 2, 1, 1, 2, 3, 4),
    R(C('render_stars_device'), 'subtract must be True or False', 8, 8, 2, 2, 1, 2, 3, 4, subtract=1),
    R(C('render_stars_device'), 'subtract needs image_ptr', 8, 8, 2, 2, 1, 2, 3, 4, subtract=True),
    R(C('find_stars'), 'return_map must be True or False', np.zeros((8, 8)), BIG, return_map=1),
    R(C('find_stars_device'), 'ny must be an integer between 1 and 16384', 0, 8, 1, 2, 3, 3, 5.0, 10, 3, 4),
    R(C('find_stars_device'), 'sep must be an integer between 1 and 16', 8, 8, 1, 2, 3, 0, 5.0, 10, 3, 4),
    R(C('find_stars_device'), 'image_ptr, psf_ptr, star_out_ptr and count_ptr must be device pointers', 8, 8, 1, 2, 3, 3,
      5.0, 10, 3, 0),
    R(C('frame_background'), 'return_rms must be True or False', np.zeros((8, 8)), return_rms=1),
    R(C('frame_background_device'), 'nl must be a positive integer', 0, 8, 8, 1, 2, 3),
    R(C('frame_background_device'), 'box must be an integer between 8 and 64', 1, 8, 8, 1, 2, 3, box=7),
    R(C('frame_background_device'), 'image_ptr, mesh_ptr and head_ptr must be device pointers', 1, 8, 8, 1, 2, 0),
    R(C('frame_background_device'), 'apply_to_ptr and applied_ptr must both be None or both be device pointers', 1, 8, 8, 1,
      2, 3, apply_to_ptr=4),
    R(C('frame_background_device'), 'applied_ptr may not be image_ptr', 1, 8, 8, 1, 2, 3, apply_to_ptr=4, applied_ptr=1),
    R(C('group_stars_device'), 'nx must be an integer between 1 and 16384', 8, 0, 2, 1, 2, 1.0, 2, 2, 3, 4),
    R(C('group_stars_device'), CRIT, 8, 8, 2, 1, 2, 0.0, 2, 2, 3, 4),
    R(C('group_stars_device'), 'pos_ptr, label_ptr, group_ptr and count_ptr must be device pointers', 8, 8, 2, 0, 2, 1.0, 2,
      2, 3, 4),
    R(C('group_stars_device'), 'origin_ptr and shift_ptr must both be None or both be device pointers', 8, 8, 2, 1, 2, 1.0, 2,
      2, 3, 4, origin_ptr=5),
    R(C('fit_frame_psf'), 'return_residual must be True or False', FRAME, Z40, [[0, 0]], return_residual=1),
    R(C('fit_frame_psf'), 'return_residual must be True or False', FRAME, Z40, [[0, 0]], return_residual=np.array(True)),
    R(C('fit_frame_psf'), 'tol must lie in (0, 1)', FRAME, Z40, [[0, 0]], tol=0.0, return_residual=1),      # order
    R(C('fit_frame_psf_free'), 'return_residual must be True or False', FRAME, Z40, [[0, 0]], return_residual=None),
    R(C('fit_frame_psf_free'), 'min_snr must be >= 0', FRAME, Z40, [[0, 0]], min_snr=-1.0, return_residual=None),   # order
    R(C('fit_cube_psf'), 'return_residual must be True or False', CUBE, np.zeros((1, 2, 40, 40)), [[0, 0]],
      return_residual='no'),
    R(C('fit_cube_psf_free'), 'return_residual must be True or False', CUBE, np.zeros((1, 2, 40, 40)), [[0, 0]],
      return_residual=0),
    R(frame_dev, 'ny must be an integer between 1 and 16384', ny=0, nstar=0),                            # order
    R(frame_dev, 'nstar must be an integer between 1 and 1048576', nstar=0, npsf=0),                     # order
    R(frame_dev, 'npsf must be a positive integer', npsf=0, head_ptr=0),                                 # order
    R(frame_dev, 'image_ptr, psf_ptr, origin_ptr, star_out_ptr and head_ptr must be device pointers', npsf=1, head_ptr=0),
    R(frame_dev, NSTAR_EQ, npsf=1, radius=0.0),                                                          # order
    R(frame_dev, 'radius must lie between 1 and 20 pixels', radius=0.5),
    R(free_dev, 'image_ptr, psf_ptr, origin_ptr, star_out_ptr, shift_out_ptr and head_ptr must be device pointers',
      shift_out_ptr=None),
    R(free_dev, NSTAR_EQ, npsf=3), R(free_dev, 'nstar must be an integer between 1 and 1048576', nstar=True),
    R(free_dev, 'max_move must lie in (0, 4] pixels', max_move=5.0),
    R(cube_dev, 'a cube has 1 to 4096 layers, not 0', nl=0, nstar=0),                                    # order
    R(cube_dev, 'cube_ptr, psf_ptr, origin_ptr, star_out_ptr and head_ptr must be device pointers', head_ptr=0),
    R(cube_dev, NSTAR_EQ, npsf=1), R(cube_dev, 'layer_batch must be an integer, 0 or above', layer_batch=-1),
    R(cube_free_dev, 'a cube has 1 to 4096 layers, not 4097', nl=4097),
    R(cube_free_dev, 'cube_ptr, psf_ptr, origin_ptr, star_out_ptr, head_ptr, pos_ptr, shift_out_ptr and call_ptr must be '
      'device pointers', call_ptr=0),
    R(cube_free_dev, NSTAR_EQ, npsf=5), R(cube_free_dev, 'pos_tol must be > 0', pos_tol=0.0),
    R(cube_free_dev, WORK, nl=600, ny=4096, nx=4096, nstar=1, npsf=1),
    # ---- the checks of psfrec.py on the primitives: all before a context exists
    R(P.fit_psf_cube, 'circular must be True or False', LB3, np.zeros((3, 40, 40)), circular=1),
    R(P.fit_psf_cube, 'fit_back must be True or False', LB3, np.zeros((3, 40, 40)), fit_back='x'),
    R(P.fit_stars_with_psf, 'fit_back must be True or False', Z40, Z40, fit_back=1),
    R(P.fit_stars_with_psf, 'fixed_shift must be True or False', Z40, Z40, fixed_shift=0),
    R(P.fit_stars_with_psf, 'pixscale must be positive', Z40, Z40, pixscale=0.0),
    R(P.fit_stars_with_psf, 'shift must be a numeric array', Z40, Z40, shift='abc'),
    R(P.fit_stars_with_psf, 'fit_back must be True or False', Z40, Z40, fit_back=1, pixscale=0.0),          # order
    R(P.fit_star_spectra_with_psf, 'fit_back must be True or False', Z40[None], Z40[None], [500.0], fit_back=None),
    R(P.fit_star_spectra_with_psf, 'drift must be True or False', Z40[None], Z40[None], [500.0], drift=1),
    R(P.fit_star_spectra_with_psf, 'lbda must be a numeric array', Z40[None], Z40[None], 'abc'),
    R(P.fit_star_spectra_with_psf, 'shift must be a numeric array', Z40[None], Z40[None], [500.0], shift='abc'),
    R(P.fit_star_groups_with_psf, 'fit_back must be True or False', Z40, Z40, [[[0.0, 0.0]]], fit_back=1),
    R(found_stars, 'fit_back must be True or False', fit_back=1),
    R(found_stars, 'psf must be a numeric array', psf='abc'),
    R(crowded, 'fit_back must be True or False', fit_back=1),
    R(crowded, 'psf must be a numeric array', psf='abc'),
    R(crowded, 'psf must be a numeric array', psf=Holder('abc')),
    R(crowded, 'return_sky must be True or False', return_sky=1),
    R(crowded, 'sky: passes must be an integer between 1 and 8', sky={'passes': True}),
    R(crowded, 'sky: passes must be an integer between 1 and 8', sky={'passes': 0}),
    R(crowded, 'sky: passes must be an integer between 1 and 8', sky={'passes': 9}),
    R(crowded, 'sky: passes must be an integer between 1 and 8', sky={'passes': 2.0}),
    R(crowded_spectra, 'fit_back must be True or False', fit_back=1),
    R(crowded_spectra, 'psf must be a numeric array', psf='abc'),
    R(crowded_spectra, 'lbda must be a numeric array', lbda='abc'),
    R(crowded_spectra, 'layer_shift must be a numeric array', layer_shift='abc'),
    R(P.cut_star_stamps, 'positions must be a numeric array', np.zeros((8, 8)), 'abc'),
    R(P._shift_pixels, 'shift must be a numeric array', [[1.0], 'x'], 0.2),
    R(P.psf_metrics, PRECISION, Z40, precision='fp32'),
    R(field_psf, PRECISION, precision='double'), R(band_psf, PRECISION, precision=None),
    R(profile_psf, PRECISION, precision='MIXED'),
    R(field_psf, NPSFLIN, npsflin=True), R(field_psf, NPSFLIN, npsflin=0), R(field_psf, NPSFLIN, npsflin=6),
    R(band_psf, NPSFLIN, npsflin=2.0), R(band_psf, NPSFLIN, npsflin=6), R(profile_psf, NPSFLIN, npsflin=0),
    R(profile_psf, NPSFLIN, npsflin='1'),
    R(field_psf, SCALARS, seeing='a'), R(field_psf, SCALARS, GL=None), R(band_psf, SCALARS, L0=[1.0, 2.0]),
    R(field_psf, 'need seeing > 0, L0 > 0 and 0 <= GL <= 1', seeing=0.0),
    R(field_psf, 'need seeing > 0, L0 > 0 and 0 <= GL <= 1', L0=NAN),
    R(band_psf, 'need seeing > 0, L0 > 0 and 0 <= GL <= 1', GL=1.5),
    R(field_psf, 'exactly two layers are supported (psfrec.py:66)', h=(1.0, 2.0, 3.0)),
    R(band_psf, 'exactly two layers are supported (psfrec.py:66)', h=(1.0,)),
    R(field_psf, SCALARS, seeing='a', precision='x', npsflin=0),                                         # order
    R(band_psf, PRECISION, precision='x', npsflin=0),                                                    # order
]


@pytest.mark.parametrize('k', range(len(REFUSALS)))
def test_refusal(k):
    fn, args, kwargs, message = REFUSALS[k]
    with pytest.raises(ValueError) as err:
        fn(*args, **kwargs)
    assert str(err.value) == message


def describe(x):
    """`x` as literals: arrays as (dtype, shape, C-contiguous, values with NaN as 'nan'), scalars with their type."""
    if isinstance(x, np.ndarray):
        flat = np.asarray(x).ravel()
        if x.size > 64 and np.array_equal(flat, np.arange(x.size)):
            values = 'arange'
        else:
            values = ['nan' if isinstance(v, float) and v != v else v for v in flat.tolist()]
        return (type(x).__name__, x.dtype.name, x.shape, bool(x.flags.c_contiguous), values)
    if isinstance(x, (tuple, list)):
        return tuple(describe(v) for v in x)
    if x is None:
        return None
    return (type(x).__name__, x.item() if isinstance(x, np.generic) else x)


def K(fn, *args, **kwargs):
    return fn, args, kwargs


ACCEPTED = [
    # the primitives: what they return, and the types they take
    K(A.integer, 'n', 1, 1, 5), K(A.integer, 'n', np.int64(5), 1, 5), K(A.integer, 'n', np.uint8(3), 1, 5),
    K(A.number, 'v', 3), K(A.number, 'v', np.float32(0.5)), K(A.number, 'v', np.int64(-2)), K(A.number, 'v', 1e308),
    K(A.flag, 'f', True), K(A.flag, 'f', np.False_), K(A.flag, 'f', np.True_),
    # the four array behaviours on a masked array, an object with .data, nested lists, Fortran order, float32
    K(A.array, 'a', MASKED), K(A.array, 'a', MASKED, fill=True), K(A.array, 'a', MASKED, unwrap=True),
    K(A.array, 'a', MASKED, fill=True, unwrap=True), K(A.array, 'a', Holder([[1, 2], [3, 4]]), unwrap=True),
    K(A.array, 'a', Holder(MASKED), fill=True, unwrap=True), K(A.array, 'a', [[1, 2], [3, 4]]),
    K(A.array, 'a', ST.astype(np.float32)), K(A.array, 'a', np.asfortranarray(FRAME)), K(A.array, 'a', 3),
    K(A.stamp_stack, 's', ST, 2), K(A.stamp_stack, 's', np.asfortranarray(ST2), 2), K(A.stamp_stack, 's', BIG, 40),
    K(A.stamp_stack, 's', np.arange(16.0).reshape(2, 2, 2, 2), 2),
    K(A._positive_int, 'n', np.int32(7)), K(A._positive_int, 'n', 1 << 40), K(A._group_size, 2), K(A._group_size, np.int64(4)),
    K(A._spec_layers, 1), K(A._spec_layers, 4096), K(A._device_pointers, a_ptr=1, b_ptr=2),
    K(A._model_per_star, 2, 2, None), K(A._model_per_star, 1, 2, 0x10),
    K(A._frame_fit_device, 8, 8, np.int64(2), 2, None, image_ptr=1),
    # the reconstruct calls
    K(A.field_positions, [[60.0, -60.0], [0, 1]]), K(A.field_positions, np.zeros((26, 2)), None),
    K(A.field_positions, np.asfortranarray(np.array([[1.0, 2.0], [3.0, 4.0]], dtype=np.float32))),
    K(A.grid_side, 1), K(A.grid_side, np.int64(5)),
    K(A._grid_or_positions, None, None), K(A._grid_or_positions, 3, None), K(A._grid_or_positions, None, [[1.0, 2.0]]),
    K(A._grid_or_positions, 0, [[1.0, 2.0]]),
    K(A.profile_layers, [0, 50000], 12.5, [0.5, -0.5]), K(A.profile_layers, [[100.0]], [100.0], 1),
    K(A.profile_weights, [1, 3], 2, 2), K(A.profile_weights, [[0.5, 0.5], [0.0, 2.0]], 2, 2),
    K(A.band_weight_matrix, [1, 0, 1], 3), K(A.band_weight_matrix, [[1.0, 2.0, 1.0], [0.0, 1.0, 3.0]], 3),
    # the stamp family
    K(A.elliptical_stamps, ST, 2), K(A.elliptical_stamps, MASKED, 2), K(A.elliptical_stamps, Holder(ST2), 2),
    K(A.elliptical_stamps, BIG),
    K(A.observed_flags, True, True), K(A.observed_flags, False, False), K(A.observed_flags, np.True_, np.False_),
    K(A.observed_stamps, ST, None, 2), K(A.observed_stamps, MASKED, MASKED, 2), K(A.observed_stamps, [[[1, 2], [3, 4]]], ST, 2),
    K(A.observed_stamps, np.asfortranarray(ST2), ST2.astype(np.float32), 2), K(A.observed_stamps, BIG),
    K(A.psf_fit_flags, True, False), K(A.psf_fit_flags, False, True),
    K(A.psf_fit_arguments, 1, ST, None, None, True, False, 2),
    K(A.psf_fit_arguments, 2, MASKED, np.array([0, 0], dtype=np.uint8), [[8.0, -8.0], [0, 1]], False, True, 2),
    K(A.psf_fit_arguments, 2, Holder(ST2), [1, 0], np.array([[0.5, 0.25], [1, 2]], dtype=np.float32), True, False, 2),
    K(A.group_fit_flags, True, 'free'), K(A.group_fit_flags, False, 'common'), K(A.group_fit_flags, True, 'fixed'),
    K(A.group_fit_arguments, 1, ST, None, [[[1, 2], [3, 4]]], True, 'common', 2),
    K(A.group_fit_arguments, 2, ST, np.array([0, 0]), np.arange(-8.0, 8.0).reshape(2, 4, 2), False, 'fixed', 2),
    K(A.spectra_fit_flags, True, None, 1), K(A.spectra_fit_flags, False, [-1, 1], 2),
    K(A.spectra_fit_flags, True, [[0.0, 0.5, 1.0]], 3),
    K(A.spectra_fit_arguments, ST2, None, ST2, None, None, True, None, 2),
    K(A.spectra_fit_arguments, ST2[None], ST2[None], np.arange(16.0).reshape(2, 2, 2, 2), [1], [[0.5, -0.5]], False, [-1, 1], 2),
    K(A.metric_stamps, ST, 2), K(A.metric_stamps, MASKED, 2), K(A.metric_stamps, BIG),
    K(A.metric_stamps, [[[1, 2], [3, NAN]]], 2),
    K(A.metric_parameters, [1, 4], None, 0.5, 2), K(A.metric_parameters, None, (2.0,), [0.25, 0.75], 2),
    K(A.metric_centers, [[100, -100]], 1), K(A.metric_centers, np.asfortranarray(np.arange(4.0).reshape(2, 2)), 2),
    # the frame calls
    K(A.frame_shape, 1, 16384), K(A.frame_shape, np.int64(8192), np.int32(8192)),
    K(A.frame_images, FRAME), K(A.frame_images, np.ma.array(FRAME[:2, :2], mask=[[True, False], [False, False]]), ST),
    K(A.frame_images, np.asfortranarray(FRAME), FRAME.astype(np.float32)), K(A.frame_images, [[1, NAN]], [[0, -1]]),
    K(A.star_origins, [[1 << 30, -(1 << 30)]]), K(A.star_origins, np.array([[1, 2], [3, 4]], dtype=np.uint8), 2),
    K(A.render_flags, True), K(A.render_flags, np.False_),
    K(A.star_scales, 'scale', [1, 2], 2), K(A.star_scales, 'scale0', 3.0, 1), K(A.star_scales, 'scale', np.float32(2), 1),
    K(A.render_arguments, ST, [[0, 0]], [2], None, None, None, (3, np.int64(4)), False, 2),
    K(A.render_arguments, ST, [[0, 0], [1, 1]], [2, 3], [[0, 1], [2, 3]], [0, 0], FRAME, (3, 4), True, 2),
    K(A.find_parameters, 1, 1, 5, 1, 40), K(A.find_parameters, np.int64(8), 16, np.float32(2.5), 1 << 24, 40),
    K(A.find_parameters, 2, 3, -1.5, 10, 4),
    K(A.find_arguments, FRAME, None, CORE, 1, 1, 5.0, 10, 4),
    K(A.find_arguments, FRAME, FRAME, CORE.astype(np.float32).T, 2, 2, 0, 7, 4),
    K(A.background_parameters, 8, 1, 1, 0, 1), K(A.background_parameters, np.int64(64), np.int64(5), 100.0, 16, 1e-3),
    K(A.background_parameters, 32, 3, np.float32(3), 5, 0.25),
    K(A.background_shape, 1, 8192, 8192), K(A.background_shape, np.int64(4), 4096, 4096),
    K(A.background_arguments, FRAME, None, None, 32, 3, 3.0, 5, 0.25),
    K(A.background_arguments, np.ma.array(ST2, mask=ST2 > 6), ST2, [[[1, 2], [3, 4]], [[5, 6], [7, 8]]], 8, 5, 2, 1, 1.0),
    K(A.group_parameters, 1, 2, 16, None), K(A.group_parameters, np.int64(1 << 24), (1 << 31) - 1, np.float32(0.5), 1),
    K(A.group_parameters, 5, 8, 1e-9, (1 << 31) - 1),
    K(A.group_arguments, [[-1, 4], [NAN, 99], [3, -1]], 2, (3, 4)),
    K(A.group_arguments, np.asfortranarray(np.array([[0.0, 0.0, 7.0]])), 1.5, (np.int64(3), 4), 9),
    K(A.group_offsets, [6, 1, 2, 0, 3, 0]), K(A.group_shift_rows, np.arange(24.0), [3, 1, 1, 0, 1, 0]),
    # the crowded-field fits
    K(A.frame_fit_stars, 1), K(A.frame_fit_stars, np.int64(1 << 20)),
    K(A.frame_fit_parameters, 1, True, 1, 0.5), K(A.frame_fit_parameters, 20.0, False, np.int64(1000), np.float32(0.25)),
    K(A.frame_free_parameters, 0, 1e-3, 1, 4, 0), K(A.frame_free_parameters, np.int64(16), np.float32(0.5), 0.5, 2.0, 3),
    K(frame_fit), K(frame_fit, var=FRAME, psf=ST2, psf_index=[1], shift=[[0.5, 8]], scale0=[2], radius=1, background=False,
                    max_iter=np.int64(7), tol=np.float32(0.5)),
    K(A.cube_fit_layers, 1), K(A.cube_fit_layers, np.int64(4096)), K(A.cube_fit_batch, 0), K(A.cube_fit_batch, (1 << 31) - 1),
    K(cube_fit), K(cube_fit, cube=np.ma.array(CUBE, mask=CUBE > 16), var=Holder(CUBE), psf=Holder(CPSF), psf_index=[0],
                   shift=[[1.0, -1.0]], layer_shift=[[7, 0], [0, -7]], scale0=[[1], [2]], layer_batch=np.int64(3)),
    K(cube_fit, cube=Holder(np.ma.array(CUBE, mask=CUBE > 16))),
    K(A.cube_free_work, 2, 3, 3, 1), K(A.cube_free_work, 64, 1024, 1024, 1000),
    K(cube_free), K(cube_free, max_outer=0),
    # the psfrec helpers written once
    K(P._check_circular, np.True_), K(P._check_precision, 'f64'), K(P._grid_or_field, 5, None),
    K(P._grid_or_field, 'ignored', [[1, 2]]), K(P._two_layer_atmosphere, 1, np.float32(0.5), '25', (100, 10000)),
    K(P._shift_pixels, None, 0.2), K(P._shift_pixels, [[1, 2]], 0.5), K(P._sky_parameters, True),
    K(P._sky_parameters, {'passes': np.int64(8), 'box': 16}),
    # a masked psf into find_arguments (neither filled nor unwrapped: the value under the mask, inside the core, stays)
    K(A.find_arguments, FRAME, None, np.ma.array(CORE, mask=CORE > 14), 1, 1, 5.0, 10, 4),
    K(P._sky_parameters, {'passes': 1}),
]

EXPECTED = [           # row for row with ACCEPTED
    ('int', 1),
    ('int', 5),
    ('int', 3),
    ('float', 3.0),
    ('float', 0.5),
    ('float', -2.0),
    ('float', 1e+308),
    ('bool', True),
    ('bool', False),
    ('bool', True),
    ('ndarray', 'float64', (2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (2, 2), True, [1.0, 'nan', 3.0, 4.0]),
    ('ndarray', 'float64', (2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (2, 2), True, [1.0, 'nan', 3.0, 4.0]),
    ('ndarray', 'float64', (2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (3, 4), False, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]),
    ('ndarray', 'float64', (), True, [3.0]),
    ('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (2, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]),
    ('ndarray', 'float64', (1, 40, 40), True, 'arange'),
    ('ndarray', 'float64', (4, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0,
     14.0, 15.0]),
    None,
    None,
    None,
    None,
    None,
    None,
    None,
    None,
    None,
    ('int', 2),
    ('ndarray', 'float64', (2, 2), True, [60.0, -60.0, 0.0, 1.0]),
    ('ndarray', 'float64', (26, 2), True, [0.0] * 52),
    ('ndarray', 'float64', (2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('int', 1),
    ('int', 5),
    (('int', 1), ('int', 0), None),
    (('int', 3), ('int', 0), None),
    (('int', 0), ('int', 1), ('ndarray', 'float64', (1, 2), True, [1.0, 2.0])),
    (('int', 0), ('int', 1), ('ndarray', 'float64', (1, 2), True, [1.0, 2.0])),
    (('ndarray', 'float64', (2,), True, [0.0, 50000.0]), ('ndarray', 'float64', (2,), True, [12.5, 12.5]), ('ndarray',
     'float64', (2,), True, [0.5, -0.5])),
    (('ndarray', 'float64', (1,), True, [100.0]), ('ndarray', 'float64', (1,), True, [100.0]), ('ndarray', 'float64',
     (1,), True, [1.0])),
    ('ndarray', 'float64', (2, 2), True, [1.0, 3.0, 1.0, 3.0]),
    ('ndarray', 'float64', (2, 2), True, [0.5, 0.5, 0.0, 2.0]),
    ('ndarray', 'float64', (1, 3), True, [1.0, 0.0, 1.0]),
    ('ndarray', 'float64', (2, 3), True, [1.0, 2.0, 1.0, 0.0, 1.0, 3.0]),
    ('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (2, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]),
    ('ndarray', 'float64', (1, 40, 40), True, 'arange'),
    ('int', 1),
    ('int', 2),
    ('int', 3),
    (('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]), None),
    (('ndarray', 'float64', (1, 2, 2), True, [1.0, 'nan', 3.0, 4.0]), ('ndarray', 'float64', (1, 2, 2), True, [1.0,
     'nan', 3.0, 4.0])),
    (('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]), ('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0,
     3.0, 4.0])),
    (('ndarray', 'float64', (2, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]), ('ndarray', 'float64', (2, 2,
     2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])),
    (('ndarray', 'float64', (1, 40, 40), True, 'arange'), None),
    ('int', 1),
    ('int', 4),
    (('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]), None, None, ('int', 1)),
    (('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]), ('ndarray', 'int32', (2,), True, [0, 0]),
     ('ndarray', 'float64', (2, 2), True, [8.0, -8.0, 0.0, 1.0]), ('int', 4)),
    (('ndarray', 'float64', (2, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]), ('ndarray', 'int32', (2,),
     True, [1, 0]), ('ndarray', 'float64', (2, 2), True, [0.5, 0.25, 1.0, 2.0]), ('int', 1)),
    ('int', 1),
    ('int', 8),
    ('int', 5),
    (('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]), None, ('ndarray', 'float64', (1, 2, 2), True,
     [1.0, 2.0, 3.0, 4.0]), ('int', 9)),
    (('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]), ('ndarray', 'int32', (2,), True, [0, 0]),
     ('ndarray', 'float64', (2, 4, 2), True, [-8.0, -7.0, -6.0, -5.0, -4.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0,
     5.0, 6.0, 7.0]), ('int', 4)),
    (('int', 1), None),
    (('int', 16), ('ndarray', 'float64', (2,), True, [-1.0, 1.0])),
    (('int', 17), ('ndarray', 'float64', (3,), True, [0.0, 0.5, 1.0])),
    (('ndarray', 'float64', (1, 2, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]), None, ('ndarray',
     'float64', (1, 2, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]), None, None, None, ('int', 1)),
    (('ndarray', 'float64', (1, 2, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]), ('ndarray', 'float64', (1,
     2, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]), ('ndarray', 'float64', (2, 2, 2, 2), True, [0.0, 1.0,
     2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0, 14.0, 15.0]), ('ndarray', 'int32', (1,), True,
     [1]), ('ndarray', 'float64', (1, 2), True, [0.5, -0.5]), ('ndarray', 'float64', (2,), True, [-1.0, 1.0]), ('int',
     16)),
    ('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]),
    ('ndarray', 'float64', (1, 40, 40), True, 'arange'),
    ('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 'nan']),
    (('ndarray', 'float64', (2,), True, [1.0, 4.0]), ('ndarray', 'float64', (0,), True, []), ('ndarray', 'float64',
     (1,), True, [0.5])),
    (('ndarray', 'float64', (0,), True, []), ('ndarray', 'float64', (1,), True, [2.0]), ('ndarray', 'float64', (2,),
     True, [0.25, 0.75])),
    ('ndarray', 'float64', (1, 2), True, [100.0, -100.0]),
    ('ndarray', 'float64', (2, 2), True, [0.0, 1.0, 2.0, 3.0]),
    (('int', 1), ('int', 16384)),
    (('int', 8192), ('int', 8192)),
    (('ndarray', 'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), None),
    (('ndarray', 'float64', (2, 2), True, ['nan', 1.0, 4.0, 5.0]), ('ndarray', 'float64', (2, 2), True, [1.0, 2.0,
     3.0, 4.0])),
    (('ndarray', 'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), ('ndarray',
     'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0])),
    (('ndarray', 'float64', (1, 2), True, [1.0, 'nan']), ('ndarray', 'float64', (1, 2), True, [0.0, -1.0])),
    ('ndarray', 'int32', (1, 2), True, [1073741824, -1073741824]),
    ('ndarray', 'int32', (2, 2), True, [1, 2, 3, 4]),
    ('int', 1),
    ('int', 0),
    ('ndarray', 'float64', (2,), True, [1.0, 2.0]),
    ('ndarray', 'float64', (1,), True, [3.0]),
    ('ndarray', 'float64', (1,), True, [2.0]),
    (None, ('int', 3), ('int', 4), ('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]), None, ('ndarray',
     'int32', (1, 2), True, [0, 0]), None, ('ndarray', 'float64', (1,), True, [2.0]), ('int', 0)),
    (('ndarray', 'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), ('int', 3),
     ('int', 4), ('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]), ('ndarray', 'int32', (2,), True, [0,
     0]), ('ndarray', 'int32', (2, 2), True, [0, 0, 1, 1]), ('ndarray', 'float64', (2, 2), True, [0.0, 1.0, 2.0,
     3.0]), ('ndarray', 'float64', (2,), True, [2.0, 3.0]), ('int', 1)),
    (('int', 1), ('int', 1), ('float', 5.0), ('int', 1)),
    (('int', 8), ('int', 16), ('float', 2.5), ('int', 16777216)),
    (('int', 2), ('int', 3), ('float', -1.5), ('int', 10)),
    (('ndarray', 'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), None,
     ('ndarray', 'float64', (4, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0,
     14.0, 15.0]), ('int', 1), ('int', 1), ('float', 5.0), ('int', 10)),
    (('ndarray', 'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), ('ndarray',
     'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), ('ndarray', 'float64',
     (4, 4), True, [0.0, 4.0, 8.0, 12.0, 1.0, 5.0, 9.0, 13.0, 2.0, 6.0, 10.0, 14.0, 3.0, 7.0, 11.0, 15.0]), ('int',
     2), ('int', 2), ('float', 0.0), ('int', 7)),
    (('int', 8), ('int', 1), ('float', 1.0), ('int', 0), ('float', 1.0)),
    (('int', 64), ('int', 5), ('float', 100.0), ('int', 16), ('float', 0.001)),
    (('int', 32), ('int', 3), ('float', 3.0), ('int', 5), ('float', 0.25)),
    (('int', 1), ('int', 8192), ('int', 8192)),
    (('int', 4), ('int', 4096), ('int', 4096)),
    (('ndarray', 'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), None, None,
     ('int', 32), ('int', 3), ('float', 3.0), ('int', 5), ('float', 0.25)),
    (('ndarray', 'float64', (2, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 'nan']), ('ndarray', 'float64', (2,
     2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]), ('ndarray', 'float64', (2, 2, 2), True, [1.0, 2.0, 3.0,
     4.0, 5.0, 6.0, 7.0, 8.0]), ('int', 8), ('int', 5), ('float', 2.0), ('int', 1), ('float', 1.0)),
    (('int', 1), ('int', 2), ('float', 16.0), ('int', 1)),
    (('int', 16777216), ('int', 2147483647), ('float', 0.5), ('int', 1)),
    (('int', 5), ('int', 8), ('float', 1e-09), ('int', 2147483647)),
    (('ndarray', 'float64', (3, 2), True, [-1.0, 4.0, 'nan', 99.0, 3.0, -1.0]), ('int', 3), ('int', 4), ('float',
     2.0), ('int', 3)),
    (('ndarray', 'float64', (1, 3), True, [0.0, 0.0, 7.0]), ('int', 3), ('int', 4), ('float', 1.5), ('int', 9)),
    ('ndarray', 'int64', (6,), True, [0, 1, 3, 3, 6, 6]),
    ('ndarray', 'float64', (3, 4, 2), True, [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 8.0, 9.0, 10.0, 11.0, 0.0, 0.0,
     0.0, 0.0, 16.0, 17.0, 18.0, 19.0, 20.0, 21.0, 22.0, 23.0]),
    ('int', 1),
    ('int', 1048576),
    (('float', 1.0), ('int', 1), ('int', 1), ('float', 0.5)),
    (('float', 20.0), ('int', 0), ('int', 1000), ('float', 0.25)),
    (('int', 0), ('float', 0.001), ('float', 1.0), ('float', 4.0), ('float', 0.0)),
    (('int', 16), ('float', 0.5), ('float', 0.5), ('float', 2.0), ('float', 3.0)),
    (('ndarray', 'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), None,
     ('ndarray', 'float64', (1, 2, 2), True, [1.0, 2.0, 3.0, 4.0]), None, ('ndarray', 'int32', (1, 2), True, [0, 0]),
     None, None, ('float', 8.0), ('int', 1), ('int', 100), ('float', 1e-10)),
    (('ndarray', 'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), ('ndarray',
     'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), ('ndarray', 'float64',
     (2, 2, 2), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]), ('ndarray', 'int32', (1,), True, [1]), ('ndarray',
     'int32', (1, 2), True, [0, 0]), ('ndarray', 'float64', (1, 2), True, [0.5, 8.0]), ('ndarray', 'float64', (1,),
     True, [2.0]), ('float', 1.0), ('int', 0), ('int', 7), ('float', 0.5)),
    ('int', 1),
    ('int', 4096),
    ('int', 0),
    ('int', 2147483647),
    (('ndarray', 'float64', (2, 3, 3), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0,
     13.0, 14.0, 15.0, 16.0, 17.0]), None, ('ndarray', 'float64', (1, 2, 2, 2), True, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0,
     1.0, 1.0]), None, ('ndarray', 'int32', (1, 2), True, [0, 0]), None, None, None, ('float', 8.0), ('int', 1),
     ('int', 100), ('float', 1e-10), ('int', 0)),
    (('ndarray', 'float64', (2, 3, 3), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0,
     13.0, 14.0, 15.0, 16.0, 'nan']), ('ndarray', 'float64', (2, 3, 3), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0,
     8.0, 9.0, 10.0, 11.0, 12.0, 13.0, 14.0, 15.0, 16.0, 17.0]), ('ndarray', 'float64', (1, 2, 2, 2), True, [1.0, 1.0,
     1.0, 1.0, 1.0, 1.0, 1.0, 1.0]), ('ndarray', 'int32', (1,), True, [0]), ('ndarray', 'int32', (1, 2), True, [0,
     0]), ('ndarray', 'float64', (1, 2), True, [1.0, -1.0]), ('ndarray', 'float64', (2, 2), True, [7.0, 0.0, 0.0,
     -7.0]), ('ndarray', 'float64', (2, 1), True, [1.0, 2.0]), ('float', 8.0), ('int', 1), ('int', 100), ('float',
     1e-10), ('int', 3)),
    (('ndarray', 'float64', (2, 3, 3), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0,
     13.0, 14.0, 15.0, 16.0, 17.0]), None, ('ndarray', 'float64', (1, 2, 2, 2), True, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0,
     1.0, 1.0]), None, ('ndarray', 'int32', (1, 2), True, [0, 0]), None, None, None, ('float', 8.0), ('int', 1),
     ('int', 100), ('float', 1e-10), ('int', 0)),
    ('int', 1472),
    ('int', 1088808804),
    (('ndarray', 'float64', (2, 3, 3), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0,
     13.0, 14.0, 15.0, 16.0, 17.0]), None, ('ndarray', 'float64', (1, 2, 2, 2), True, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0,
     1.0, 1.0]), None, ('ndarray', 'int32', (1, 2), True, [0, 0]), None, None, None, ('float', 8.0), ('int', 1),
     ('int', 100), ('float', 1e-10), (('int', 8), ('float', 0.001), ('float', 0.5), ('float', 2.0), ('float', 3.0))),
    (('ndarray', 'float64', (2, 3, 3), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0,
     13.0, 14.0, 15.0, 16.0, 17.0]), None, ('ndarray', 'float64', (1, 2, 2, 2), True, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0,
     1.0, 1.0]), None, ('ndarray', 'int32', (1, 2), True, [0, 0]), None, None, None, ('float', 8.0), ('int', 1),
     ('int', 100), ('float', 1e-10), (('int', 0), ('float', 0.001), ('float', 0.5), ('float', 2.0), ('float', 3.0))),
    ('bool', True),
    None,
    None,
    ('ndarray', 'float64', (1, 2), True, [1.0, 2.0]),
    (('float', 1.0), ('float', 0.5), ('float', 25.0)),
    None,
    ('ndarray', 'float64', (1, 2), True, [2.0, 4.0]),
    (('int', 2), ('dict', {'box': 32, 'filter': 3, 'kappa': 3.0, 'max_clip': 5, 'min_frac': 0.25})),
    (('int', 8), ('dict', {'box': 16, 'filter': 3, 'kappa': 3.0, 'max_clip': 5, 'min_frac': 0.25})),
    (('ndarray', 'float64', (3, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0]), None,
     ('ndarray', 'float64', (4, 4), True, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0,
     14.0, 15.0]), ('int', 1), ('int', 1), ('float', 5.0), ('int', 10)),
    (('int', 1), ('dict', {'box': 32, 'filter': 3, 'kappa': 3.0, 'max_clip': 5, 'min_frac': 0.25})),
]


@pytest.mark.parametrize('k', range(len(ACCEPTED)))
def test_accepted(k):
    fn, args, kwargs = ACCEPTED[k]
    assert len(EXPECTED) == len(ACCEPTED)
    assert describe(fn(*args, **kwargs)) == EXPECTED[k]


def test_no_copy():
    """Where the caller's own float64, C-contiguous array was handed on without a copy, it still is."""
    var = FRAME + 1.0
    im, va = A.frame_images(FRAME, var)
    assert im is FRAME and va is var
    assert A.find_arguments(FRAME, None, CORE, 1, 1, 5.0, 10, 4)[2] is CORE
    pos = np.array([[1.0, 1.0, 5.0]])
    assert A.group_arguments(pos, 1.0, (4, 4))[0] is pos
    res = cube_fit(var=CUBE)                    # (an ndarray's own .data is unwrapped: a view of the same memory)
    assert np.shares_memory(res[0], CUBE) and np.shares_memory(res[1], CUBE) and np.shares_memory(res[2], CPSF)
    a, b, c = A.background_arguments(CUBE, CUBE, CUBE, 32, 3, 3.0, 5, 0.25)[:3]
    assert a is CUBE and b is CUBE and c is CUBE
    assert A.array('a', ST) is ST and A.array('a', Holder(ST), unwrap=True) is ST
    for view, base in ((A.stamp_stack('s', ST2, 2), ST2), (A.elliptical_stamps(ST, 2), ST),
                       (A.observed_stamps(ST2, ST2, 2)[1], ST2), (A.metric_stamps(ST2, 2), ST2),
                       (A.psf_fit_arguments(1, ST, None, np.zeros((1, 2)), True, False, 2)[0], ST),
                       (A.star_scales('scale', ST[0], 2), ST), (A.metric_centers(ST, 2), ST)):
        assert np.shares_memory(view, base)
