"""The checked calls and the predecessors of tests/test_gpu_stamp_call_history.py (DESIGN.md "Call-order independence",
the second table), shared with P9 of tests/test_gpu_call_history.py.

A checked call is one call of a stamp, frame or cube entry point on the seeded scene its parity test uses:
CHECKED[name] = (run, hold).  run(api, ctx) returns the call's output arrays by name, every one in full (the rows behind
a count included: the host form copies them back from the staging buffer as they are).  hold(api, out, prec) asserts
them against the entry point's fp64 reference with the helper and the bounds of its own parity test, imported from
that test, so that the bit comparison of the history test cannot be between two wrong results.

PREDECESSORS[name] are the calls run between two runs of the checked call: {label: fn(api, ctx)}.  The labels start
with the kind of the leftovers:
  L  the same entry point, larger (frame 131 x 170, more stars or stamps, 5 layers): every array of the checked call
     lies over the lists and frames of L
  S  the same entry point, smaller (frame 40 x 45: 2 x 2 ragged tiles, a few stars or stamps, 1 or 2 layers)
  X  the other tenant of the workspace (fit_frame_psf <-> fit_frame_psf_free on framefit, fit_cube_psf <->
     fit_cube_psf_free on cubefit, the host form of fit_cube_psf with layer_batch = 2 over 5 layers, render_stars with
     the pile of 300 before a fit of the same frame shape; for the stamp calls the host form of fit_cube_psf, which holds
     one batch of layers at a time in the staging buffer; frame_background, which has no workspace and leaves three input and five output
     planes in the staging buffer, before the frame calls and cut_stamps, and find, a frame fit and the cube's host form
     before it)
  T  another terminal state at the same shape: only the steering words differ
  N  the same entry point on data of NaN, +-inf and +-1e300: the workspaces are left holding non-finite doubles
  F  a refused call of the same entry point (MPSFR_E_INVALID) between two good ones
Every predecessor is a legal call: nothing is poisoned.
"""
import numpy as np

import background_ref as BG
import cube_fit_cases as K
import cube_free_cases as Q
import cube_free_ref as CR
import find_ref as FI
import frame_fit_ref as F
import frame_free_ref as G
import group_ref as GR
import moffat_ell_ref as M
import psf_fit_ref as PF
import psf_group_ref as PG
import psf_spec_ref as SR
import render_ref as Y

DIM = 128                                      # of the contexts: the stamp, frame and cube calls do not depend on it
NS = 40
LARGE, SMALL = (131, 170), (40, 45)
E_INVALID = -1
ONE_STEP = dict(max_step=0.15)                 # of the free frame fit: the rule clips 20 of 32 steps, one star is held
CUBE_STEP = dict(max_step=0.15, min_snr=20.0)  # of the free cube fit: 24 steps clipped, two stars held by min_snr
FIND_MAX = 256


def context(api, prec):
    return api.Context(dim=DIM, pixscale=api.grid_pixscale(DIM), precision=prec)


def bits(a):
    """The bytes of `a` one per element of a last axis: what np.array_equal compares (NaN equals NaN, -0 is not +0)."""
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))


def difference(got, want):
    """None if the arrays have the same type, shape and bytes, else (differing elements, first differing index)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return 'dtype or shape', (str(got.dtype), got.shape, str(want.dtype), want.shape)
    bad = np.flatnonzero(np.any(bits(got) != bits(want), axis=-1).reshape(-1))
    if bad.size == 0:
        return None
    return int(bad.size), tuple(int(i) for i in np.unravel_index(bad[0], got.shape)) if got.ndim else ()


def differences(checked, pred, got, want):
    """The failure messages of a (checked call, predecessor) pair: one per output array that differs."""
    assert sorted(got) == sorted(want)
    out = []
    for k in sorted(want):
        d = difference(got[k], want[k])
        if d is not None:
            out.append('%s after %s: output %s differs in %s elements, the first at index %s' % ((checked, pred, k) + d))
    return out


# ---- scenes of the predecessors -------------------------------------------------------------------------------------

_FIELD = {}


def field(shape, n, seed, nl=0, wild=False):
    """n stars at random on a frame of `shape` and one wholly off it, the four models of render_ref by k % 4, sky, var =
    4 + model / 2 and Gaussian noise of that variance, 1 % NaN pixels; default_rng(seed).  nl > 0: a cube of nl layers
    (the models rotated by layer, cube_fit_cases.layer_shifts, the fluxes 1 + l times as bright).  wild: 8 % of the data
    are +-inf and +-1e300.  A dict as frame_fit_ref.scene() (nl = 0) or
    cube_fit_cases.cube() gives."""
    key = (tuple(shape), n, seed, nl, wild)
    if key in _FIELD:
        return _FIELD[key]
    rng = np.random.default_rng(seed)
    ny, nx = shape
    pos = np.concatenate([np.stack([rng.uniform(2, ny - 2, n), rng.uniform(2, nx - 2, n)], axis=1), [[-70.0, 10.3]]])
    n += 1
    origin = (np.rint(pos) - NS // 2).astype(np.int32)
    shift = pos - (origin + NS // 2)
    index = (np.arange(n) % 4).astype(np.int32)
    layers = max(nl, 1)
    psf = np.stack([np.roll(Y.models(), l, axis=0) for l in range(layers)], axis=1)
    ls = K.layer_shifts(layers)
    data, var = np.empty((layers,) + tuple(shape)), np.empty((layers,) + tuple(shape))
    for l in range(layers):
        flux = rng.uniform(200, 5000, n) * (1.0 + l)
        model, _, _ = Y.render(None, np.ascontiguousarray(psf[:, l]), index, origin, shift + ls[l], flux, shape=shape)
        var[l] = 4.0 + model / 2.0
        data[l] = model + F.SKY + rng.normal(size=shape) * np.sqrt(var[l])
        data[l][rng.uniform(size=shape) < 0.01] = np.nan
    if wild:
        u = rng.uniform(size=data.shape)
        for lo, v in ((0.0, np.inf), (0.02, -np.inf), (0.04, 1e300), (0.06, -1e300)):
            data[(u >= lo) & (u < lo + 0.02)] = v
    s = dict(psf=psf, index=index, origin=origin, shift=shift, n=n)
    if nl:
        s.update(cube=data, var=var, layer_shift=ls)
    else:
        s.update(image=data[0], var=var[0], psf=np.ascontiguousarray(psf[:, 0]))
    _FIELD[key] = s
    return s


def lost_stars(s):
    """The scene or cube `s` with every star off the frame: empty lists, nothing fitted."""
    return dict(s, origin=s['origin'] - np.int32(1000))


def wild_copy(a, seed=41):
    """`a` with 8 % of its values replaced by +-inf and +-1e300."""
    a = np.array(a, dtype=np.float64)
    u = np.random.default_rng(seed).uniform(size=a.shape)
    for lo, v in ((0.0, np.inf), (0.02, -np.inf), (0.04, 1e300), (0.06, -1e300)):
        a[(u >= lo) & (u < lo + 0.02)] = v
    return a


# ---- the calls on a scene dict --------------------------------------------------------------------------------------

def render(ctx, s, image='scene', subtract=False):
    im = s['image'] if isinstance(image, str) else image
    frame, rows = ctx.render_stars(s['psf'], s['origin'], s['scale'], shift=s['shift'], psf_index=s['index'], image=im,
                                   shape=None if im is not None else s['shape'], subtract=subtract, return_status=True)
    return dict(frame=frame, rows=rows)


def render_scene(s, seed=3):
    """A fit scene as a render scene: its stars with scales in +-1000."""
    return dict(s, scale=np.random.default_rng(seed).uniform(-1000, 1000, s['n']), shape=s['image'].shape)


def frame_fit(ctx, s, with_var=True, **kw):
    rows, head, resid = ctx.fit_frame_psf(s['image'], s['psf'], s['origin'], var=s['var'] if with_var else None,
                                          shift=s['shift'], psf_index=s['index'], return_residual=True, **kw)
    return dict(rows=rows, head=head, resid=resid)


def frame_free(ctx, s, with_var=True, **kw):
    rows, shifts, head, resid = ctx.fit_frame_psf_free(s['image'], s['psf'], s['origin'],
                                                       var=s['var'] if with_var else None, shift=s['shift'],
                                                       psf_index=s['index'], return_residual=True, **kw)
    return dict(rows=rows, shifts=shifts, head=head, resid=resid)


def cube_fit(ctx, c, with_var=True, **kw):
    rows, head, resid = ctx.fit_cube_psf(c['cube'], c['psf'], c['origin'], var=c['var'] if with_var else None,
                                         shift=c['shift'], layer_shift=c['layer_shift'], psf_index=c['index'],
                                         return_residual=True, **kw)
    return dict(rows=rows, head=head, resid=resid)


def cube_free(ctx, c, with_var=True, **kw):
    rows, pos, shifts, head, call, resid = ctx.fit_cube_psf_free(
        c['cube'], c['psf'], c['origin'], var=c['var'] if with_var else None, shift=c['shift'],
        layer_shift=c['layer_shift'], psf_index=c['index'], return_residual=True, **kw)
    return dict(rows=rows, pos=pos, shifts=shifts, head=head, call=call, resid=resid)


def _find(ctx, image, psf, var, half=3, sep=3, threshold=5.0, max_stars=FIND_MAX, **kw):
    import test_gpu_find as T
    return T.raw_find(ctx, image, psf, var, half, sep, threshold, max_stars, **kw)


def _group(ctx, pos, crit, shape, **kw):
    import test_gpu_group as T
    return T.raw_group(ctx, pos, crit, shape, **kw)


def _arrays(d, keys):
    return {k: np.asarray(d[k]) for k in keys}


FIND_OUT = ('rows', 'origin', 'count', 'map')
GROUP_OUT = ('label', 'groups', 'origin', 'shift', 'counts')


# ---- the checked calls: run and hold --------------------------------------------------------------------------------

def run_render(api, ctx):
    return render(ctx, Y.scene(), subtract=True)


def hold_render(api, out, prec):
    import test_gpu_render as T
    s = Y.scene()
    want, npix, S = Y.scene_reference(True)
    assert T._worst_ratio(out['frame'], want, S) <= T.PARITY
    rows = out['rows']
    assert np.array_equal(rows[:, 1], npix) and np.all(rows[:, 2:] == 0)
    assert np.array_equal(rows[:, 0], np.where(npix == 0, 1, 0)) and len(s['off_frame']) == int(rows[:, 0].sum())


def _cut_inputs():
    """The frame, the variances and the origins of tests/test_gpu_render.py::test_cut_is_numpy_slicing_bit_for_bit."""
    rng = np.random.default_rng(4)
    ny, nx = 97, 150
    image = rng.normal(size=(ny, nx))
    image[rng.uniform(size=image.shape) < 0.01] = np.nan
    image[3, 4], image[5, 6] = np.inf, -0.0
    var = rng.uniform(-0.1, 2.0, (ny, nx))
    origin = np.array([[0, 0], [-39, -39], [ny - 1, nx - 1], [-40, 10], [10, nx], [30, 60], [57, 110], [-17, 133],
                       [5000, 5000], [-(2 ** 30), 2 ** 30], [2 ** 30, -(2 ** 30)], [2 ** 30, 20], [20, -(2 ** 30)]],
                      dtype=np.int32)
    return image, var, origin


def cut(ctx, image, var, origin):
    if var is None:
        return dict(stamps=ctx.cut_stamps(image, origin))
    st, va = ctx.cut_stamps(image, origin, var=var)
    return dict(stamps=st, var=va)


def run_cut(api, ctx):
    return cut(ctx, *_cut_inputs())


def hold_cut(api, out, prec):
    image, var, origin = _cut_inputs()
    want, vwant = Y.cut(image, var, origin)
    assert difference(out['stamps'], want) is None and difference(out['var'], vwant) is None


def run_find(api, ctx):
    s = FI.scene()
    return _arrays(_find(ctx, s['image'], s['psf'], s['var'], threshold=FI.THRESHOLD[True]), FIND_OUT)


def hold_find(api, out, prec):
    import test_gpu_find as T
    ref = FI.scene_reference(True, 3, 3, FI.THRESHOLD[True])
    assert 10 <= ref['count'] < FIND_MAX
    T.assert_parity(dict(out, count=int(out['count'])), ref, 'call history')


def run_group(api, ctx):
    pos, crit, shape = GR.scenes()['field']
    return _arrays(_group(ctx, pos, crit, shape), GROUP_OUT)


def hold_group(api, out, prec):
    import test_gpu_group as T
    pos, crit, shape, ref = GR.scene_reference('field')
    T.assert_reference(out, ref, len(pos))


def _fit_test():
    import test_gpu_frame_fit as T
    return T


def run_frame_fit(api, ctx):
    T = _fit_test()
    return frame_fit(ctx, F.scene(), max_iter=T.MAX_ITER, tol=T.TOL)


def hold_frame_fit(api, out, prec):
    T = _fit_test()
    ref = F.scene_reference(True, True, 8.0)
    T._check_against(out['rows'], out['head'], ref, F.bounds(ref, T.TOL, T.MAX_ITER))
    assert np.array_equal(np.isnan(out['resid']), np.isnan(F.scene()['image']))


def run_frame_free(api, ctx):
    import test_gpu_frame_free as T
    return frame_free(ctx, G.displaced_scene(True), max_iter=T.MAX_ITER, tol=T.TOL, max_outer=1, **ONE_STEP)


def hold_frame_free(api, out, prec):
    import test_gpu_frame_free as T
    ref = T.check_one_step(G.displaced_scene(True), out['rows'], out['shifts'], out['head'], **ONE_STEP)
    flags = ref['flags'][ref['problem'].acc]
    assert (flags & G.HELD).any() and (flags & G.CLIPPED).any()


_LAYER_REF = {}


def _cube_layer_reference(l):
    c = Q.cube(True)
    key = l
    if key not in _LAYER_REF:
        _LAYER_REF[key] = F.solve(c['cube'][l], c['var'][l], np.ascontiguousarray(c['psf'][:, l]), c['index'], c['origin'],
                              c['shift'] + c['layer_shift'][l], 8.0, True)
    return _LAYER_REF[key]


def run_cube_fit(api, ctx):
    T = _fit_test()
    return cube_fit(ctx, Q.cube(True), max_iter=T.MAX_ITER, tol=T.TOL)


def hold_cube_fit(api, out, prec):
    T = _fit_test()
    c = Q.cube(True)
    assert out['rows'].shape == (Q.NL, c['n'], 8) and Q.NL == 3
    for l in range(Q.NL):
        ref = _cube_layer_reference(l)
        T._check_against(out['rows'][l], out['head'][l], ref, F.bounds(ref, T.TOL, T.MAX_ITER))
    assert out['rows'][Q.MASK_LAYER, Q.MASKED, 7] == 2


def run_cube_free(api, ctx):
    import test_gpu_cube_free as T
    return cube_free(ctx, Q.cube(True), max_iter=T.MAX_ITER, tol=T.TOL, max_outer=1, **CUBE_STEP)


def hold_cube_free(api, out, prec):
    import test_gpu_cube_free as T
    ref = T.check_one_step(Q.cube(True), out['rows'], out['pos'], out['shifts'], out['head'], out['call'],
                           **CUBE_STEP)
    assert (ref['flags'] & G.HELD).any() and (ref['flags'] & G.CLIPPED).any() and np.all(out['head'][:, 7] != 2)


def _ell_pars():
    import test_gpu_fit_ell as T
    return T._synthetic_grid()[::15]


def run_fit_ell(api, ctx):
    return dict(fit=ctx.fit_stamps_elliptical(np.array([M.stamp(*p) for p in _ell_pars()])))


def hold_fit_ell(api, out, prec):
    import test_gpu_fit_ell as T
    fit = out['fit']
    assert np.all(fit[:, 18].astype(int) & 3 == 0) and np.all(fit[:, 21:] == 0.0)
    for p, row in zip(_ell_pars(), fit):
        worst = T._compare(M.gpu_derived(row), T._want(p), T.TOL[prec])
        assert max(worst.values()) <= 1.0, worst


def run_fit_obs(api, ctx):
    import test_gpu_fit_obs as T
    data, var, _ = T._yardstick(True, True)
    return dict(fit=ctx.fit_stamps_observed(data, var, background=True, circular=False))


def hold_fit_obs(api, out, prec):
    import test_gpu_fit_obs as T
    _, _, ref = T._yardstick(True, True)
    fit = out['fit']
    assert np.all(T._status(fit) & 7 == 0) and np.all(np.isfinite(fit))
    worst, worst_err = T.parity_worst(fit, ref, True, True)
    assert max(worst.values()) <= T.SIGMA_TOL[prec], worst
    assert max(worst_err.values()) <= T.ERR_TOL, worst_err


def run_fit_psf(api, ctx):
    data, var, psf, _, shift, _ = PF.yardstick(True, False)
    return dict(fit=ctx.fit_stamps_psf(data, psf, var=var, shift=shift, background=True, fixed_shift=False))


def hold_fit_psf(api, out, prec):
    import test_gpu_psf_fit as T
    ref = PF.yardstick(True, False)[5]
    fit = out['fit']
    assert np.all(T._status(fit) == 0) and np.all(np.isfinite(fit))
    for row, want in zip(fit, ref):
        assert int(row[11]) == want['npix']
        s, e = T._sigma(row, want)
        assert s <= T.SIGMA_TOL[prec] and e <= T.ERR_TOL
        assert abs(row[4] - want['chi2']) <= T.ERR_TOL * want['chi2']


GROUP_CASE = (3, True, 'free')


def run_fit_groups(api, ctx):
    data, var, psf, _, _, _, given, _ = PG.yardstick(*GROUP_CASE)
    return dict(fit=ctx.fit_groups_psf(data, psf, given, var=var, background=True, mode='free'))


def hold_fit_groups(api, out, prec):
    import test_gpu_psf_group as T
    ref = PG.yardstick(*GROUP_CASE)[7]
    fit = out['fit']
    assert np.all(T._status(fit) == 0) and np.all(np.isfinite(fit))
    assert [int(r[5]) for r in fit] == [w['npix'] for w in ref]
    for row, want in zip(fit, ref):
        s, e, c = T._sigma(row, want, *GROUP_CASE)
        assert s <= T.SIGMA_TOL[prec] and e <= T.ERR_TOL and c <= T.ERR_TOL
        assert abs(row[2] - want['chi2']) <= T.ERR_TOL * want['chi2']


SPEC_STARS = (0, 1)                            # of psf_spec_ref.stars: 5 layers, the default start, one layer all NaN


def spectra(ctx, ss, drift=True, x=None, back=True):
    cubes, var, psf, sh = SR.batch(ss)
    head, lay = ctx.fit_spectra_psf(cubes, psf, var=var, shift=sh, background=back,
                                    x=(ss[0]['x'] if x is None else x) if drift else None)
    return dict(head=head, layers=lay)


def run_fit_spectra(api, ctx):
    ss = SR.stars(True, True)
    return spectra(ctx, [ss[k] for k in SPEC_STARS])


def hold_fit_spectra(api, out, prec):
    import test_gpu_psf_spec as T
    ss, refs = SR.yardstick(True, True)
    assert SR.NAN_LAYER[0] in SPEC_STARS
    for i, k in enumerate(SPEC_STARS):
        head, lay = out['head'][i], out['layers'][i]
        assert int(head[10]) == 0 and np.all(np.isfinite(head)) and np.all(np.isfinite(lay))
        sig, err, chi = T._compare(head, lay, refs[k], SR.problem(ss[k], True, True))
        assert sig <= T.SIGMA_TOL[prec] and err <= T.ERR_TOL and chi <= T.ERR_TOL


def _metric_stamps():
    import test_gpu_metrics as T
    return np.array([M.stamp(*p) for p in T._synthetic_grid()[::25]])


def run_metrics(api, ctx):
    import test_gpu_metrics as T
    return dict(rows=ctx.stamp_metrics(_metric_stamps(), T.RADII, T.BOXES, ()))


def hold_metrics(api, out, prec):
    import test_gpu_metrics as T
    worst = T._compare_rows(out['rows'], _metric_stamps(), T.RADII, T.BOXES)
    assert max(worst.values()) <= 1.0, worst


BACK_OUT = ('mesh', 'head', 'map', 'rms', 'applied')


def background(ctx, image, var=None, apply=None, **kw):
    """mpsfr_frame_background through the raw call of its parity test (canaries behind every output)."""
    import test_gpu_background as T
    return T.raw_back(ctx, image, var, apply, **kw)


def run_background(api, ctx):
    s = BG.scene()
    return _arrays(background(ctx, s['image'], s['var'], s['apply']), BACK_OUT)


def hold_background(api, out, prec):
    import test_gpu_background as T
    ref = BG.scene_reference(True, BG.DEFAULTS['box'], BG.DEFAULTS['filter'], BG.DEFAULTS['max_clip'])
    assert (ref['mesh'][0][..., 7].astype(int) & BG.FILLED).any() and np.any(ref['mesh'][0][..., 6] >= 2)
    T.assert_parity(out, ref, 'call history', BG.scene()['apply'])


CHECKED = {
    'render_stars': (run_render, hold_render),
    'cut_stamps': (run_cut, hold_cut),
    'find_stars': (run_find, hold_find),
    'group_stars': (run_group, hold_group),
    'fit_frame_psf': (run_frame_fit, hold_frame_fit),
    'fit_frame_psf_free': (run_frame_free, hold_frame_free),
    'fit_cube_psf': (run_cube_fit, hold_cube_fit),
    'fit_cube_psf_free': (run_cube_free, hold_cube_free),
    'fit_stamps_elliptical': (run_fit_ell, hold_fit_ell),
    'fit_stamps_observed': (run_fit_obs, hold_fit_obs),
    'fit_stamps_psf': (run_fit_psf, hold_fit_psf),
    'fit_groups_psf': (run_fit_groups, hold_fit_groups),
    'fit_spectra_psf': (run_fit_spectra, hold_fit_spectra),
    'stamp_metrics': (run_metrics, hold_metrics),
    'frame_background': (run_background, hold_background),
}
FRAME_CALLS = ('render_stars', 'find_stars', 'group_stars', 'fit_frame_psf', 'fit_frame_psf_free', 'fit_cube_psf',
               'fit_cube_psf_free', 'frame_background')
AFTER_BACKGROUND = tuple(c for c in FRAME_CALLS if c != 'frame_background') + ('cut_stamps',)      # have X_background


# ---- variants: other terminal states as the checked call itself -----------------------------------------------------
# A predecessor list runs one way only.  These run the other way: the state that is a T predecessor above is the
# checked call here, after the converging or multi-step call.  '<entry point>.<state>'.

FIND_NO_MAP_OUT = ('rows', 'origin', 'count')


def run_find_no_map(api, ctx):
    """find_stars without the map: FindWork holds the map itself, and mask, count, offset and list lie behind it."""
    s = FI.scene()
    return _arrays(_find(ctx, s['image'], s['psf'], s['var'], threshold=FI.THRESHOLD[True], want_map=False),
                   FIND_NO_MAP_OUT)


def hold_find_no_map(api, out, prec):
    import test_gpu_find as T
    ref = FI.scene_reference(True, 3, 3, FI.THRESHOLD[True])
    T.assert_parity(dict(out, count=int(out['count'])), ref, 'call history, no map', with_map=False)


def _hold_capped(rows, head, ref, moved=False):
    """A solve stopped by max_iter = 1.  The yardstick has no bound for an iterate that has not converged, so the
    values are held to what tests/test_gpu_frame_fit.py::test_iteration_cap_gives_status_one_and_finite_rows asserts of
    this state -- status 1, finite rows -- and everything the iteration does not touch to the fp64 reference: who is
    fitted, the pixel counts, and N_kk within its bound (not of a free fit, moved=True, whose N_kk is that of the shifts
    after the step while the reference is the solve at the start)."""
    assert head[7] == 1 and np.all(np.isfinite(rows)) and np.all(np.isfinite(head))
    np.testing.assert_array_equal(rows[:, 7], ref['status'])
    np.testing.assert_array_equal(rows[:, 5], ref['ndisc'])
    assert (head[3], head[6]) == (ref['nomega'], ref['nacc'])
    acc = ref['acc']
    if not moved:
        assert np.max(np.abs(rows[acc, 6] - ref['nkk'][acc]) / ref['nkk'][acc]) <= F.bounds(ref, 1e-10, 100)['nkk_rel']
    assert np.all(rows[acc, 1] > 0) and not rows[np.setdiff1d(np.arange(len(rows)), acc), :7].any()


def run_frame_fit_capped(api, ctx):
    return frame_fit(ctx, F.scene(), max_iter=1, tol=_fit_test().TOL)


def hold_frame_fit_capped(api, out, prec):
    assert out['head'][4] == 1
    _hold_capped(out['rows'], out['head'], F.scene_reference(True, True, 8.0))


def run_cube_fit_capped(api, ctx):
    return cube_fit(ctx, Q.cube(True), max_iter=1, tol=_fit_test().TOL)


def hold_cube_fit_capped(api, out, prec):
    for l in range(Q.NL):
        assert out['head'][l, 4] == 1
        _hold_capped(out['rows'][l], out['head'][l], _cube_layer_reference(l))


_START_REF = {}


def _frame_start_reference():
    s = G.displaced_scene(True)
    if not _START_REF:
        _START_REF['ref'] = F.solve(s['image'], s['var'], s['psf'], s['index'], s['origin'], s['shift'], 8.0, True)
    return _START_REF['ref']


def run_frame_free_no_outer(api, ctx):
    return frame_free(ctx, G.displaced_scene(True), max_outer=0, max_iter=100, tol=1e-10)


def hold_frame_free_no_outer(api, out, prec):
    import test_gpu_frame_free as T
    T.check_no_outer_step(G.displaced_scene(True), out['rows'], out['shifts'], out['head'], True)


def run_frame_free_capped(api, ctx):
    import test_gpu_frame_free as T
    return frame_free(ctx, G.displaced_scene(True), max_iter=1, tol=T.TOL, max_outer=1, **ONE_STEP)


def hold_frame_free_capped(api, out, prec):
    assert np.all(np.isfinite(out['shifts']))
    _hold_capped(out['rows'][:, :8], out['head'], _frame_start_reference(), moved=True)


_CUBE_PROBLEM = {}


def _cube_problem():
    if not _CUBE_PROBLEM:
        c = Q.cube(True)
        _CUBE_PROBLEM['p'] = CR.CubeProblem(c['cube'], c['var'], c['psf'], c['index'], c['origin'], c['shift'],
                                            c['layer_shift'], 8.0, True)
    return _CUBE_PROBLEM['p']


def run_cube_free_no_outer(api, ctx):
    import test_gpu_cube_free as T
    return cube_free(ctx, Q.cube(True), max_outer=0, max_iter=T.MAX_ITER, tol=T.TOL)


def hold_cube_free_no_outer(api, out, prec):
    """max_outer = 0: the closing solve at the start shifts, every layer against the dense solve there with the checks
    and the bounds of tests/test_gpu_cube_free.py's parity test; nothing moved, nobody free."""
    import test_gpu_cube_free as T
    c, cp = Q.cube(True), _cube_problem()
    rows, head, pos, call = out['rows'], out['head'], out['pos'], out['call']
    for l in range(Q.NL):
        pr = cp.layers[l]
        np.testing.assert_array_equal(rows[l, :, 7], pr.base['status'])
        np.testing.assert_array_equal(rows[l, :, 5], pr.base['ndisc'])
        assert (head[l, 3], head[l, 6], head[l, 7]) == (pr.nomega, pr.nacc, 0)
        ref = pr.held(c['shift'] + c['layer_shift'][l])
        ratios = T._check_layer(rows[l], head[l], ref, F.bounds(ref, T.TOL, T.MAX_ITER), pr.acc)
        assert max(ratios.values()) < 1.0, (l, ratios)
    assert difference(out['shifts'], c['shift']) is None and difference(pos[:, :2], c['shift']) is None
    assert not pos[:, 2:].any() and list(call[2:5]) == [0, 0, 0] and call[6] == 0 and call[7] <= T.TOL


def run_cube_free_capped(api, ctx):
    import test_gpu_cube_free as T
    return cube_free(ctx, Q.cube(True), max_iter=1, tol=T.TOL, max_outer=1, **CUBE_STEP)


def hold_cube_free_capped(api, out, prec):
    cp = _cube_problem()
    assert out['call'][6] == 1 and all(np.all(np.isfinite(out[k])) for k in ('pos', 'shifts', 'call'))
    for l in range(Q.NL):
        _hold_capped(out['rows'][l], out['head'][l], cp.layers[l].base, moved=True)


CHECKED.update({
    'find_stars.no_map': (run_find_no_map, hold_find_no_map),
    'fit_frame_psf.max_iter_1': (run_frame_fit_capped, hold_frame_fit_capped),
    'fit_cube_psf.max_iter_1': (run_cube_fit_capped, hold_cube_fit_capped),
    'fit_frame_psf_free.max_outer_0': (run_frame_free_no_outer, hold_frame_free_no_outer),
    'fit_frame_psf_free.max_iter_1': (run_frame_free_capped, hold_frame_free_capped),
    'fit_cube_psf_free.max_outer_0': (run_cube_free_no_outer, hold_cube_free_no_outer),
    'fit_cube_psf_free.max_iter_1': (run_cube_free_capped, hold_cube_free_capped),
})
VARIANTS = tuple(k for k in CHECKED if '.' in k)


# ---- the predecessors -----------------------------------------------------------------------------------------------

def _large(nl=0, wild=False):
    return field(LARGE, 56, 21, nl=nl, wild=wild)              # (56 + 1 stars: 1.5 times the 34 of the fit scene and more)


def _small(nl=0):
    return field(SMALL, 5, 22, nl=nl)


def _refused(rc):
    assert rc == E_INVALID, rc


def _cube_host_batches(api, ctx):
    """The host form of fit_cube_psf on the five layers of cube_fit_cases two at a time: a ragged last batch, the
    staging buffer laid out for one batch and refilled batch by batch."""
    cube_fit(ctx, K.cube(), layer_batch=2)


def _cube_host_small(api, ctx):
    cube_fit(ctx, _small(2), layer_batch=1)


def _render_pile(api, ctx):
    render(ctx, Y.scene(), subtract=False)


def _dead_layer(c, l=1):
    d = dict(c, cube=c['cube'].copy())
    d['cube'][l] = np.nan
    return d


_BACK_SCENES = {}


def _back_scenes():
    """The frames of the background predecessors: `cube` 3 x 200 x 310 with var and apply (every array of the checked
    call lies over its planes in the staging buffer), `tiny` 9 x 11, `large` the L frame of the suite with a NaN tile
    and its variances."""
    if not _BACK_SCENES:
        rng = np.random.default_rng(31)
        shape = (3, 200, 310)
        lf = _large()
        tile = lf['image'].copy()
        tile[32:64, 64:96] = np.nan
        _BACK_SCENES.update(cube=rng.normal(size=shape) + 4.0, cube_var=rng.uniform(0.5, 1.5, shape),
                            cube_apply=rng.normal(size=shape), tiny=rng.normal(size=(9, 11)), large=tile,
                            large_var=lf['var'])
    return _BACK_SCENES


def _background_large(api, ctx):
    """X_background: the staging buffer's newest tenant before a frame call -- three input and five output planes."""
    b = _back_scenes()
    out = background(ctx, b['large'], b['large_var'], b['large'], box=32, filter=3)
    assert out['head'][0, 0] == 1.0 and out['applied'] is not None


def _fit_family(call, scene, large, small, wild, other, kw, free):
    """The predecessors of a frame or cube fit: `call` is the entry point on a scene dict, `other` the other tenant of
    its workspace, `kw` the solver's keywords of the checked call, `free` whether the positions are free."""
    p = {
        'L_larger': lambda api, ctx: call(ctx, large(), **kw),
        'S_smaller': lambda api, ctx: call(ctx, small(), **kw),
        'X_other_tenant': lambda api, ctx: other(ctx, scene()),
        'X_other_tenant_larger': lambda api, ctx: other(ctx, large()),
        'X_render_pile': _render_pile,
        'T_max_iter_1': lambda api, ctx: call(ctx, scene(), **dict(kw, max_iter=1)),
        'T_nothing_fitted': lambda api, ctx: call(ctx, lost_stars(scene()), **kw),
        'T_background_off': lambda api, ctx: call(ctx, scene(), background=False, **kw),
        'T_no_variance': lambda api, ctx: call(ctx, scene(), with_var=False, **kw),
        'N_non_finite': lambda api, ctx: call(ctx, wild(), **kw),
    }
    if free:
        p['T_max_outer_0'] = lambda api, ctx: call(ctx, scene(), **dict(kw, max_outer=0))
        p['T_max_outer_6'] = lambda api, ctx: call(ctx, scene(), **dict(kw, max_outer=6, max_step=0.5))
        p['T_all_held'] = lambda api, ctx: call(ctx, scene(), **dict(kw, max_outer=3, min_snr=1e30))
        p['T_none_held'] = lambda api, ctx: call(ctx, scene(), **dict(kw, max_outer=3, min_snr=0.0))
    return p


def _frame_refusal(api, ctx):
    _refused(_fit_test()._raw(ctx, F.scene(), radius=0.5)[0])


def _frame_free_refusal(api, ctx):
    import test_gpu_frame_free as T
    _refused(T._raw(ctx, G.displaced_scene(True), max_step=0.0)[0])


def _cube_refusal(api, ctx):
    import test_gpu_cube_fit as T
    _refused(T._raw(ctx, Q.cube(True), radius=0.5)[0])


def _cube_free_refusal(api, ctx):
    import test_gpu_cube_free as T
    _refused(T._raw(ctx, Q.cube(True), max_step=0.0)[0])


def _solver(module):
    import importlib
    T = importlib.import_module(module)
    return dict(max_iter=T.MAX_ITER, tol=T.TOL)


def _predecessors():
    P = {}
    # render_stars
    big, tiny = render_scene(field(LARGE, 560, 23)), render_scene(_small())
    ys = Y.scene()
    P['render_stars'] = {
        'L_larger': lambda api, ctx: render(ctx, big, subtract=True),
        'S_smaller': lambda api, ctx: render(ctx, tiny, subtract=True),
        'X_frame_fit': lambda api, ctx: frame_fit(ctx, F.scene()),
        'X_frame_free': lambda api, ctx: frame_free(ctx, G.displaced_scene(True), max_outer=2),
        'T_nothing_on_the_frame': lambda api, ctx: render(ctx, lost_stars(ys), subtract=True),
        'T_added_to_zeros': lambda api, ctx: render(ctx, dict(ys, shape=Y.FRAME), image=None),
        'N_non_finite': lambda api, ctx: render(ctx, dict(ys, scale=ys['scale'] * 1e300), image=wild_copy(ys['image'])),
        'F_refused': lambda api, ctx: _refused(ctx.lib.mpsfr_render_stars(
            ctx._h, 97, 150, None, 0, 4, None, None, None, None, None, 0, None, None, 0)),
    }
    # cut_stamps
    cim, cva, cor = _cut_inputs()
    lf = _large()
    P['cut_stamps'] = {
        'L_larger': lambda api, ctx: cut(ctx, lf['image'], lf['var'], lf['origin']),
        'S_smaller_no_var': lambda api, ctx: cut(ctx, _small()['image'], None, _small()['origin'][:2]),
        'N_non_finite': lambda api, ctx: cut(ctx, wild_copy(cim), wild_copy(cva, 42), cor),
        'X_cube_host': _cube_host_small,
        'F_refused': lambda api, ctx: _refused(ctx.lib.mpsfr_cut_stamps(ctx._h, 97, 150, None, None, 0, None, None,
                                                                         None, 0)),
    }
    # find_stars
    fs = FI.scene()
    thr = FI.THRESHOLD[True]
    P['find_stars'] = {
        'L_larger': lambda api, ctx: _find(ctx, lf['image'], fs['psf'], lf['var'], max_stars=600),
        'S_smaller': lambda api, ctx: _find(ctx, _small()['image'], fs['psf'], _small()['var'], max_stars=7),
        'T_without_map': lambda api, ctx: _find(ctx, fs['image'], fs['psf'], fs['var'], threshold=thr, want_map=False),
        'T_without_origin': lambda api, ctx: _find(ctx, fs['image'], fs['psf'], fs['var'], threshold=thr,
                                                   want_origin=False),
        'T_more_peaks_than_max_stars': lambda api, ctx: _find(ctx, fs['image'], fs['psf'], fs['var'], threshold=thr,
                                                              max_stars=4),
        'T_no_variance_half_8': lambda api, ctx: _find(ctx, fs['image'], fs['psf'], None, half=8, sep=16,
                                                       threshold=FI.THRESHOLD[False]),
        'T_no_peaks': lambda api, ctx: _find(ctx, fs['image'], fs['psf'], fs['var'], threshold=1e300),
        'N_non_finite': lambda api, ctx: _find(ctx, wild_copy(fs['image']), fs['psf'], fs['var'], threshold=thr),
        'X_render_pile': _render_pile,
        'F_refused': lambda api, ctx: _find(ctx, fs['image'], fs['psf'], fs['var'], expect_rc=E_INVALID,
                                            override=dict(half=0)),
    }
    # group_stars
    pos, crit, shape = GR.scenes()['field']
    chains = GR.chains_scene()
    wide = GR.wide_scene()
    gone = pos.copy()
    gone[::3, 0] = np.nan                      # (a finite position off the frame is refused: NaN is the only filler)
    gone[1::3, 1] = np.nan
    P['group_stars'] = {
        'L_larger': lambda api, ctx: _group(ctx, GR.random_field(9, 2300, (260, 260)), crit, (260, 260)),
        'S_smaller': lambda api, ctx: _group(ctx, *wide),
        'T_oversize_chains': lambda api, ctx: _group(ctx, *chains),
        'T_max_groups_too_small': lambda api, ctx: _group(ctx, pos, crit, shape, max_groups=5),
        'T_chains_max_groups_2': lambda api, ctx: _group(ctx, *chains, max_groups=2),
        'T_without_tables': lambda api, ctx: _group(ctx, pos, crit, shape, tables=False),
        'T_widest_crit': lambda api, ctx: _group(ctx, pos, 16.0, shape),
        'N_fillers': lambda api, ctx: _group(ctx, gone, crit, shape),
        'X_find': lambda api, ctx: _find(ctx, fs['image'], fs['psf'], fs['var'], threshold=thr),
        'F_refused': lambda api, ctx: _group(ctx, pos, crit, shape, expect_rc=E_INVALID, override=dict(crit=-1.0)),
    }
    # the frame fits
    kw = _solver('test_gpu_frame_fit')
    P['fit_frame_psf'] = _fit_family(frame_fit, F.scene, _large, _small, lambda: _large(wild=True),
                                     lambda ctx, s: frame_free(ctx, s, max_outer=3), kw, False)
    P['fit_frame_psf']['F_refused'] = _frame_refusal
    kw = dict(_solver('test_gpu_frame_free'), max_outer=1, **ONE_STEP)
    P['fit_frame_psf_free'] = _fit_family(frame_free, lambda: G.displaced_scene(True), _large, _small,
                                          lambda: _large(wild=True), lambda ctx, s: frame_fit(ctx, s), kw, True)
    P['fit_frame_psf_free']['F_refused'] = _frame_free_refusal
    # the cube fits
    cube = lambda: Q.cube(True)                                                       # noqa: E731
    kw = _solver('test_gpu_frame_fit')
    P['fit_cube_psf'] = _fit_family(cube_fit, cube, lambda: _large(5), lambda: _small(2),
                                    lambda: _large(5, wild=True), lambda ctx, c: cube_free(ctx, c, max_outer=3), kw,
                                    False)
    P['fit_cube_psf'].update({
        'X_host_batches_of_2': _cube_host_batches,
        'T_dead_layer_1': lambda api, ctx: cube_fit(ctx, _dead_layer(Q.cube(True)), **kw),
        'T_one_layer_at_a_time': lambda api, ctx: cube_fit(ctx, Q.cube(True), layer_batch=1, **kw),
        'F_refused': _cube_refusal})
    kwf = dict(_solver('test_gpu_cube_free'), max_outer=1, **CUBE_STEP)
    P['fit_cube_psf_free'] = _fit_family(cube_free, cube, lambda: _large(5), lambda: _small(2),
                                         lambda: _large(5, wild=True), lambda ctx, c: cube_fit(ctx, c), kwf, True)
    P['fit_cube_psf_free'].update({
        'X_host_batches_of_2': _cube_host_batches,
        'T_dead_layer_1': lambda api, ctx: cube_free(ctx, _dead_layer(Q.cube(True)), **kwf),
        'F_refused': _cube_free_refusal})
    # frame_background: a tenant of the staging buffer with no workspace of its own
    bs, bk = BG.scene(), _back_scenes()
    P['frame_background'] = {
        'L_larger': lambda api, ctx: background(ctx, bk['cube'], bk['cube_var'], bk['cube_apply'], box=64, filter=5),
        'S_smaller': lambda api, ctx: background(ctx, bk['tiny'], None, bk['tiny'], box=8, filter=1),
        'X_find': lambda api, ctx: _find(ctx, fs['image'], fs['psf'], fs['var'], threshold=thr),
        'X_frame_fit': lambda api, ctx: frame_fit(ctx, F.scene()),
        'X_cube_host': _cube_host_small,
        'T_all_dead': lambda api, ctx: background(ctx, np.full(BG.FRAME, np.nan), bs['var'], bs['apply']),
        'T_mesh_only': lambda api, ctx: background(ctx, bs['image'], bs['var'], None, want=()),
        'N_non_finite': lambda api, ctx: background(ctx, wild_copy(bs['image']), wild_copy(bs['var'], 42),
                                                    wild_copy(bs['apply'], 43)),
        'F_refused': lambda api, ctx: _refused(background(ctx, bs['image'], expect_rc=E_INVALID, box=7)['rc']),
    }
    # ... and a predecessor of the frame calls and of cut_stamps
    for name in AFTER_BACKGROUND:
        P[name]['X_background'] = _background_large
    # the variants: the family of their entry point at the variant's own keywords, and the checked call before them
    def variant(name, base, call, scene, large, small, other, kw, free, refusal, extra=()):
        p = _fit_family(call, scene, large, small, (lambda: large(wild=True)), other, kw, free)
        p['T_checked_call'] = lambda api, ctx: CHECKED[base][0](api, ctx)
        if free:
            p['T_max_outer_6_converging'] = lambda api, ctx: call(ctx, scene(), max_outer=6, max_iter=100, tol=1e-10)
        p['F_refused'] = refusal
        p.update(extra)
        P[name] = p
    lc, sc = (lambda wild=False: _large(5, wild=wild)), (lambda: _small(2))
    both = {'X_host_batches_of_2': _cube_host_batches}
    tf, tc = _solver('test_gpu_frame_fit')['tol'], _solver('test_gpu_cube_free')['tol']
    variant('fit_frame_psf.max_iter_1', 'fit_frame_psf', frame_fit, F.scene, _large, _small,
            lambda ctx, s: frame_free(ctx, s, max_outer=3), dict(max_iter=1, tol=tf), False, _frame_refusal)
    variant('fit_cube_psf.max_iter_1', 'fit_cube_psf', cube_fit, cube, lc, sc,
            lambda ctx, c: cube_free(ctx, c, max_outer=3), dict(max_iter=1, tol=tf), False, _cube_refusal, both)
    dscene = lambda: G.displaced_scene(True)                                          # noqa: E731
    variant('fit_frame_psf_free.max_outer_0', 'fit_frame_psf_free', frame_free, dscene, _large, _small,
            lambda ctx, s: frame_fit(ctx, s), dict(max_outer=0, max_iter=100, tol=1e-10), True, _frame_free_refusal)
    variant('fit_frame_psf_free.max_iter_1', 'fit_frame_psf_free', frame_free, dscene, _large, _small,
            lambda ctx, s: frame_fit(ctx, s), dict(max_iter=1, tol=tf, max_outer=1, **ONE_STEP), True,
            _frame_free_refusal)
    variant('fit_cube_psf_free.max_outer_0', 'fit_cube_psf_free', cube_free, cube, lc, sc,
            lambda ctx, c: cube_fit(ctx, c), dict(max_outer=0, max_iter=100, tol=tc), True, _cube_free_refusal, both)
    variant('fit_cube_psf_free.max_iter_1', 'fit_cube_psf_free', cube_free, cube, lc, sc,
            lambda ctx, c: cube_fit(ctx, c), dict(max_iter=1, tol=tc, max_outer=1, **CUBE_STEP), True,
            _cube_free_refusal, both)
    P['find_stars.no_map'] = {
        'T_with_map': lambda api, ctx: run_find(api, ctx),
        'T_without_origin': lambda api, ctx: _find(ctx, fs['image'], fs['psf'], fs['var'], threshold=thr,
                                                   want_map=False, want_origin=False),
        'L_larger': lambda api, ctx: _find(ctx, lf['image'], fs['psf'], lf['var'], max_stars=600, want_map=False),
        'S_smaller': lambda api, ctx: _find(ctx, _small()['image'], fs['psf'], _small()['var'], max_stars=7,
                                            want_map=False),
        'N_non_finite': lambda api, ctx: _find(ctx, wild_copy(fs['image']), fs['psf'], fs['var'], threshold=thr,
                                               want_map=False),
        'X_render_pile': _render_pile,
        'F_refused': lambda api, ctx: _find(ctx, fs['image'], fs['psf'], fs['var'], expect_rc=E_INVALID,
                                            want_map=False, override=dict(half=0)),
    }
    # the stamp calls: the staging buffer alone (and specx)
    data, var, psf, _ = PF.noisy_stars(True, 37, 12)
    few = slice(0, 3)

    def stamp_family(larger, smaller, wild, refusal):
        return {'L_more_stamps': larger, 'S_fewer_stamps': smaller, 'N_non_finite': wild, 'X_cube_host': _cube_host_small,
                'X_cube_host_batches_of_2': _cube_host_batches, 'F_refused': refusal}
    P['fit_stamps_elliptical'] = stamp_family(
        lambda api, ctx: ctx.fit_stamps_elliptical(psf), lambda api, ctx: ctx.fit_stamps_elliptical(psf[few]),
        lambda api, ctx: ctx.fit_stamps_elliptical(psf[:20] * 1e300),
        lambda api, ctx: _refused(ctx.lib.mpsfr_fit_stamps_elliptical(ctx._h, 0, None, None, 0)))
    P['fit_stamps_observed'] = stamp_family(
        lambda api, ctx: ctx.fit_stamps_observed(np.tile(data, (2, 1, 1)), np.tile(var, (2, 1, 1)), circular=False),
        lambda api, ctx: ctx.fit_stamps_observed(data[few], None, background=False),
        lambda api, ctx: ctx.fit_stamps_observed(wild_copy(data), var, circular=False),
        lambda api, ctx: _refused(ctx.lib.mpsfr_fit_stamps_observed(ctx._h, 0, None, None, 0, None, 0)))
    P['fit_stamps_psf'] = stamp_family(
        lambda api, ctx: ctx.fit_stamps_psf(data, psf, var=var),
        lambda api, ctx: ctx.fit_stamps_psf(data[few], psf[few], background=False),
        lambda api, ctx: ctx.fit_stamps_psf(wild_copy(data), psf, var=var),
        lambda api, ctx: _refused(ctx.lib.mpsfr_fit_stamps_psf(ctx._h, 0, None, None, 0, None, None, None, 0, None, 0)))

    def blends(K, back, mode):
        d = PG.groups(K, back)
        return d[0], d[1], d[2], None, None, None, PG.given_positions(d[4], mode)
    g4, g2, g3 = blends(4, True, 'free'), blends(2, False, 'fixed'), blends(*GROUP_CASE)
    P['fit_groups_psf'] = stamp_family(
        lambda api, ctx: ctx.fit_groups_psf(np.tile(g4[0], (3, 1, 1)), np.tile(g4[2], (3, 1, 1)),
                                                  np.tile(g4[6], (3, 1, 1)), var=np.tile(g4[1], (3, 1, 1))),
        lambda api, ctx: ctx.fit_groups_psf(g2[0][few], g2[2][few], g2[6][few], background=False, mode='fixed'),
        lambda api, ctx: ctx.fit_groups_psf(wild_copy(g3[0]), g3[2], g3[6], var=g3[1]),
        lambda api, ctx: _refused(ctx.lib.mpsfr_fit_groups_psf(ctx._h, 0, 2, None, None, 0, None, None, None, 0, None,
                                                               0)))
    ss = SR.stars(True, True)
    deep = [ss[4], ss[5]] * 3
    other_x = ss[2]['x'] ** 3
    wild_star = dict(ss[0], cube=wild_copy(ss[0]['cube']))

    def drifts(api, ctx):
        spectra(ctx, deep)                                                            # one x of 12 layers
        spectra(ctx, ss[2:4], x=other_x)                                              # another x, of 5 layers
        spectra(ctx, ss[2:4], drift=False)                                            # no drift: specx is not written
    P['fit_spectra_psf'] = stamp_family(
        lambda api, ctx: spectra(ctx, deep), lambda api, ctx: spectra(ctx, ss[3:4], drift=False, back=False),
        lambda api, ctx: spectra(ctx, [wild_star, ss[1]]),
        lambda api, ctx: _refused(ctx.lib.mpsfr_fit_spectra_psf(ctx._h, 0, 5, None, None, 0, None, None, None, None, 0,
                                                                None, 0)))
    P['fit_spectra_psf']['T_drift_x_then_another_x_then_none'] = drifts
    import test_gpu_metrics as TM
    P['stamp_metrics'] = stamp_family(
        lambda api, ctx: ctx.stamp_metrics(psf, TM.RADII, TM.BOXES, TM.FRACS),
        lambda api, ctx: ctx.stamp_metrics(psf[few], TM.RADII[:2], (), ()),
        lambda api, ctx: ctx.stamp_metrics(wild_copy(data), TM.RADII, TM.BOXES, TM.FRACS),
        lambda api, ctx: _refused(ctx.lib.mpsfr_stamp_metrics(ctx._h, 0, None, None, 0, None, 0, None, 0, None, None,
                                                              0)))
    return P


_PRED = {}


def predecessors():
    if not _PRED:
        _PRED.update(_predecessors())
    return _PRED


# The labels, known without building a scene (the parametrisation of the tests)
_FIT = ['L_larger', 'S_smaller', 'X_other_tenant', 'X_other_tenant_larger', 'X_render_pile', 'T_max_iter_1',
        'T_nothing_fitted', 'T_background_off', 'T_no_variance', 'N_non_finite', 'F_refused']
_FREE = ['T_max_outer_0', 'T_max_outer_6', 'T_all_held', 'T_none_held']
_STAMP = ['L_more_stamps', 'S_fewer_stamps', 'N_non_finite', 'X_cube_host', 'X_cube_host_batches_of_2', 'F_refused']
_BACK = ['X_background']                       # of AFTER_BACKGROUND
LABELS = {
    'render_stars': ['L_larger', 'S_smaller', 'X_frame_fit', 'X_frame_free', 'T_nothing_on_the_frame',
                     'T_added_to_zeros', 'N_non_finite', 'F_refused'] + _BACK,
    'cut_stamps': ['L_larger', 'S_smaller_no_var', 'N_non_finite', 'X_cube_host', 'F_refused'] + _BACK,
    'find_stars': ['L_larger', 'S_smaller', 'T_without_map', 'T_without_origin', 'T_more_peaks_than_max_stars',
                   'T_no_variance_half_8', 'T_no_peaks', 'N_non_finite', 'X_render_pile', 'F_refused'] + _BACK,
    'group_stars': ['L_larger', 'S_smaller', 'T_oversize_chains', 'T_max_groups_too_small', 'T_chains_max_groups_2',
                    'T_without_tables', 'T_widest_crit', 'N_fillers', 'X_find', 'F_refused'] + _BACK,
    'fit_frame_psf': _FIT + _BACK,
    'fit_frame_psf_free': _FIT + _FREE + _BACK,
    'fit_cube_psf': _FIT + ['X_host_batches_of_2', 'T_dead_layer_1', 'T_one_layer_at_a_time'] + _BACK,
    'fit_cube_psf_free': _FIT + _FREE + ['X_host_batches_of_2', 'T_dead_layer_1'] + _BACK,
    'fit_stamps_elliptical': _STAMP,
    'fit_stamps_observed': _STAMP,
    'fit_stamps_psf': _STAMP,
    'fit_groups_psf': _STAMP,
    'fit_spectra_psf': _STAMP + ['T_drift_x_then_another_x_then_none'],
    'stamp_metrics': _STAMP,
    'frame_background': ['L_larger', 'S_smaller', 'X_find', 'X_frame_fit', 'X_cube_host', 'T_all_dead', 'T_mesh_only',
                         'N_non_finite', 'F_refused'],
    'find_stars.no_map': ['T_with_map', 'T_without_origin', 'L_larger', 'S_smaller', 'N_non_finite', 'X_render_pile',
                          'F_refused'],
    'fit_frame_psf.max_iter_1': _FIT + ['T_checked_call'],
    'fit_cube_psf.max_iter_1': _FIT + ['T_checked_call', 'X_host_batches_of_2'],
    'fit_frame_psf_free.max_outer_0': _FIT + _FREE + ['T_checked_call', 'T_max_outer_6_converging'],
    'fit_frame_psf_free.max_iter_1': _FIT + _FREE + ['T_checked_call', 'T_max_outer_6_converging'],
    'fit_cube_psf_free.max_outer_0': _FIT + _FREE + ['T_checked_call', 'T_max_outer_6_converging', 'X_host_batches_of_2'],
    'fit_cube_psf_free.max_iter_1': _FIT + _FREE + ['T_checked_call', 'T_max_outer_6_converging', 'X_host_batches_of_2'],
}
# f64: the frame and cube calls run the same fp64 kernels in both modes -- L, X and one T per checked call; the stamp
# calls have kernels of their own per mode and run their whole list
_F64_FRAME = ('L_larger', 'X_other_tenant', 'X_cube_host', 'X_frame_fit', 'X_find', 'X_render_pile', 'T_max_iter_1',
              'T_without_map', 'T_oversize_chains', 'T_nothing_on_the_frame', 'T_checked_call', 'T_with_map',
              'X_background', 'T_mesh_only')
F64_LABELS = {name: [p for p in labels if p in _F64_FRAME]
              if name in FRAME_CALLS + VARIANTS + ('cut_stamps',) else list(labels)
              for name, labels in LABELS.items()}


def run_all(api, ctx):
    """P9 of tests/test_gpu_call_history.py: every checked call once, in the order of CHECKED."""
    for run, _ in CHECKED.values():
        run(api, ctx)


# ---- the device forms: every output into a buffer prefilled with the byte 0xA5 ---------------------------------------

SENTINEL = 0xA5
TAIL = 256                                     # bytes of sentinel behind every output buffer


class DeviceOutputs:
    """Output buffers of a device-form call: each as many bytes as the header documents for the array and TAIL more, all
    holding SENTINEL before the call."""
    def __init__(self, torch):
        self.torch, self.bufs = torch, {}

    def new(self, key, shape, dtype=np.float64):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        buf = self.torch.full((nbytes + TAIL,), SENTINEL, dtype=self.torch.uint8, device=self.torch.device('cuda:0'))
        self.bufs[key] = (buf, tuple(shape), np.dtype(dtype), nbytes)
        return buf.data_ptr()

    def fetch(self):
        """({key: array}, {key: bytes of the tail that no longer hold the sentinel})"""
        out, tails = {}, {}
        for key, (buf, shape, dtype, nbytes) in self.bufs.items():
            raw = buf.cpu().numpy()
            out[key] = raw[:nbytes].copy().view(dtype).reshape(shape)
            tails[key] = int(np.sum(raw[nbytes:] != SENTINEL))
        return out, tails


def holds_sentinel(a):
    """The elements of `a` whose bytes are all SENTINEL: what a call that skipped them would leave."""
    return np.all(bits(a) == SENTINEL, axis=-1)


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda:0'))


def dev_render(api, ctx, torch, o):
    s = Y.scene()
    ny, nx = s['image'].shape
    t = {k: _up(torch, s[k]) for k in ('image', 'psf', 'origin', 'shift', 'scale', 'index')}
    ctx.render_stars_device(ny, nx, s['n'], len(s['psf']), t['psf'].data_ptr(), t['origin'].data_ptr(),
                            t['scale'].data_ptr(), o.new('frame', (ny, nx)), image_ptr=t['image'].data_ptr(),
                            shift_ptr=t['shift'].data_ptr(), psf_index_ptr=t['index'].data_ptr(),
                            star_out_ptr=o.new('rows', (s['n'], 4)), subtract=True)
    return t


def dev_cut(api, ctx, torch, o):
    image, var, origin = _cut_inputs()
    t = [_up(torch, a) for a in (image, var, origin)]
    n = len(origin)
    ctx.cut_stamps_device(image.shape[0], image.shape[1], t[0].data_ptr(), n, t[2].data_ptr(),
                          o.new('stamps', (n, NS, NS)), var_ptr=t[1].data_ptr(), var_stamps_ptr=o.new('var', (n, NS, NS)))
    return t


def dev_find(api, ctx, torch, o):
    s = FI.scene()
    ny, nx = s['image'].shape
    t = [_up(torch, s[k]) for k in ('image', 'psf', 'var')]
    ctx.find_stars_device(ny, nx, t[0].data_ptr(), t[1].data_ptr(), 3, 3, FI.THRESHOLD[True], FIND_MAX,
                          o.new('rows', (FIND_MAX, 8)), o.new('count', (1,), np.int32), var_ptr=t[2].data_ptr(),
                          origin_ptr=o.new('origin', (FIND_MAX, 2), np.int32), map_ptr=o.new('map', (ny, nx)))
    return t


def dev_find_no_map(api, ctx, torch, o):
    s = FI.scene()
    ny, nx = s['image'].shape
    t = [_up(torch, s[k]) for k in ('image', 'psf', 'var')]
    ctx.find_stars_device(ny, nx, t[0].data_ptr(), t[1].data_ptr(), 3, 3, FI.THRESHOLD[True], FIND_MAX,
                          o.new('rows', (FIND_MAX, 8)), o.new('count', (1,), np.int32), var_ptr=t[2].data_ptr(),
                          origin_ptr=o.new('origin', (FIND_MAX, 2), np.int32))
    return t


def dev_group(api, ctx, torch, o):
    pos, crit, shape = GR.scenes()['field']
    n = len(pos)
    t = _up(torch, pos)
    ctx.group_stars_device(shape[0], shape[1], n, t.data_ptr(), 2, crit, n, o.new('label', (n,), np.int32),
                           o.new('groups', (n, 8), np.int32), o.new('counts', (6,), np.int32),
                           origin_ptr=o.new('origin', (n, 2), np.int32), shift_ptr=o.new('shift', (n * 8,)))
    return t


def _frame_inputs(torch, s, image='image'):
    return {k: _up(torch, s[k]) for k in (image, 'var', 'psf', 'origin', 'shift', 'index')
            + (('layer_shift',) if image == 'cube' else ())}


def dev_frame_fit(api, ctx, torch, o):
    s = F.scene()
    ny, nx = s['image'].shape
    t = _frame_inputs(torch, s)
    ctx.fit_frame_psf_device(ny, nx, t['image'].data_ptr(), s['n'], len(s['psf']), t['psf'].data_ptr(),
                             t['origin'].data_ptr(), o.new('rows', (s['n'], 8)), o.new('head', (8,)),
                             var_ptr=t['var'].data_ptr(), shift_ptr=t['shift'].data_ptr(),
                             psf_index_ptr=t['index'].data_ptr(), resid_ptr=o.new('resid', (ny, nx)),
                             **_solver('test_gpu_frame_fit'))
    return t


def dev_frame_free(api, ctx, torch, o):
    s = G.displaced_scene(True)
    ny, nx = s['image'].shape
    t = _frame_inputs(torch, s)
    ctx.fit_frame_psf_free_device(ny, nx, t['image'].data_ptr(), s['n'], len(s['psf']), t['psf'].data_ptr(),
                                  t['origin'].data_ptr(), o.new('rows', (s['n'], 16)), o.new('shifts', (s['n'], 2)),
                                  o.new('head', (12,)), var_ptr=t['var'].data_ptr(), shift_ptr=t['shift'].data_ptr(),
                                  psf_index_ptr=t['index'].data_ptr(), resid_ptr=o.new('resid', (ny, nx)), max_outer=1,
                                  **_solver('test_gpu_frame_free'), **ONE_STEP)
    return t


def dev_cube_fit(api, ctx, torch, o):
    c = Q.cube(True)
    nl, ny, nx = c['cube'].shape
    t = _frame_inputs(torch, c, 'cube')
    ctx.fit_cube_psf_device(nl, ny, nx, t['cube'].data_ptr(), c['n'], len(c['psf']), t['psf'].data_ptr(),
                            t['origin'].data_ptr(), o.new('rows', (nl, c['n'], 8)), o.new('head', (nl, 8)),
                            var_ptr=t['var'].data_ptr(), shift_ptr=t['shift'].data_ptr(),
                            layer_shift_ptr=t['layer_shift'].data_ptr(), psf_index_ptr=t['index'].data_ptr(),
                            resid_ptr=o.new('resid', (nl, ny, nx)), **_solver('test_gpu_frame_fit'))
    return t


def dev_cube_free(api, ctx, torch, o):
    c = Q.cube(True)
    nl, ny, nx = c['cube'].shape
    n = c['n']
    t = _frame_inputs(torch, c, 'cube')
    ctx.fit_cube_psf_free_device(nl, ny, nx, t['cube'].data_ptr(), n, len(c['psf']), t['psf'].data_ptr(),
                                 t['origin'].data_ptr(), o.new('rows', (nl, n, 8)), o.new('head', (nl, 8)),
                                 o.new('pos', (n, 8)), o.new('shifts', (n, 2)), o.new('call', (8,)),
                                 var_ptr=t['var'].data_ptr(), shift_ptr=t['shift'].data_ptr(),
                                 layer_shift_ptr=t['layer_shift'].data_ptr(), psf_index_ptr=t['index'].data_ptr(),
                                 resid_ptr=o.new('resid', (nl, ny, nx)), max_outer=1,
                                 **_solver('test_gpu_cube_free'), **CUBE_STEP)
    return t


def dev_background(api, ctx, torch, o):
    s = BG.scene()
    ny, nx = s['image'].shape
    my, mx = BG.mesh_shape(ny, nx, BG.DEFAULTS['box'])
    t = [_up(torch, np.array(s[k])) for k in ('image', 'var', 'apply')]          # (the scene's arrays are read-only)
    ctx.frame_background_device(1, ny, nx, t[0].data_ptr(), o.new('mesh', (1, my, mx, 8)), o.new('head', (1, 4)),
                                var_ptr=t[1].data_ptr(), map_ptr=o.new('map', (ny, nx)), rms_ptr=o.new('rms', (ny, nx)),
                                apply_to_ptr=t[2].data_ptr(), applied_ptr=o.new('applied', (ny, nx)), **BG.DEFAULTS)
    return t


def dev_fit_ell(api, ctx, torch, o):
    st = _up(torch, np.array([M.stamp(*p) for p in _ell_pars()]))
    ctx.fit_stamps_elliptical_device(len(st), st.data_ptr(), o.new('fit', (len(st), api.NFIT_ELL)))
    return st


def dev_fit_obs(api, ctx, torch, o):
    import test_gpu_fit_obs as T
    data, var, _ = T._yardstick(True, True)
    t = [_up(torch, data), _up(torch, var)]
    ctx.fit_stamps_observed_device(len(data), t[0].data_ptr(), o.new('fit', (len(data), api.NFIT_ELL)),
                                   var_ptr=t[1].data_ptr(), background=True, circular=False)
    return t


def dev_fit_psf(api, ctx, torch, o):
    data, var, psf, _, shift, _ = PF.yardstick(True, False)
    assert shift is None
    t = [_up(torch, a) for a in (data, var, psf)]
    ctx.fit_stamps_psf_device(len(data), t[0].data_ptr(), len(psf), t[2].data_ptr(),
                              o.new('fit', (len(data), api.NFIT_PSF)), var_ptr=t[1].data_ptr(), background=True)
    return t


def dev_fit_groups(api, ctx, torch, o):
    data, var, psf, _, _, _, given, _ = PG.yardstick(*GROUP_CASE)
    t = [_up(torch, a) for a in (data, var, psf, given)]
    ctx.fit_groups_psf_device(len(data), given.shape[1], t[0].data_ptr(), len(psf), t[2].data_ptr(), t[3].data_ptr(),
                              o.new('fit', (len(data), api.NFIT_GROUP)), var_ptr=t[1].data_ptr(), background=True,
                              mode='free')
    return t


def dev_fit_spectra(api, ctx, torch, o):
    ss = [SR.stars(True, True)[k] for k in SPEC_STARS]
    cubes, var, psf, sh = SR.batch(ss)
    assert sh is None
    n, nl = cubes.shape[:2]
    t = [_up(torch, a) for a in (cubes, var, psf)]
    ctx.fit_spectra_psf_device(n, nl, t[0].data_ptr(), n, t[2].data_ptr(),
                               o.new('fit', (n, api.NFIT_SPEC + api.NFIT_SPEC_LAYER * nl)), var_ptr=t[1].data_ptr(),
                               background=True, x=ss[0]['x'])
    return t


def dev_metrics(api, ctx, torch, o):
    import test_gpu_metrics as T
    st = _up(torch, _metric_stamps())
    ctx.stamp_metrics_device(len(st), st.data_ptr(), o.new('rows', (len(st), T.HEAD + len(T.RADII) + len(T.BOXES))),
                             T.RADII, T.BOXES, ())
    return st


def _spectra_split(api, out):
    fit = out.pop('fit')
    n = fit.shape[0]
    out['head'] = fit[:, :api.NFIT_SPEC].copy()
    out['layers'] = fit[:, api.NFIT_SPEC:].reshape(n, -1, api.NFIT_SPEC_LAYER).copy()


DEVICE = {
    'render_stars': dev_render, 'cut_stamps': dev_cut, 'find_stars': dev_find, 'find_stars.no_map': dev_find_no_map,
    'group_stars': dev_group,
    'fit_frame_psf': dev_frame_fit, 'fit_frame_psf_free': dev_frame_free, 'fit_cube_psf': dev_cube_fit,
    'fit_cube_psf_free': dev_cube_free, 'fit_stamps_elliptical': dev_fit_ell, 'fit_stamps_observed': dev_fit_obs,
    'fit_stamps_psf': dev_fit_psf, 'fit_groups_psf': dev_fit_groups, 'fit_spectra_psf': dev_fit_spectra,
    'stamp_metrics': dev_metrics, 'frame_background': dev_background,
}


def device_run(api, ctx, torch, name):
    """The checked call `name` in its device form into sentinel buffers, synchronised: (outputs as run() names and
    shapes them, per output the tail bytes that were overwritten)."""
    o = DeviceOutputs(torch)
    torch.cuda.synchronize()
    keep = DEVICE[name](api, ctx, torch, o)              # (the inputs stay alive until the call has run)
    ctx.sync()
    torch.cuda.synchronize()
    out, tails = o.fetch()
    del keep
    if name == 'fit_spectra_psf':
        _spectra_split(api, out)
        tails = dict(head=tails['fit'], layers=tails['fit'])
    if name.startswith('find_stars'):
        out['count'] = np.asarray(int(out['count'][0]))
    return out, tails
