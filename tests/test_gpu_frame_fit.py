"""GPU: the crowded-field fit (mpsfr_fit_frame_psf), both precisions.

1. parity with the NumPy yardstick (frame_fit_ref) on the shared scene -- var on / off x background on / off x radius 4
   and 8: the scaled solution y = diag(N)^(1/2) x within the a-priori bound of the yardstick (convergence kappa tol |y*|
   plus the rounding terms derived there, not tuned), the integer columns and the statuses exact, chi2, overlap and N_kk
   within the bounds derived for them, the errors and fluxes from those.  Worst error / bound ratios go to
   record_margin('frame_fit', ...).
2. the residual frame equals render_stars(subtract) with the returned scales over the accepted stars, bit for bit.
3. bits: the same call twice, mixed = f64, host = device pointers, the power-of-two scaling laws.
4. the solver: a start at the solution needs at most two steps, max_iter = 1 ends with status 1 and finite rows; a
   permutation of the stars changes the result to rounding only.
5. the smallest shapes: a 1 x 1 frame, one star, a star across a tile corner of a 33 x 31 frame, 289 stars (more than
   one workgroup or wave of unknowns, a multiple of neither), two stars at one position.
6. the chain find -> fit_found_stars(crowded='frame') -> subtract_stars -> find on a rendered field with a chain of 6.
7. refusals: every MPSFR_E_INVALID of the header, outputs untouched.  8. profiling id and version.
"""
import ctypes as C

import numpy as np
import pytest

import find_ref as FR
import frame_fit_ref as F
from conftest import record_margin

pytestmark = pytest.mark.gpu

PRECS = ['mixed', 'f64']
NS = 40
TOL, MAX_ITER = 1e-10, 100
EPS = F.EPS


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


_CTX = {}


def _ctx(api, prec):
    if prec not in _CTX:
        _CTX[prec] = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision=prec)
    return _CTX[prec]


@pytest.fixture
def ctx(api, prec):
    return _ctx(api, prec)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _fit(ctx, s, with_var=True, background=True, radius=8.0, **kw):
    return ctx.fit_frame_psf(s['image'], s['psf'], s['origin'], var=s['var'] if with_var else None, shift=s['shift'],
                             psf_index=s['index'], radius=radius, background=background, **kw)


_BASE = {}


def _base(ctx, prec):
    """The fit of the scene (var, background, radius 8) with its residual, once per precision."""
    if prec not in _BASE:
        _BASE[prec] = _fit(ctx, F.scene(), return_residual=True)
    return _BASE[prec]


def _y_error(rows, head, ref):
    """|y_gpu - y_ref| in the 2-norm over all unknowns."""
    acc = ref['acc']
    x = np.concatenate([rows[acc, 0], [head[0]]]) if ref['background'] else rows[acc, 0]
    return float(np.linalg.norm((x - ref['x']) * np.sqrt(ref['dg'])))


def _check_against(rows, head, ref, b, tag=None):
    """Every column of a result against the yardstick and its bounds; returns the worst error / bound ratios."""
    acc, n = ref['acc'], len(ref['status'])
    out = np.setdiff1d(np.arange(n), acc)
    # the integer columns and the statuses: exact
    np.testing.assert_array_equal(rows[:, 7], ref['status'])
    np.testing.assert_array_equal(rows[:, 5], ref['ndisc'])
    assert not rows[out, :7].any()
    assert (head[3], head[6]) == (ref['nomega'], ref['nacc']) and head[7] == 0
    assert 1 <= head[4] <= MAX_ITER and 0 <= head[5] <= TOL
    ratios = dict(y=_y_error(rows, head, ref) / b['y'])
    dg = ref['dg'][:len(acc)]
    # F alone, N_kk, overlap
    assert np.all(np.abs(rows[acc, 0] - ref['F'][acc]) <= b['y'] / np.sqrt(dg))
    ratios['nkk'] = float(np.max(np.abs(rows[acc, 6] - ref['nkk'][acc]) / ref['nkk'][acc])) / b['nkk_rel']
    ratios['overlap'] = float(np.max(np.abs(rows[acc, 4] - ref['overlap'][acc]) / b['overlap']))
    ratios['chi2'] = abs(head[2] - ref['chi2']) / b['chi2']
    # the errors are sqrt((chi2 / dof) / N_kk) of the values beside them, the fluxes F sum P (1600 terms)
    dof = ref['nomega'] - ref['nacc'] - (1 if ref['background'] else 0)
    np.testing.assert_allclose(rows[acc, 1], np.sqrt(head[2] / dof / rows[acc, 6]), rtol=4 * EPS)
    sump = ref['flux'][acc] / ref['F'][acc]
    np.testing.assert_allclose(rows[acc, 2], rows[acc, 0] * sump, rtol=(NS * NS + 4) * EPS)
    np.testing.assert_allclose(rows[acc, 3], rows[acc, 1] * np.abs(sump), rtol=(NS * NS + 4) * EPS)
    rel = b['chi2'] / ref['chi2'] + b['nkk_rel'] + 8 * EPS
    np.testing.assert_allclose(rows[acc, 1], ref['err'][acc], rtol=rel)
    if ref['background']:
        assert abs(head[1] - ref['err_b']) <= rel * ref['err_b']
    else:
        assert head[0] == 0 and head[1] == 0
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
    if tag:
        print('frame fit %s: error / bound %s, %d iterations' %
              (tag, ', '.join('%s %.2e' % kv for kv in sorted(ratios.items())), head[4]))
        record_margin('frame_fit', **{'%s_%s' % (k, tag): v for k, v in ratios.items()})
    return ratios


# ---- 1. parity
@pytest.mark.parametrize('radius', [4.0, 8.0])
@pytest.mark.parametrize('background', [True, False])
@pytest.mark.parametrize('with_var', [True, False])
@pytest.mark.parametrize('prec', PRECS)
def test_parity_with_numpy_on_the_scene(ctx, prec, with_var, background, radius):
    s = F.scene()
    ref = F.scene_reference(with_var, background, radius)
    b = F.bounds(ref, TOL, MAX_ITER)
    rows, head = _fit(ctx, s, with_var, background, radius, max_iter=MAX_ITER, tol=TOL)
    assert rows.shape == (s['n'], 8) and head.shape == (8,)
    assert rows[s['off'], 7] == 1 and rows[s['dark'], 7] == 2
    tag = '%s_%s_%s_r%d' % (prec, 'var' if with_var else 'unit', 'back' if background else 'noback', int(radius))
    _check_against(rows, head, ref, b, tag)


# ---- 2. the residual frame is the renderer's
@pytest.mark.parametrize('prec', PRECS)
def test_residual_equals_render_subtract_bit_for_bit(ctx, prec):
    s = F.scene()
    rows, head, resid = _base(ctx, prec)
    acc = np.flatnonzero(rows[:, 7] == 0)
    assert len(acc) == head[6] and set(rows[:, 7]) == {0.0, 1.0, 2.0}
    want = ctx.render_stars(s['psf'], s['origin'][acc], rows[acc, 0], shift=s['shift'][acc], psf_index=s['index'][acc],
                            image=s['image'], subtract=True)
    assert _same(resid, want)
    assert np.array_equal(np.isnan(resid), np.isnan(s['image']))
    # it is image - sum F P~ of the yardstick to rounding, and b is not subtracted
    ref = F.scene_reference(True, True, 8.0)
    ok = ref['omega']
    assert np.max(np.abs(resid[ok] - ref['resid'][ok])) <= 1e-6 and abs(np.median(resid[ok]) - F.SKY) < 0.5
    # without the residual frame the rows are the same bits
    r2, h2 = _fit(ctx, s)
    assert _same(r2, rows) and _same(h2, head)


# ---- 3. bits
@pytest.mark.parametrize('prec', PRECS)
def test_same_call_twice_gives_the_same_bits(ctx, prec):
    rows, head, resid = _base(ctx, prec)
    r2, h2, d2 = _fit(ctx, F.scene(), return_residual=True)
    assert _same(r2, rows) and _same(h2, head) and _same(d2, resid)


def test_mixed_gives_the_bits_of_f64(api):
    a, b = _base(_ctx(api, 'mixed'), 'mixed'), _base(_ctx(api, 'f64'), 'f64')
    assert all(_same(x, y) for x, y in zip(a, b))


def _to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda:0'))


@pytest.mark.parametrize('prec', PRECS)
def test_device_pointers_give_the_bits_of_the_host_form(ctx, prec):
    import torch
    s = F.scene()
    ny, nx = F.FRAME
    n = s['n']
    rows, head, resid = _base(ctx, prec)
    t = {k: _to_dev(torch, s[k]) for k in ('image', 'var', 'psf', 'index', 'origin', 'shift')}
    trow = torch.full((n, 8), -1.0, dtype=torch.float64, device=t['psf'].device)
    thead = torch.full((8,), -1.0, dtype=torch.float64, device=t['psf'].device)
    tres = torch.full((ny, nx), -1.0, dtype=torch.float64, device=t['psf'].device)
    torch.cuda.synchronize()
    ctx.fit_frame_psf_device(ny, nx, t['image'].data_ptr(), n, 4, t['psf'].data_ptr(), t['origin'].data_ptr(),
                             trow.data_ptr(), thead.data_ptr(), var_ptr=t['var'].data_ptr(),
                             shift_ptr=t['shift'].data_ptr(), psf_index_ptr=t['index'].data_ptr(),
                             resid_ptr=tres.data_ptr())
    ctx.sync()
    assert _same(trow.cpu().numpy(), rows) and _same(thead.cpu().numpy(), head) and _same(tres.cpu().numpy(), resid)
    # in the device form a star outside the domain is status 2 where the host form refuses the call
    bad = s['shift'].copy()
    bad[3, 0] = np.nan
    tbad = _to_dev(torch, bad)
    torch.cuda.synchronize()
    ctx.fit_frame_psf_device(ny, nx, t['image'].data_ptr(), n, 4, t['psf'].data_ptr(), t['origin'].data_ptr(),
                             trow.data_ptr(), thead.data_ptr(), var_ptr=t['var'].data_ptr(), shift_ptr=tbad.data_ptr(),
                             psf_index_ptr=t['index'].data_ptr())
    ctx.sync()
    got, h = trow.cpu().numpy(), thead.cpu().numpy()
    assert got[3, 7] == 2 and not got[3, :7].any() and h[6] == head[6] - 1 and h[7] == 0


@pytest.mark.parametrize('prec', PRECS)
def test_power_of_two_scaling_laws_hold_bit_for_bit(ctx, prec):
    s = F.scene()
    rows, head, resid = _base(ctx, prec)
    start = np.where(rows[:, 7] == 0, rows[:, 0] * 0.75, 0.0)
    r0, h0, d0 = _fit(ctx, s, scale0=start, return_residual=True)
    # a power of two on var: chi2 and N_kk scale with 1 / var, nothing else moves
    t = dict(s, var=s['var'] * 16.0)
    r1, h1, d1 = _fit(ctx, t, return_residual=True)
    for k in (0, 1, 2, 3, 4, 5, 7):
        assert _same(r1[:, k], rows[:, k]), k
    assert _same(r1[:, 6] * 16.0, rows[:, 6])
    assert _same(h1[[0, 1, 3, 4, 5, 6, 7]], head[[0, 1, 3, 4, 5, 6, 7]]) and h1[2] * 16.0 == head[2]
    assert _same(d1, resid)
    # 2^k on the data (and the start) with 4^k on var: F, b, the fluxes and their errors scale by 2^k
    for k in (3, -5):
        f = 2.0 ** k
        t = dict(s, image=s['image'] * f, var=s['var'] * f * f)
        r2, h2, d2 = _fit(ctx, t, scale0=start * f, return_residual=True)
        assert _same(r2[:, :4], r0[:, :4] * f) and _same(r2[:, [4, 5, 7]], r0[:, [4, 5, 7]])
        assert _same(r2[:, 6] * f * f, r0[:, 6])
        assert _same(h2[:2], h0[:2] * f) and _same(h2[2:], h0[2:])
        assert _same(d2, d0 * f)


# ---- 4. the solver
@pytest.mark.parametrize('prec', PRECS)
def test_start_at_the_solution_needs_at_most_two_steps(ctx, prec):
    # (without the background: b starts at 0 whatever scale0 is.  The stop rule is relative to the start's own
    # residual, so the tolerance is 1/4: tests/test_frame_fit_host.py shows that the textbook iteration then needs at
    # most two steps from the solution -- and falls far below it: a factor of 50 and more.)
    s = F.scene()
    ref = F.scene_reference(True, False, 8.0)
    b = F.bounds(ref, TOL, MAX_ITER)
    rows, head = _fit(ctx, s, background=False, max_iter=MAX_ITER, tol=TOL)
    r2, h2 = _fit(ctx, s, background=False, scale0=rows[:, 0], max_iter=MAX_ITER, tol=0.25)
    assert h2[7] == 0 and h2[4] <= 2 and h2[5] <= 0.25
    # the same answer within the bound: the first solve's, and kappa tol of it for the steps from there
    assert _y_error(r2, h2, ref) <= b['y'] * (1.0 + b['kappa'] * 0.25)
    assert _y_error(r2, h2, ref) <= 2.0 * b['y'] and np.all(np.isfinite(r2))
    np.testing.assert_array_equal(r2[:, [5, 7]], rows[:, [5, 7]])


@pytest.mark.parametrize('prec', PRECS)
def test_iteration_cap_gives_status_one_and_finite_rows(ctx, prec):
    s = F.scene()
    rows, head, resid = _fit(ctx, s, max_iter=1, return_residual=True)
    assert head[7] == 1 and head[4] == 1 and 1e-10 < head[5] < 10.0
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(head))
    full = _base(ctx, prec)[0]
    np.testing.assert_array_equal(rows[:, [5, 6, 7]], full[:, [5, 6, 7]])          # who is fitted does not depend on it
    acc = rows[:, 7] == 0
    assert np.all(rows[acc, 1] > 0) and head[2] > _base(ctx, prec)[1][2]
    # the values are the last iterate, and the residual frame is theirs
    want = ctx.render_stars(s['psf'], s['origin'][acc], rows[acc, 0], shift=s['shift'][acc], psf_index=s['index'][acc],
                            image=s['image'], subtract=True)
    assert _same(resid, want)
    # a few steps more: the residual the head reports falls
    h5 = _fit(ctx, s, max_iter=5)[1]
    assert h5[7] == 1 and h5[4] == 5 and h5[5] < head[5]


@pytest.mark.parametrize('prec', PRECS)
def test_permuted_stars_agree_to_rounding(ctx, prec):
    s = F.scene()
    ref = F.scene_reference(True, True, 8.0)
    b = F.bounds(ref, TOL, MAX_ITER)
    perm = np.random.default_rng(8).permutation(s['n'])
    t = dict(s, origin=s['origin'][perm], shift=s['shift'][perm], index=s['index'][perm])
    rows, head = _fit(ctx, t)
    back = np.empty_like(rows)
    back[perm] = rows
    _check_against(back, head, ref, b)
    base = _base(ctx, prec)[0]
    np.testing.assert_array_equal(back[:, [5, 7]], base[:, [5, 7]])       # (the other bits may differ: sums reorder)


# ---- 5. the smallest shapes
@pytest.mark.parametrize('prec', PRECS)
def test_one_pixel_frame(ctx, prec):
    # one pixel cannot carry an unknown and a degree of freedom: nothing fitted, the residual is the image
    psf = F.Y.models()[:1]
    image = np.array([[3.5]])
    for background in (True, False):
        rows, head, resid = ctx.fit_frame_psf(image, psf, [[-20, -20]], background=background, return_residual=True)
        assert list(rows[0]) == [0, 0, 0, 0, 0, 0, 0, 2] and list(head) == [0, 0, 0, 1, 0, 0, 1, 2]
        assert _same(resid, image)
    ref = F.solve(image, None, psf, None, np.array([[-20, -20]]), None, 8.0, False)
    assert ref['head_status'] == 2 and ref['nomega'] == 1
    # two pixels carry one star
    image = np.array([[3.5, 2.5]])
    rows, head = ctx.fit_frame_psf(image, psf, [[-20, -20]], background=False, radius=1.0)
    ref = F.solve(image, None, psf, None, np.array([[-20, -20]]), None, 1.0, False)
    assert head[7] == 0 and head[3] == 2 == ref['nomega'] and head[4] == 1
    _check_against(rows, head, ref, F.bounds(ref, TOL, MAX_ITER))


@pytest.mark.parametrize('prec', PRECS)
def test_one_star(ctx, prec):
    rng = np.random.default_rng(3)
    psf = F.Y.models()
    origin, shift, index = np.array([[7, 11]], dtype=np.int32), np.array([[0.3, -0.45]]), np.array([2], dtype=np.int32)
    model, _, _ = F.Y.render(None, psf, index, origin, shift, [800.0], shape=(64, 70))
    image = model + 3.0 + rng.normal(size=(64, 70))
    for background in (True, False):
        ref = F.solve(image, None, psf, index, origin, shift, 6.0, background)
        rows, head = ctx.fit_frame_psf(image, psf, origin, shift=shift, psf_index=index, radius=6.0,
                                       background=background)
        assert head[4] <= 2 + (1 if background else 0)           # conjugate gradients end in as many steps as unknowns
        _check_against(rows, head, ref, F.bounds(ref, TOL, MAX_ITER))
        assert ref['overlap'][0] == 0.0 and abs(rows[0, 4]) < 1e-11         # alone: no overlap


@pytest.mark.parametrize('prec', PRECS)
def test_star_across_a_tile_corner(ctx, prec):
    rng = np.random.default_rng(4)
    psf = F.Y.models()
    shape = (33, 31)
    # the disc of the first star covers the corner (32, 32) of the tile grid's first tile ... as far as the frame goes
    pos = np.array([[31.6, 29.8], [12.3, 8.9], [30.2, 3.1]])
    origin = (np.rint(pos) - NS // 2).astype(np.int32)
    shift = pos - (origin + NS // 2)
    index = np.array([0, 1, 3], dtype=np.int32)
    model, _, _ = F.Y.render(None, psf, index, origin, shift, [900.0, 400.0, 1500.0], shape=shape)
    var = 1.0 + model / 4.0
    image = model + 2.0 + rng.normal(size=shape) * np.sqrt(var)
    image[rng.uniform(size=shape) < 0.02] = np.nan
    ref = F.solve(image, var, psf, index, origin, shift, 8.0, True)
    rows, head, resid = ctx.fit_frame_psf(image, psf, origin, var=var, shift=shift, psf_index=index,
                                          return_residual=True)
    _check_against(rows, head, ref, F.bounds(ref, TOL, MAX_ITER))
    assert ref['nomega'] < 33 * 31 and np.array_equal(np.isnan(resid), np.isnan(image))


def lattice():
    """289 stars on a jittered 17 x 17 lattice of 11 px pitch in a 200 x 200 frame."""
    rng = np.random.default_rng(6)
    g = 12.0 + 11.0 * np.arange(17)
    pos = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2) + rng.uniform(-1.5, 1.5, (289, 2))
    flux = rng.uniform(300.0, 3000.0, 289)
    origin = (np.rint(pos) - NS // 2).astype(np.int32)
    shift = pos - (origin + NS // 2)
    index = (np.arange(289) % 4).astype(np.int32)
    psf = F.Y.models()
    model, _, _ = F.Y.render(None, psf, index, origin, shift, flux, shape=(200, 200))
    var = 4.0 + model / 2.0
    image = model + F.SKY + rng.normal(size=(200, 200)) * np.sqrt(var)
    return dict(image=image, var=var, psf=psf, index=index, origin=origin, shift=shift, flux=flux, n=289)


_LATTICE = {}


def _lattice_reference():
    if not _LATTICE:
        s = lattice()
        _LATTICE['s'] = s
        _LATTICE['ref'] = F.solve(s['image'], s['var'], s['psf'], s['index'], s['origin'], s['shift'], 5.0, True)
    return _LATTICE['s'], _LATTICE['ref']


@pytest.mark.parametrize('prec', PRECS)
def test_more_stars_than_a_workgroup(ctx, prec):
    s, ref = _lattice_reference()
    assert s['n'] == 289 and s['n'] % 64 and s['n'] % 256 and ref['nacc'] == 289
    b = F.bounds(ref, TOL, MAX_ITER)
    rows, head = _fit(ctx, s, radius=5.0, max_iter=MAX_ITER, tol=TOL)
    _check_against(rows, head, ref, b, 'lattice_%s' % prec)
    z = (rows[:, 0] - s['flux']) / ref['sigma']
    assert np.abs(z).max() < 5.0


@pytest.mark.parametrize('prec', PRECS)
def test_two_stars_at_one_position(ctx, prec):
    rng = np.random.default_rng(9)
    psf = F.Y.models()
    origin, shift = np.array([[10, 14], [30, 50]], dtype=np.int32), np.array([[0.2, 0.4], [-0.3, 0.1]])
    index = np.array([1, 0], dtype=np.int32)
    model, _, _ = F.Y.render(None, psf, index, origin, shift, [1000.0, 700.0], shape=(80, 100))
    image = model + rng.normal(size=(80, 100))
    ref = F.solve(image, None, psf, index, origin, shift, 8.0, False)
    b = F.bounds(ref, TOL, MAX_ITER)
    one, h1 = ctx.fit_frame_psf(image, psf, origin, shift=shift, psf_index=index, background=False)
    _check_against(one, h1, ref, b)
    # the first star twice: N is singular, the sum is determined
    o2, s2, i2 = origin[[0, 1, 0]], shift[[0, 1, 0]], index[[0, 1, 0]]
    two, h2 = ctx.fit_frame_psf(image, psf, o2, shift=s2, psf_index=i2, background=False)
    assert h2[7] in (0, 1) and h2[6] == 3 and np.all(np.isfinite(two)) and np.all(two[:, 7] == 0)
    y_one = np.array([one[0, 0], one[1, 0]]) * np.sqrt(ref['dg'])
    y_two = np.array([two[0, 0] + two[2, 0], two[1, 0]]) * np.sqrt(ref['dg'])
    assert np.linalg.norm(y_two - y_one) <= 2.0 * b['y']
    assert _same(two[0, 6], one[0, 6]) and _same(two[2, 6], one[0, 6]) and abs(two[0, 4] - 1.0 - one[0, 4]) < 1e-9


# ---- 6. the chain
@pytest.mark.parametrize('prec', PRECS)
def test_find_fit_crowded_subtract_find(api, ctx, prec, monkeypatch):
    monkeypatch.setattr(api.psfrec, 'get_context', lambda *a, **k: ctx)
    pos, flux, chain = F.loop_field()
    psf = FR.model()
    n = len(pos)
    index = np.zeros(n, dtype=np.int32)
    frame = ctx.render_stars(psf[None], (np.rint(pos) - NS // 2).astype(np.int32), flux, shift=pos - np.rint(pos),
                             psf_index=index, image=F.loop_background())
    var = np.ones_like(frame)
    ps = 0.2
    found = api.find_stars(frame, psf, var, pixscale=ps, **F.LOOP_FIND)
    assert len(found) == n
    fp = np.asarray(found['position'])
    near = np.argmin(((fp[:, None] - pos[None]) ** 2).sum(-1), axis=1)
    assert sorted(near) == list(range(n))
    member = np.isin(near, chain)
    # the gap: without the frame solve the chain is not fitted
    skip, origin0 = api.fit_found_stars(frame, psf, found, var=var, crit=F.LOOP_CRIT, pixscale=ps)
    assert np.array_equal(np.asarray(skip['crowded']), member) and member.sum() == F.LOOP_CHAIN
    assert np.all(np.isnan(np.asarray(skip['scale'])[member])) and np.all(np.asarray(skip['status'])[member] == 2)
    fit, origin = api.fit_found_stars(frame, psf, found, var=var, crit=F.LOOP_CRIT, pixscale=ps, crowded='frame')
    assert len(fit) == n and origin.shape == (len(origin0) + F.LOOP_CHAIN, 2)
    assert np.array_equal(np.asarray(fit['crowded']), member)
    for name in ('scale', 'flux', 'err_scale', 'err_flux', 'back', 'err_back', 'chi2'):
        assert np.all(np.isfinite(np.asarray(fit[name]))), name
    assert np.all(np.isfinite(np.asarray(fit['shift']))) and np.all((np.asarray(fit['status']) & 3) != 2)
    for name in fit.colnames:
        np.testing.assert_array_equal(np.asarray(fit[name])[~member], np.asarray(skip[name])[~member])
    # the chain's fluxes against the truth, in marginal sigma of the yardstick at the found positions
    rows = np.flatnonzero(member)
    own = (np.rint(fp[rows]) - NS // 2).astype(np.int32)
    sh = fp[rows] - (own + NS // 2)
    ref = F.solve(frame, var, psf[None], np.zeros(len(rows), dtype=int), own, sh, 8.0, True)
    z = (np.asarray(fit['flux'])[rows] - flux[near[rows]]) / ref['sigma']
    print('chain %s: worst flux error of a chain member %.2f marginal sigma; overlap up to %.2f' %
          (prec, np.abs(z).max(), ref['overlap'].max()))
    assert np.all(np.abs(z) <= 4.0)
    where = origin[np.asarray(fit['group'])] + NS // 2 + np.asarray(fit['shift']) / ps
    assert np.abs(where - pos[near]).max() < 0.5
    residual, status = api.subtract_stars(frame, psf[None], origin, fit, psf_index=np.zeros(len(origin), dtype=np.int32),
                                          pixscale=ps)
    assert np.all(status == 0)
    again = api.find_stars(residual, psf, var, pixscale=ps, **F.LOOP_FIND)
    if len(again):
        d = np.sqrt(((np.asarray(again['position'])[:, None] - pos[chain][None]) ** 2).sum(-1))
        assert d.min() > 3.0
    # with crowded='skip' the chain stays in the residual frame: the finder sees it again
    left, _ = api.subtract_stars(frame, psf[None], origin0, skip, psf_index=np.zeros(len(origin0), dtype=np.int32),
                                 pixscale=ps)
    seen = api.find_stars(left, psf, var, pixscale=ps, **F.LOOP_FIND)
    assert len(seen) >= F.LOOP_CHAIN - 1
    # fit_crowded_stars on the whole frame, from the finder's table
    allfit, og, res = api.fit_crowded_stars(frame, psf, found, var=var, start='found', return_residual=True, pixscale=ps)
    assert np.all(np.asarray(allfit['status']) == 0) and allfit.meta['status'] == 0 and allfit.meta['iterations'] > 2
    assert abs(allfit.meta['back'] - 5.0) < 0.1 and len(api.find_stars(res, psf, var, pixscale=ps, **F.LOOP_FIND)) == 0


# ---- 7. refusals
def _raw(ctx, s, **override):
    """The C call on host pointers with sentinel outputs; returns (rc, rows, head, resid)."""
    n = s['n']
    ny, nx = s['image'].shape
    a = dict(ny=ny, nx=nx, image=s['image'], var=s['var'], nstar=n, npsf=len(s['psf']), psf=s['psf'], index=s['index'],
             origin=s['origin'], shift=s['shift'], scale0=None, radius=8.0, flags=1, max_iter=100, tol=1e-10,
             rows=np.full((n, 8), -7.0), head=np.full(8, -7.0), resid=np.full((ny, nx), -7.0), on_device=0)
    a.update(override)

    def p(v):
        return None if v is None else C.c_void_p(np.ascontiguousarray(v).ctypes.data)
    keep = {k: np.ascontiguousarray(a[k]) if a[k] is not None else None
            for k in ('image', 'var', 'psf', 'index', 'origin', 'shift', 'scale0')}
    rc = ctx.lib.mpsfr_fit_frame_psf(ctx._h, a['ny'], a['nx'], p(keep['image']), p(keep['var']), a['nstar'], a['npsf'],
                                     p(keep['psf']), p(keep['index']), p(keep['origin']), p(keep['shift']),
                                     p(keep['scale0']), float(a['radius']), a['flags'], a['max_iter'], float(a['tol']),
                                     p(a['rows']), p(a['head']), p(a['resid']), a['on_device'])
    return rc, a['rows'], a['head'], a['resid']


def test_bad_arguments_are_refused_and_leave_the_outputs(api):
    ctx = _ctx(api, 'mixed')
    s = F.scene()
    n = s['n']
    far, nan, inf = s['shift'].copy(), s['shift'].copy(), np.zeros(n)
    far[2, 1], nan[5, 0], inf[1] = 8.25, np.nan, np.inf
    bad_index, bad_origin = s['index'].copy(), s['origin'].copy()
    bad_index[4], bad_origin[0, 0] = 4, (1 << 30) + 1
    neg_index = s['index'].copy()
    neg_index[0] = -1
    cases = [dict(ny=0), dict(nx=0), dict(ny=-1), dict(ny=16385), dict(nx=16385), dict(ny=8193, nx=8192),
             dict(nstar=0), dict(nstar=-1), dict(nstar=(1 << 20) + 1), dict(npsf=0), dict(npsf=-1),
             dict(image=None), dict(psf=None), dict(origin=None), dict(rows=None), dict(head=None),
             dict(index=None),                                                    # npsf = 4 != nstar
             dict(radius=0.999), dict(radius=20.001), dict(radius=np.nan), dict(radius=np.inf), dict(radius=-8.0),
             dict(tol=0.0), dict(tol=1.0), dict(tol=-1e-10), dict(tol=np.nan), dict(tol=np.inf),
             dict(max_iter=0), dict(max_iter=-1), dict(max_iter=1001),
             dict(flags=2), dict(flags=4), dict(flags=3), dict(flags=-1),
             dict(index=bad_index), dict(index=neg_index), dict(shift=far), dict(shift=nan), dict(origin=bad_origin),
             dict(scale0=inf), dict(scale0=np.full(n, np.nan))]
    for kw in cases:
        rc, rows, head, resid = _raw(ctx, s, **kw)
        assert rc == -1, kw
        assert b'fit_frame_psf' in ctx.lib.mpsfr_last_error(), kw
        assert all(np.all(out == -7.0) for out in (rows, head, resid) if out is not None), kw
    # their neighbours are legal, and var, shift, scale0 and resid_out are optional
    for kw in (dict(radius=1.0), dict(radius=20.0), dict(tol=0.999), dict(tol=1e-300, max_iter=2), dict(max_iter=1),
               dict(flags=0), dict(var=None), dict(shift=None), dict(scale0=np.zeros(n)), dict(resid=None)):
        rc, rows, head, resid = _raw(ctx, s, **kw)
        assert rc == 0 and head[6] >= 1 and head[7] != -7.0 and np.all(rows[:, 7] != -7.0), kw


# ---- 8. housekeeping
def test_timed_under_the_profiling_id_of_the_fit(api):
    ctx = api.Context(dim=128, pixscale=api.grid_pixscale(128), precision='mixed')
    assert ctx.lib.mpsfr_profile_count() == 16 and ctx.lib.mpsfr_version() == 102
    ctx.set_option('profile', 1)
    ctx.profile_reset()
    rows, head = _fit(ctx, F.scene())
    prof = ctx.profile()
    assert head[7] == 0 and prof['fit'][1] == 1 and prof['fit'][0] > 0
    assert all(v[1] == 0 for k, v in prof.items() if k != 'fit'), prof
    ctx.close()
