"""GPU: the crowded-field fit with free positions (mpsfr_fit_frame_psf_free; frame_free.hip).

1. parity with the converged yardstick (frame_free_ref) on the noiseless displaced scene -- var on / off x background on /
   off x radius 4 and 8, both precisions: every free star's final shift within pos_tol rho / (1 - rho) plus the inner
   term derived there, pos_tol ten times the largest inner term, the outer step count the yardstick's; columns 0 - 7
   and the head against the dense solve at the returned shifts within section 24's bounds; the position errors from
   the yardstick's blocks.  One Gauss-Newton step on the noisy scene against the same rule with exact solves.  Worst
   error / bound ratios go to record_margin('frame_free', ...).
2. the residual frame is render_stars(subtract) of shift_out and column 0, bit for bit, also at max_outer = 0 and
   max_iter = 1.
3. bits: the same call twice, mixed = f64, host = device pointers; permuted stars agree to rounding; both power-of-two
   laws with the positions bit for bit.
4. max_outer = 0 is section 24's solve at the start.
5. edges: a shift that crosses an integer, max_move, the +-8 bound, max_step, min_snr, nobody free, two stars at one
   position, stars left out, 1 x 2 and 33 x 31 frames, 289 stars on 80 x 80.
6. refusals: every MPSFR_E_INVALID of the header, outputs untouched.
7. the chain find -> fit_found_stars(crowded='free') -> subtract_stars -> find.
"""
import ctypes as C

import numpy as np
import pytest

import find_ref as FR
import frame_fit_ref as F
import frame_free_ref as G
from conftest import record_margin

pytestmark = pytest.mark.gpu

PRECS = ['mixed', 'f64']
NS = 40
TOL, MAX_ITER = 1e-12, 100
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


def _free(ctx, s, with_var=True, background=True, radius=8.0, **kw):
    return ctx.fit_frame_psf_free(s['image'], s['psf'], s['origin'], var=s['var'] if with_var else None,
                                  shift=s['shift'], psf_index=s['index'], radius=radius, background=background, **kw)


def _render_of(ctx, s, rows, shifts):
    acc = np.flatnonzero(rows[:, 7] == 0)
    return ctx.render_stars(s['psf'], s['origin'][acc], rows[acc, 0], shift=shifts[acc], psf_index=s['index'][acc],
                            image=s['image'], subtract=True)


_BASE = {}


def _base(ctx, prec):
    """The call on the noisy displaced scene at its defaults, with its residual, once per precision."""
    if prec not in _BASE:
        _BASE[prec] = _free(ctx, G.displaced_scene(True), return_residual=True)
    return _BASE[prec]


# ---- 1. parity
_HELD = {}
_RULE = {}


def _held_reference(conv, shifts, ever):
    key = (id(conv), shifts.tobytes(), ever)
    if key not in _HELD:
        _HELD[key] = conv['problem'].held(shifts, ever)
    return _HELD[key]


def _check_closing(rows, head, ref, b, acc):
    """Columns 0 - 7 and the head's first eight against the dense solve at the returned shifts (section 24's checks)."""
    nacc = len(acc)
    assert 0 <= head[4] <= MAX_ITER and 0 <= head[5] <= TOL
    x = np.concatenate([rows[acc, 0], [head[0]]]) if ref['background'] else rows[acc, 0]
    ratios = dict(y=float(np.linalg.norm((x - ref['x']) * np.sqrt(ref['dg']))) / b['y'])
    assert np.all(np.abs(rows[acc, 0] - ref['F']) <= b['y'] / np.sqrt(ref['nkk']))
    ratios['nkk'] = float(np.max(np.abs(rows[acc, 6] - ref['nkk']) / ref['nkk'])) / b['nkk_rel']
    ratios['overlap'] = float(np.max(np.abs(rows[acc, 4] - ref['overlap']) / b['overlap']))
    ratios['chi2'] = abs(head[2] - ref['chi2']) / b['chi2']
    np.testing.assert_allclose(rows[acc, 1], np.sqrt(head[2] / ref['dof'] / rows[acc, 6]), rtol=4 * EPS)
    if ref['background']:
        assert abs(head[1] - np.sqrt(head[2] / ref['dof'] / ref['dg'][nacc])) <= (b['nkk_rel'] + 8 * EPS) * head[1]
    else:
        assert head[0] == 0 and head[1] == 0
    return ratios


@pytest.mark.parametrize('radius', [4.0, 8.0])
@pytest.mark.parametrize('background', [True, False])
@pytest.mark.parametrize('with_var', [True, False])
@pytest.mark.parametrize('prec', PRECS)
def test_parity_with_the_converged_yardstick(ctx, prec, with_var, background, radius):
    s = G.displaced_scene(False)
    conv = G.scene_converged(with_var, background, radius, False, max_outer=10)
    pr, acc, fi = conv['problem'], conv['problem'].acc, conv['last']['free_idx']
    assert conv['rho'] < 0.5 and len(fi) == len(acc)
    # pos_tol: ten times the largest inner term and more, so that the inner solves decide no stop test (frame_free_ref)
    pos_tol = G.parity_pos_tol(conv, TOL, MAX_ITER)
    bound, _ = G.position_bounds(conv, pos_tol, TOL, MAX_ITER)
    steps = np.array(conv['steps'])
    assert not np.any(np.abs(steps - pos_tol) <= 0.1 * pos_tol)
    nouter = int(np.argmax(steps <= pos_tol)) + 1
    rows, shifts, head = _free(ctx, s, with_var, background, radius, max_iter=MAX_ITER, tol=TOL, max_outer=10,
                               pos_tol=pos_tol)
    assert rows.shape == (s['n'], 16) and shifts.shape == (s['n'], 2) and head.shape == (12,)
    tag = '%s_%s_%s_r%d' % (prec, 'var' if with_var else 'unit', 'back' if background else 'noback', int(radius))
    # who is fitted, the counts, the stop: exact
    np.testing.assert_array_equal(rows[:, 7], conv['status'])
    np.testing.assert_array_equal(rows[:, 5], pr.base['ndisc'])
    assert (head[3], head[6], head[7], head[8], head[10]) == (pr.nomega, pr.nacc, 0, nouter, len(acc))
    # (no solve runs into max_iter: test_frame_free_host.py counts the steps the tolerance asks for on these systems)
    assert head[9] <= pos_tol
    key = (with_var, background, radius)
    if key not in _RULE:
        _RULE[key] = G.refine(s['image'], s['var'] if with_var else None, s['psf'], s['index'], s['origin'], s['shift'],
                              radius, background, max_outer=10, pos_tol=pos_tol)
    rule = _RULE[key]
    assert rule['nouter'] == nouter and rule['posok']
    np.testing.assert_array_equal(rows[acc, 15], rule['nfree'][acc])
    np.testing.assert_array_equal(rows[acc, 14], rule['flags'][acc])
    # a star left out echoes its shift and is zero elsewhere
    out = np.setdiff1d(np.arange(s['n']), acc)
    assert len(out) >= 2 and _same(shifts[out], s['shift'][out]) and _same(rows[out, 8:10], s['shift'][out])
    assert not rows[out, :7].any() and not rows[out, 10:].any()
    assert _same(rows[:, 8:10], shifts) and _same(rows[acc, 12:14], shifts[acc] - s['shift'][acc])
    # the positions against the minimiser
    err = np.abs(shifts[acc][fi] - conv['shift'][acc][fi])
    ratios = dict(position=float(np.max(err / bound)))
    # the closing solve against the dense solve at the returned shifts
    ref = _held_reference(conv, shifts, int(np.sum(rule['nfree'] > 0)))
    ratios.update(_check_closing(rows, head, ref, F.bounds(ref, TOL, MAX_ITER), acc))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
    print('frame free %s: error / bound %s; pos_tol %.2e, %d outer steps, %d inner iterations' %
          (tag, ', '.join('%s %.2e' % kv for kv in sorted(ratios.items())), pos_tol, head[8], head[11]))
    record_margin('frame_free', **{'%s_%s' % (k, tag): v for k, v in ratios.items()})


@pytest.mark.parametrize('prec', PRECS)
def test_one_step_on_the_noisy_scene_follows_the_rule(ctx, prec):
    # (with noise the trio within 2 px does not contract: one step is compared, the residual not zero, some stars held)
    s = G.displaced_scene(True)
    rows, shifts, head = _free(ctx, s, max_iter=MAX_ITER, tol=TOL, max_outer=1)
    ref = check_one_step(s, rows, shifts, head)
    record_margin('frame_free', **{'one_step_%s' % prec: ref['ratio']})


_ONE_STEP = {}


def check_one_step(s, rows, shifts, head, **kw):
    """The outputs of a call with max_iter = MAX_ITER, tol = TOL, max_outer = 1 and the step parameters `kw` on the scene
    `s` = G.displaced_scene(True) (var, background, radius 8) against one step of the rule with exact solves.  Returns the yardstick's run with
    the worst position error / bound under 'ratio'."""
    assert s is G.displaced_scene(True)          # (the yardstick is kept per step parameters, of this scene alone)
    key = tuple(sorted(kw.items()))
    if key not in _ONE_STEP:
        _ONE_STEP[key] = G.refine(s['image'], s['var'], s['psf'], s['index'], s['origin'], s['shift'], 8.0, True,
                                  max_outer=1, **kw)
    ref = _ONE_STEP[key]
    acc, fi = ref['problem'].acc, ref['last']['free_idx']
    _, by, bx = G.inner_bounds(ref['last'], TOL, MAX_ITER)
    err = np.abs(shifts[acc][fi] - ref['shift'][acc][fi])
    ratio = float(np.max(err / np.stack([by, bx], axis=1)))
    assert ratio <= 1.0
    np.testing.assert_array_equal(rows[acc, 14], ref['flags'][acc])
    np.testing.assert_array_equal(rows[acc, 15], ref['nfree'][acc])
    assert (head[8], head[10]) == (1, ref['nfree_last']) and head[7] == (0 if ref['steps'][0] <= 1e-3 else 1)
    assert abs(head[9] - ref['steps'][0]) <= float(max(by.max(), bx.max()))
    assert 0 < ref['nfree_last'] < len(acc) and (ref['flags'][acc] & G.HELD).any()
    held = acc[ref['nfree'][acc] == 0]
    assert _same(shifts[held], s['shift'][held]) and not rows[held, 10:14].any()
    # the position errors: the yardstick's blocks, its chi2 / dof and F
    free = acc[fi]
    np.testing.assert_allclose(rows[free, 10:12], ref['err_shift'][free], rtol=1e-6)
    return dict(ref, ratio=ratio)


# ---- 2. the residual frame is the renderer's
@pytest.mark.parametrize('prec', PRECS)
def test_residual_equals_render_subtract_bit_for_bit(ctx, prec):
    s = G.displaced_scene(True)
    rows, shifts, head, resid = _base(ctx, prec)
    assert set(rows[:, 7]) == {0.0, 1.0, 2.0} and head[8] >= 1 and np.abs(shifts - s['shift']).max() > 0.05
    assert _same(resid, _render_of(ctx, s, rows, shifts))
    assert np.array_equal(np.isnan(resid), np.isnan(s['image']))
    for kw in (dict(max_outer=0), dict(max_iter=1), dict(max_outer=2, max_iter=3)):
        r, sh, h, d = _free(ctx, s, return_residual=True, **kw)
        assert _same(d, _render_of(ctx, s, r, sh)) and np.all(np.isfinite(r)) and np.all(np.isfinite(h)), kw
        assert h[7] == (1 if 'max_iter' in kw else 0), kw
    # without the residual frame the rows are the same bits
    r2, s2, h2 = _free(ctx, s)
    assert _same(r2, rows) and _same(s2, shifts) and _same(h2, head)


# ---- 3. bits
@pytest.mark.parametrize('prec', PRECS)
def test_same_call_twice_gives_the_same_bits(ctx, prec):
    a = _base(ctx, prec)
    b = _free(ctx, G.displaced_scene(True), return_residual=True)
    assert all(_same(x, y) for x, y in zip(a, b))


def test_mixed_gives_the_bits_of_f64(api):
    a, b = _base(_ctx(api, 'mixed'), 'mixed'), _base(_ctx(api, 'f64'), 'f64')
    assert all(_same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('prec', PRECS)
def test_device_pointers_give_the_bits_of_the_host_form(ctx, prec):
    import torch
    s = G.displaced_scene(True)
    ny, nx = F.FRAME
    n = s['n']
    dev = torch.device('cuda:0')
    t = {k: torch.from_numpy(np.ascontiguousarray(s[k])).to(dev) for k in ('image', 'var', 'psf', 'index', 'origin', 'shift')}
    trow = torch.full((n, 16), -1.0, dtype=torch.float64, device=dev)
    tsh = torch.full((n, 2), -1.0, dtype=torch.float64, device=dev)
    thead = torch.full((12,), -1.0, dtype=torch.float64, device=dev)
    tres = torch.full((ny, nx), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_frame_psf_free_device(ny, nx, t['image'].data_ptr(), n, 4, t['psf'].data_ptr(), t['origin'].data_ptr(),
                                  trow.data_ptr(), tsh.data_ptr(), thead.data_ptr(), var_ptr=t['var'].data_ptr(),
                                  shift_ptr=t['shift'].data_ptr(), psf_index_ptr=t['index'].data_ptr(),
                                  resid_ptr=tres.data_ptr())
    ctx.sync()
    got = (trow.cpu().numpy(), tsh.cpu().numpy(), thead.cpu().numpy(), tres.cpu().numpy())
    assert all(_same(x, y) for x, y in zip(got, _base(ctx, prec)))
    # shift_out is what the renderer and the flux-only fit read: a device chain without repacking
    trow8 = torch.full((n, 8), -1.0, dtype=torch.float64, device=dev)
    thead8 = torch.full((8,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_frame_psf_device(ny, nx, t['image'].data_ptr(), n, 4, t['psf'].data_ptr(), t['origin'].data_ptr(),
                             trow8.data_ptr(), thead8.data_ptr(), var_ptr=t['var'].data_ptr(), shift_ptr=tsh.data_ptr(),
                             psf_index_ptr=t['index'].data_ptr())
    ctx.sync()
    r8 = trow8.cpu().numpy()
    fitted = got[0][:, 7] == 0
    # (the flux-only solve draws its discs around the refined centres, the free one around the start: another Omega,
    # the same stars, fluxes that agree within the noise -- one conditional error)
    assert np.array_equal(r8[:, 7], got[0][:, 7])
    assert np.all(np.abs(r8[fitted, 0] - got[0][fitted, 0]) <= got[0][fitted, 1])
    # in the device form a star outside the domain is left out and echoes its shift
    bad = s['shift'].copy()
    bad[3, 0] = np.nan
    tbad = torch.from_numpy(bad).to(dev)
    trow.fill_(-1.0)
    torch.cuda.synchronize()
    ctx.fit_frame_psf_free_device(ny, nx, t['image'].data_ptr(), n, 4, t['psf'].data_ptr(), t['origin'].data_ptr(),
                                  trow.data_ptr(), tsh.data_ptr(), thead.data_ptr(), var_ptr=t['var'].data_ptr(),
                                  shift_ptr=tbad.data_ptr(), psf_index_ptr=t['index'].data_ptr())
    ctx.sync()
    r, sh = trow.cpu().numpy(), tsh.cpu().numpy()
    assert r[3, 7] == 2 and not r[3, :7].any() and not r[3, 10:].any() and np.isnan(sh[3, 0]) and sh[3, 1] == bad[3, 1]


@pytest.mark.parametrize('prec', PRECS)
def test_permuted_stars_agree_to_rounding(ctx, prec):
    # (on the noiseless scene, where the iteration contracts: the sums reorder, the minimiser is the same)
    s = G.displaced_scene(False)
    conv = G.scene_converged(True, True, 8.0, False, max_outer=10)
    acc = conv['problem'].acc
    pos_tol = G.parity_pos_tol(conv, TOL, MAX_ITER)
    bound, _ = G.position_bounds(conv, pos_tol, TOL, MAX_ITER)
    perm = np.random.default_rng(8).permutation(s['n'])
    t = dict(s, origin=s['origin'][perm], shift=s['shift'][perm], index=s['index'][perm])
    kw = dict(max_iter=MAX_ITER, tol=TOL, max_outer=10, pos_tol=pos_tol)
    rows, shifts, head = _free(ctx, t, **kw)
    r0, s0, h0 = _free(ctx, s, **kw)
    back, sback = np.empty_like(rows), np.empty_like(shifts)
    back[perm], sback[perm] = rows, shifts
    np.testing.assert_array_equal(back[:, [5, 7, 14, 15]], r0[:, [5, 7, 14, 15]])
    assert h0[8] == head[8] and np.all(np.abs(sback[acc] - s0[acc]) <= 2.0 * bound)
    np.testing.assert_allclose(back[acc, 0], r0[acc, 0], rtol=1e-6)


@pytest.mark.parametrize('prec', PRECS)
def test_power_of_two_scaling_laws_hold_bit_for_bit(ctx, prec):
    s = G.displaced_scene(True)
    rows, shifts, head, resid = _base(ctx, prec)
    start = np.where(rows[:, 7] == 0, rows[:, 0] * 0.75, 0.0)
    r0, s0, h0, d0 = _free(ctx, s, scale0=start, return_residual=True)
    assert h0[8] >= 1
    # a power of two on var: chi2 and N_kk scale with 1 / var, nothing else moves
    r1, s1, h1, d1 = _free(ctx, dict(s, var=s['var'] * 16.0), return_residual=True)
    for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15):
        assert _same(r1[:, k], rows[:, k]), k
    assert _same(r1[:, 6] * 16.0, rows[:, 6]) and _same(s1, shifts) and _same(d1, resid)
    assert _same(h1[[0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11]], head[[0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11]])
    assert h1[2] * 16.0 == head[2]
    # 2^k on the data (and the start) with 4^k on var: F, b, the fluxes and their errors scale by 2^k
    for k in (3, -5):
        f = 2.0 ** k
        t = dict(s, image=s['image'] * f, var=s['var'] * f * f)
        r2, s2, h2, d2 = _free(ctx, t, scale0=start * f, return_residual=True)
        assert _same(r2[:, :4], r0[:, :4] * f) and _same(r2[:, [4, 5, 7]], r0[:, [4, 5, 7]])
        assert _same(r2[:, 6] * f * f, r0[:, 6]) and _same(r2[:, 8:], r0[:, 8:]) and _same(s2, s0)
        assert _same(h2[:2], h0[:2] * f) and _same(h2[2:], h0[2:]) and _same(d2, d0 * f)


# ---- 4. max_outer = 0
@pytest.mark.parametrize('background', [True, False])
@pytest.mark.parametrize('prec', PRECS)
def test_no_outer_step_is_the_solve_at_the_start(ctx, prec, background):
    s = G.displaced_scene(True)
    rows, shifts, head = _free(ctx, s, background=background, max_outer=0, max_iter=100, tol=1e-10)
    check_no_outer_step(s, rows, shifts, head, background)


_START = {}


def check_no_outer_step(s, rows, shifts, head, background):
    """The outputs of a call with max_outer = 0, max_iter = 100 and tol = 1e-10 on G.displaced_scene(True) (var, radius
    8) against frame_fit_ref.solve at the start shifts, within frame_fit_ref.bounds."""
    assert s is G.displaced_scene(True)
    if background not in _START:
        _START[background] = F.solve(s['image'], s['var'], s['psf'], s['index'], s['origin'], s['shift'], 8.0, background)
    ref = _START[background]
    b = F.bounds(ref, 1e-10, 100)
    acc = ref['acc']
    np.testing.assert_array_equal(rows[:, 7], ref['status'])
    np.testing.assert_array_equal(rows[:, 5], ref['ndisc'])
    assert (head[3], head[6], head[7]) == (ref['nomega'], ref['nacc'], 0) and 1 <= head[4] <= 100 and head[5] <= 1e-10
    x = np.concatenate([rows[acc, 0], [head[0]]]) if background else rows[acc, 0]
    assert float(np.linalg.norm((x - ref['x']) * np.sqrt(ref['dg']))) <= b['y']
    assert np.max(np.abs(rows[acc, 6] - ref['nkk'][acc]) / ref['nkk'][acc]) <= b['nkk_rel']
    assert np.all(np.abs(rows[acc, 4] - ref['overlap'][acc]) <= b['overlap']) and abs(head[2] - ref['chi2']) <= b['chi2']
    rel = b['chi2'] / ref['chi2'] + b['nkk_rel'] + 8 * EPS
    np.testing.assert_allclose(rows[acc, 1], ref['err'][acc], rtol=rel)
    # the positions stay, nothing was free, the head says so
    assert _same(shifts, s['shift']) and _same(rows[:, 8:10], s['shift']) and not rows[:, 10:].any()
    assert list(head[8:11]) == [0, 0, 0] and head[11] == head[4]


# ---- 5. edges
def _field(shape, pos, flux, index, seed=None, sky=0.0, sigma=1.0):
    """A rendered field: (dict of the call's arrays at the true positions, truth shifts)."""
    psf = F.Y.models()
    pos = np.asarray(pos, dtype=float)
    origin = (np.rint(pos) - NS // 2).astype(np.int32)
    shift = pos - (origin + NS // 2)
    index = np.asarray(index, dtype=np.int32)
    image, _, _ = F.Y.render(None, psf, index, origin, shift, flux, shape=shape)
    if seed is not None:
        image = image + sky + sigma * np.random.default_rng(seed).normal(size=shape)
    return dict(image=image, var=None, psf=psf, index=index, origin=origin, shift=shift.copy(), n=len(pos)), shift


TIGHT = dict(max_iter=200, tol=1e-12, max_outer=12, pos_tol=1e-9, background=False)
# (noiseless fields of well separated stars: the minimiser is the truth, Gauss-Newton converges quadratically (rho far
# below 1/2: the step after one below 1e-9 px is below rounding), the inner term kappa tol |y*| / (F sqrt(N_aa)) with
# kappa of a few and tol 1e-12 is below 1e-10 px: 1e-8 px bounds the sum with a margin of ten over both.)
EXACT = 1e-8


@pytest.mark.parametrize('prec', PRECS)
def test_a_shift_that_crosses_an_integer(ctx, prec):
    # the truth at shift 1.1 from a start at 0.9: floor(-shift) changes, the stage windows of both kernels move
    psf = F.Y.models()
    origin, index, truth = np.array([[0, 0]], dtype=np.int32), np.array([1], dtype=np.int32), np.array([[1.1, 0.3]])
    image, _, _ = F.Y.render(None, psf, index, origin, truth, [1000.0], shape=(40, 40))
    s = dict(image=image, var=None, psf=psf, index=index, origin=origin, shift=np.array([[0.9, 0.4]]), n=1)
    rows, shifts, head = _free(ctx, s, with_var=False, **TIGHT)
    assert head[7] == 0 and head[8] >= 2 and rows[0, 14] == 0 and rows[0, 15] == head[8]
    assert np.abs(shifts - truth).max() <= EXACT and np.floor(-shifts[0, 0]) != np.floor(-0.9)
    assert abs(rows[0, 0] - 1000.0) <= 1e-6


@pytest.mark.parametrize('prec', PRECS)
def test_the_clips_and_their_flags(ctx, prec):
    s, truth = _field((40, 40), [[12.3, 13.4], [27.6, 25.2]], [1000.0, 800.0], [0, 2])
    start = truth + np.array([[0.3, 0.0], [0.0, 0.0]])
    s['shift'] = start
    # max_move: star 0 comes to rest 0.2 px from its start, on the side of the truth; the loop cannot pass its test
    rows, shifts, head = _free(ctx, s, with_var=False, **dict(TIGHT, max_move=0.2))
    assert shifts[0, 0] == start[0, 0] - 0.2 and int(rows[0, 14]) & G.BOUND and head[7] == 1 and head[8] == 12
    assert head[9] > 0.05 and not int(rows[1, 14]) & G.BOUND and np.abs(shifts[1] - truth[1]).max() < 5e-3
    # max_step: one step of 0.05 px, flagged; the other star's step is not
    rows, shifts, head = _free(ctx, s, with_var=False, **dict(TIGHT, max_step=0.05, max_outer=1))
    assert shifts[0, 0] == start[0, 0] - 0.05 and int(rows[0, 14]) == G.CLIPPED and rows[1, 14] == 0
    assert (head[7], head[8]) == (1, 1) and 0.2 < head[9] < 0.4
    # the +-8 bound: the truth lies at shift 8.3 of this origin, the start at 7.9
    far, _ = _field((60, 60), [[38.3, 30.0]], [1000.0], [1])
    far['origin'] = np.array([[10, 10]], dtype=np.int32)
    far['shift'] = np.array([[7.9, 0.0]])
    rows, shifts, head = _free(ctx, far, with_var=False, **dict(TIGHT, max_move=4.0))
    assert shifts[0, 0] == 8.0 and int(rows[0, 14]) & G.BOUND and head[7] == 1 and abs(shifts[0, 1]) < 0.05


@pytest.mark.parametrize('prec', PRECS)
def test_min_snr_holds_a_faint_star_and_can_hold_all(ctx, prec):
    s, truth = _field((40, 40), [[12.3, 13.4], [27.6, 25.2], [14.0, 30.0]], [1e5, 8e4, 10.0], [0, 2, 1], seed=5)
    s['shift'] = truth + 0.2
    rows, shifts, head = _free(ctx, s, with_var=False, min_snr=50.0, max_outer=6)
    assert _same(shifts[2], s['shift'][2]) and int(rows[2, 14]) == G.HELD and rows[2, 15] == 0
    assert not rows[2, 10:14].any() and rows[2, 7] == 0 and np.isfinite(rows[2, 0])
    assert np.all(rows[:2, 15] == head[8]) and np.all(rows[:2, 14] == 0) and head[10] == 2
    assert np.abs(shifts[:2] - truth[:2]).max() < 0.01 and np.all(rows[:2, 10:12] > 0)
    # nobody free: the call ends after the opening solve
    r0, s0, h0 = _free(ctx, s, with_var=False, max_outer=0)
    rows, shifts, head = _free(ctx, s, with_var=False, min_snr=1e12, max_outer=6)
    assert list(head[8:11]) == [0, 0, 0] and head[7] == 0 and _same(shifts, s['shift'])
    assert np.all(rows[:, 14] == G.HELD) and not rows[:, 15].any() and not rows[:, 10:14].any()
    np.testing.assert_allclose(rows[:, :7], r0[:, :7], rtol=1e-8, atol=1e-8)


@pytest.mark.parametrize('prec', PRECS)
def test_two_stars_at_one_position(ctx, prec):
    s, truth = _field((40, 40), [[15.2, 14.4], [26.7, 27.1]], [1000.0, 700.0], [1, 0], seed=9)
    for k in ('origin', 'shift', 'index'):
        s[k] = s[k][[0, 1, 0]]
    s['n'] = 3
    rows, shifts, head, resid = _free(ctx, s, with_var=False, background=False, return_residual=True)
    assert head[7] in (0, 1) and head[6] == 3 and np.all(rows[:, 7] == 0)
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(shifts)) and np.all(np.isfinite(head))
    assert np.all(np.abs(shifts - s['shift']) <= 2.0) and _same(resid, _render_of(ctx, s, rows, shifts))


@pytest.mark.parametrize('prec', PRECS)
def test_the_smallest_frames(ctx, prec):
    # 1 x 2: two pixels carry one flux and no position -- no star is free, the solve is section 24's
    psf = F.Y.models()[:1]
    image = np.array([[3.5, 2.5]])
    rows, shifts, head = ctx.fit_frame_psf_free(image, psf, [[-20, -20]], background=False, radius=1.0)
    want, h = ctx.fit_frame_psf(image, psf, [[-20, -20]], background=False, radius=1.0)
    assert (head[7], head[3], head[8], head[10]) == (0, 2, 0, 0) and rows[0, 14] == G.HELD
    np.testing.assert_allclose(rows[0, :8], want[0], rtol=1e-12, atol=1e-12)
    assert not shifts.any()
    # 33 x 31: a star across the corner of the tile grid's first tile, two more
    pos = np.array([[31.6, 29.8], [12.3, 8.9], [30.2, 3.1]])
    s, truth = _field((33, 31), pos, [900.0, 400.0, 1500.0], [0, 1, 3])
    s['shift'] = truth + np.array([[0.15, -0.2], [-0.1, 0.25], [0.2, 0.1]])
    rows, shifts, head = _free(ctx, s, with_var=False, **TIGHT)
    assert head[7] == 0 and np.all(rows[:, 15] == head[8]) and np.abs(shifts - truth).max() <= 1e-6


@pytest.mark.parametrize('prec', PRECS)
def test_a_tile_list_longer_than_256(ctx, prec, api):
    rng = np.random.default_rng(6)
    g = 4.0 + 4.5 * np.arange(17)
    pos = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2) + rng.uniform(-0.5, 0.5, (289, 2))
    s, truth = _field((80, 80), pos, rng.uniform(300.0, 3000.0, 289), np.full(289, 2), seed=7, sky=5.0)
    assert F.Y.longest_tile_list(s, (80, 80)) > api.RENDER_SORT_CHUNK
    s['shift'] = truth + rng.uniform(-0.05, 0.05, (289, 2))
    ref = G.refine(s['image'], None, s['psf'], s['index'], s['origin'], s['shift'], 4.0, True, max_outer=1, min_snr=0.0)
    rows, shifts, head, resid = _free(ctx, s, with_var=False, radius=4.0, max_outer=1, min_snr=0.0, max_iter=1000,
                                      tol=TOL, return_residual=True)
    fi = ref['last']['free_idx']
    _, by, bx = G.inner_bounds(ref['last'], TOL, 1000)
    err = np.abs(shifts[fi] - ref['shift'][fi])
    assert head[6] == 289 == ref['problem'].nacc and head[8] == 1 and head[10] == len(fi) == ref['nfree_last']
    assert np.all(err <= np.stack([by, bx], axis=1))
    assert _same(resid, _render_of(ctx, s, rows, shifts))
    record_margin('frame_free', **{'pile_%s' % prec: float(np.max(err / np.stack([by, bx], axis=1)))})


# ---- 6. refusals
def _raw(ctx, s, **override):
    """The C call on host pointers with sentinel outputs; returns (rc, rows, shifts, head, resid)."""
    n = s['n']
    ny, nx = s['image'].shape
    a = dict(ny=ny, nx=nx, image=s['image'], var=s['var'], nstar=n, npsf=len(s['psf']), psf=s['psf'], index=s['index'],
             origin=s['origin'], shift=s['shift'], scale0=None, radius=8.0, flags=1, max_iter=100, tol=1e-10,
             max_outer=2, pos_tol=1e-3, max_step=0.5, max_move=2.0, min_snr=3.0, rows=np.full((n, 16), -7.0),
             shifts=np.full((n, 2), -7.0), head=np.full(12, -7.0), resid=np.full((ny, nx), -7.0), on_device=0)
    a.update(override)

    def p(v):
        return None if v is None else C.c_void_p(np.ascontiguousarray(v).ctypes.data)
    keep = {k: np.ascontiguousarray(a[k]) if a[k] is not None else None
            for k in ('image', 'var', 'psf', 'index', 'origin', 'shift', 'scale0')}
    rc = ctx.lib.mpsfr_fit_frame_psf_free(
        ctx._h, a['ny'], a['nx'], p(keep['image']), p(keep['var']), a['nstar'], a['npsf'], p(keep['psf']),
        p(keep['index']), p(keep['origin']), p(keep['shift']), p(keep['scale0']), float(a['radius']), a['flags'],
        a['max_iter'], float(a['tol']), a['max_outer'], float(a['pos_tol']), float(a['max_step']), float(a['max_move']),
        float(a['min_snr']), p(a['rows']), p(a['shifts']), p(a['head']), p(a['resid']), a['on_device'])
    return rc, a['rows'], a['shifts'], a['head'], a['resid']


def test_bad_arguments_are_refused_and_leave_the_outputs(api):
    ctx = _ctx(api, 'mixed')
    s = G.displaced_scene(True)
    n = s['n']
    far, nan, inf = s['shift'].copy(), s['shift'].copy(), np.zeros(n)
    far[2, 1], nan[5, 0], inf[1] = 8.25, np.nan, np.inf
    bad_index, bad_origin = s['index'].copy(), s['origin'].copy()
    bad_index[4], bad_origin[0, 0] = 4, (1 << 30) + 1
    neg_index = s['index'].copy()
    neg_index[0] = -1
    cases = [dict(ny=0), dict(nx=0), dict(ny=-1), dict(ny=16385), dict(nx=16385), dict(ny=8193, nx=8192),
             dict(nstar=0), dict(nstar=-1), dict(nstar=(1 << 20) + 1), dict(npsf=0), dict(npsf=-1),
             dict(image=None), dict(psf=None), dict(origin=None), dict(rows=None), dict(head=None), dict(shifts=None),
             dict(index=None),                                                    # npsf = 4 != nstar
             dict(radius=0.999), dict(radius=20.001), dict(radius=np.nan), dict(radius=np.inf), dict(radius=-8.0),
             dict(tol=0.0), dict(tol=1.0), dict(tol=-1e-10), dict(tol=np.nan), dict(tol=np.inf),
             dict(max_iter=0), dict(max_iter=-1), dict(max_iter=1001),
             dict(flags=2), dict(flags=4), dict(flags=3), dict(flags=-1),
             dict(max_outer=-1), dict(max_outer=17),
             dict(pos_tol=0.0), dict(pos_tol=-1e-3), dict(pos_tol=np.nan), dict(pos_tol=np.inf),
             dict(max_step=0.0), dict(max_step=1.001), dict(max_step=-0.5), dict(max_step=np.nan), dict(max_step=np.inf),
             dict(max_move=0.0), dict(max_move=4.001), dict(max_move=-1.0), dict(max_move=np.nan), dict(max_move=np.inf),
             dict(min_snr=-1e-3), dict(min_snr=np.nan), dict(min_snr=np.inf),
             dict(index=bad_index), dict(index=neg_index), dict(shift=far), dict(shift=nan), dict(origin=bad_origin),
             dict(scale0=inf), dict(scale0=np.full(n, np.nan))]
    for kw in cases:
        rc, rows, shifts, head, resid = _raw(ctx, s, **kw)
        assert rc == -1, kw
        assert b'fit_frame_psf_free' in ctx.lib.mpsfr_last_error(), kw
        assert all(np.all(out == -7.0) for out in (rows, shifts, head, resid) if out is not None), kw
    # their neighbours are legal, and var, shift, scale0 and resid_out are optional
    for kw in (dict(radius=1.0), dict(radius=20.0), dict(tol=0.999), dict(tol=1e-300, max_iter=2), dict(max_iter=1),
               dict(flags=0), dict(var=None), dict(shift=None), dict(scale0=np.zeros(n)), dict(resid=None),
               dict(max_outer=0), dict(max_outer=16, max_iter=2), dict(pos_tol=1e-300), dict(max_step=1.0),
               dict(max_move=4.0), dict(min_snr=0.0), dict(max_step=1e-300), dict(max_move=1e-300)):
        rc, rows, shifts, head, resid = _raw(ctx, s, **kw)
        assert rc == 0 and head[6] >= 1 and head[7] != -7.0 and np.all(rows[:, 7] != -7.0), kw
        assert np.all(shifts != -7.0) and np.all(head != -7.0), kw


# ---- 7. the chain
@pytest.mark.parametrize('prec', PRECS)
def test_find_refine_crowded_subtract_find(api, ctx, prec, monkeypatch):
    monkeypatch.setattr(api.psfrec, 'get_context', lambda *a, **k: ctx)
    pos, flux, chain = F.loop_field()
    psf = FR.model()
    n = len(pos)
    frame = ctx.render_stars(psf[None], (np.rint(pos) - NS // 2).astype(np.int32), flux, shift=pos - np.rint(pos),
                             psf_index=np.zeros(n, dtype=np.int32), image=F.loop_background())
    var = np.ones_like(frame)
    ps = 0.2
    found = api.find_stars(frame, psf, var, pixscale=ps, **F.LOOP_FIND)
    assert len(found) == n
    fp = np.asarray(found['position'])
    near = np.argmin(((fp[:, None] - pos[None]) ** 2).sum(-1), axis=1)
    member = np.isin(near, chain)
    rms = {}
    fits = {}
    for mode in ('frame', 'free'):
        fit, origin = api.fit_found_stars(frame, psf, found, var=var, crit=F.LOOP_CRIT, pixscale=ps, crowded=mode)
        assert np.array_equal(np.asarray(fit['crowded']), member) and member.sum() == F.LOOP_CHAIN
        where = origin[np.asarray(fit['group'])] + NS // 2 + np.asarray(fit['shift']) / ps
        rms[mode] = float(np.sqrt(np.mean((where[member] - pos[near[member]]) ** 2)))
        fits[mode] = (fit, origin)
    print('chain %s: rms position error of the chain %.4f px with crowded=frame, %.4f px with crowded=free' %
          (prec, rms['frame'], rms['free']))
    assert rms['free'] < rms['frame']
    fit, origin = fits['free']
    held = fits['frame'][0]
    for name in fit.colnames:                                     # the singles and blends: as before, bit for bit
        np.testing.assert_array_equal(np.asarray(fit[name])[~member], np.asarray(held[name])[~member])
    assert np.all(np.asarray(fit['err_shift'])[member] > 0) and np.all(np.asarray(held['err_shift'])[member] == 0)
    for name in ('scale', 'flux', 'err_scale', 'err_flux', 'back', 'chi2'):
        assert np.all(np.isfinite(np.asarray(fit[name]))), name
    residual, status = api.subtract_stars(frame, psf[None], origin, fit, psf_index=np.zeros(len(origin), dtype=np.int32),
                                          pixscale=ps)
    assert np.all(status == 0)
    assert len(api.find_stars(residual, psf, var, pixscale=ps, **F.LOOP_FIND)) == 0
    # refine_crowded_stars on the whole frame, from the finder's table
    allfit, og, res = api.refine_crowded_stars(frame, psf, found, var=var, start='found', return_residual=True, pixscale=ps)
    assert np.all(np.asarray(allfit['status']) == 0) and allfit.meta['status'] in (0, 1) and allfit.meta['outer'] >= 1
    assert abs(allfit.meta['back'] - 5.0) < 0.1 and len(api.find_stars(res, psf, var, pixscale=ps, **F.LOOP_FIND)) == 0
    err = np.asarray(allfit['position']) - pos[near]
    assert np.sqrt(np.mean(err ** 2)) < np.sqrt(np.mean((fp - pos[near]) ** 2))
    np.testing.assert_allclose(np.asarray(allfit['position']), og + NS // 2 + np.asarray(allfit['shift']) / ps, rtol=1e-13)
