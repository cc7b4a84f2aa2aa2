"""GPU: the crowded-field fit of a cube with free positions (mpsfr_fit_cube_psf_free; cube_free.hip).

1. parity with the converged yardstick (cube_free_ref) on the noiseless cube of cube_free_cases -- var on / off x
   background on / off x radius 4 and 8, both precisions: every free star's final shift within pos_tol rho / (1 - rho)
   plus the inner term derived there, the outer step count, the per-star step counts and the flags those of the rule;
   rows and heads against the dense per-layer solves at the returned shifts within section 24's bounds.  One
   Gauss-Newton step on the noisy cube against the rule with exact solves, the position errors from the yardstick's
   blocks, its chi2 / dof and its F.
   Worst error / bound ratios go to record_margin('cube_free', ...).
2. layer l of the residual cube is render_stars(subtract) of shift_out + layer_shift[l] and column 0 of layer l, bit for
   bit, also at max_outer = 0 and max_iter = 1.
3. bits: the same call twice, mixed = f64, host = device pointers, shift_out fed to fit_cube_psf_device as it is; both
   power-of-two laws with every position, position error, flag and count bit for bit.
4. agreement with the frame call: nl = 1 against fit_frame_psf_free, three identical layers against the single frame,
   within the sum of the bounds (not bits: here delta is the unknown, there a = F delta).
5. edges: the all-NaN layer and the others blind to it, the star masked in one layer, the star under min_snr in one
   layer, nobody free, max_move, max_step, a layer_shift that makes the +-8 bound bind, one star on a 1 x 2 frame with
   three layers, the 33 x 31 frame, cube_fit_cases.lattice(2) with a tile list longer than 256.
6. refusals: every MPSFR_E_INVALID of the header, outputs untouched.
"""
import ctypes as C

import numpy as np
import pytest

import cube_fit_cases as K
import cube_free_cases as Q
import cube_free_ref as R
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


def _free(ctx, c, with_var=True, background=True, radius=8.0, **kw):
    """(rows, pos, shifts, head, call[, residual]) of the host form on a case dict."""
    return ctx.fit_cube_psf_free(c['cube'], c['psf'], c['origin'], var=c['var'] if with_var else None,
                                 shift=c['shift'], layer_shift=c['layer_shift'], psf_index=c['index'], radius=radius,
                                 background=background, **kw)


def _render_of(ctx, c, l, rows, shifts):
    acc = np.flatnonzero(rows[l, :, 7] == 0)
    sh = shifts if c['layer_shift'] is None else shifts + c['layer_shift'][l]
    return ctx.render_stars(np.ascontiguousarray(c['psf'][:, l]), c['origin'][acc], rows[l, acc, 0], shift=sh[acc],
                            psf_index=c['index'][acc], image=np.ascontiguousarray(c['cube'][l]), subtract=True)


_BASE = {}


def _base(ctx, prec):
    """The call on the noisy cube at its defaults, with its residual, once per precision."""
    if prec not in _BASE:
        _BASE[prec] = _free(ctx, Q.cube(True), return_residual=True)
    return _BASE[prec]


# ---- 1. parity
_RULE = {}


def _check_layer(rows, head, ref, b, acc):
    """The rows and the head of one layer against the dense solve at the returned shifts (section 24's checks)."""
    nacc = len(acc)
    assert 0 <= head[4] <= MAX_ITER and 0 <= head[5]
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
    c = Q.cube(False)
    n, nl = c['n'], Q.NL
    conv = Q.cube_converged(with_var, background, radius, False, max_outer=10)
    cp, free = conv['problem'], conv['last']['free']
    assert conv['rho'] < 0.5 and cp.live == [0, 1, 2]
    pos_tol = R.parity_pos_tol(conv, TOL, MAX_ITER)
    bound, _ = R.position_bounds(conv, pos_tol, TOL, MAX_ITER)
    steps = np.array(conv['steps'])
    assert not np.any(np.abs(steps - pos_tol) <= 0.1 * pos_tol)
    nouter = int(np.argmax(steps <= pos_tol)) + 1
    rows, pos, shifts, head, call = _free(ctx, c, with_var, background, radius, max_iter=MAX_ITER, tol=TOL, max_outer=10,
                                          pos_tol=pos_tol)
    assert rows.shape == (nl, n, 8) and pos.shape == (n, 8) and shifts.shape == (n, 2) and head.shape == (nl, 8)
    assert call.shape == (8,)
    tag = '%s_%s_%s_r%d' % (prec, 'var' if with_var else 'unit', 'back' if background else 'noback', int(radius))
    key = (with_var, background, radius)
    if key not in _RULE:
        _RULE[key] = Q.run(c, with_var, background, radius, max_outer=10, pos_tol=pos_tol)
    rule = _RULE[key]
    assert rule['nouter'] == nouter and rule['posok']
    # who is fitted, the counts, the stop: exact
    for l in range(nl):
        pr = cp.layers[l]
        np.testing.assert_array_equal(rows[l, :, 7], pr.base['status'])
        np.testing.assert_array_equal(rows[l, :, 5], pr.base['ndisc'])
        assert (head[l, 3], head[l, 6], head[l, 7]) == (pr.nomega, pr.nacc, 0)
    assert (call[2], call[4], call[6]) == (nouter, len(free), 0) and call[3] <= pos_tol and call[7] <= TOL
    assert call[1] == sum(p.nomega - p.nacc - (1 if background else 0) for p in cp.layers) - 2 * len(free)
    assert abs(call[0] - head[:, 2].sum()) <= 4 * EPS * call[0] and np.all(head[:, 4] == head[0, 4])
    np.testing.assert_array_equal(pos[:, 7], rule['nfree'])
    np.testing.assert_array_equal(pos[:, 6], rule['flags'])
    # the star masked in layer 1 is left out there and carried by the two others
    assert rows[Q.MASK_LAYER, Q.MASKED, 7] == 2 and list(conv['carried'][:, Q.MASKED]) == [True, False, True]
    assert pos[Q.MASKED, 7] == nouter and np.all(pos[Q.MASKED, 2:4] > 0)
    # a star accepted nowhere echoes its shift and is zero elsewhere
    out = np.flatnonzero(~cp.seen)
    assert len(out) >= 2 and _same(shifts[out], c['shift'][out]) and not pos[out, 2:].any() and not rows[:, out, :7].any()
    assert _same(pos[:, :2], shifts) and _same(pos[cp.seen, 4:6], shifts[cp.seen] - c['shift'][cp.seen])
    # the positions against the joint minimiser
    ratios = dict(position=float(np.max(np.abs(shifts[free] - conv['shift'][free]) / bound)))
    # the closing solve of every layer against the dense solve at the returned shifts
    for l in range(nl):
        ref = cp.layers[l].held(shifts + c['layer_shift'][l])
        for k, v in _check_layer(rows[l], head[l], ref, F.bounds(ref, TOL, MAX_ITER), cp.layers[l].acc).items():
            ratios[k] = max(ratios.get(k, 0.0), v)
    for k, v in ratios.items():
        assert v < 1.0, (k, v)
    print('cube free %s: error / bound %s; pos_tol %.2e, %d outer steps, %d inner iterations' %
          (tag, ', '.join('%s %.2e' % kv for kv in sorted(ratios.items())), pos_tol, call[2], call[5]))
    record_margin('cube_free', **{'%s_%s' % (k, tag): v for k, v in ratios.items()})


@pytest.mark.parametrize('prec', PRECS)
def test_one_step_on_the_noisy_cube_follows_the_rule(ctx, prec):
    c = Q.cube(True)
    rows, pos, shifts, head, call = _free(ctx, c, max_iter=MAX_ITER, tol=TOL, max_outer=1)
    ref = check_one_step(c, rows, pos, shifts, head, call)
    record_margin('cube_free', **{'one_step_%s' % prec: ref['ratio']})


_ONE_STEP = {}


def check_one_step(c, rows, pos, shifts, head, call, **kw):
    """The outputs of a call with max_iter = MAX_ITER, tol = TOL, max_outer = 1 and the step parameters `kw` on the
    three-layer case `c` = Q.cube(True) (var, background, radius 8) against one step of the rule with exact solves.  Returns the
    yardstick's run with the worst position error / bound under 'ratio'."""
    assert c is Q.cube(True)                     # (the yardstick is kept per step parameters, of this case alone)
    key = tuple(sorted(kw.items()))
    if key not in _ONE_STEP:
        _ONE_STEP[key] = Q.run(c, max_outer=1, **kw)
    ref = _ONE_STEP[key]
    free = ref['last']['free']
    _, by, bx = R.inner_bounds(ref['last'], TOL, MAX_ITER, Q.NL)
    ratio = float(np.max(np.abs(shifts[free] - ref['shift'][free]) / np.stack([by, bx], axis=1)))
    assert ratio < 1.0
    np.testing.assert_array_equal(pos[:, 6], ref['flags'])
    np.testing.assert_array_equal(pos[:, 7], ref['nfree'])
    assert (call[2], call[4]) == (1, ref['nfree_last']) and call[6] == (0 if ref['steps'][0] <= 1e-3 else 1)
    assert abs(call[3] - ref['steps'][0]) <= float(max(by.max(), bx.max()))
    seen = ref['problem'].seen
    assert 0 < ref['nfree_last'] <= seen.sum() and np.all(head[:, 7] == call[6])
    held = np.flatnonzero(seen & (ref['nfree'] == 0))
    assert _same(shifts[held], c['shift'][held]) and not pos[held, 2:6].any()
    np.testing.assert_allclose(pos[free, 2:4], ref['err_shift'][free], rtol=1e-6)
    return dict(ref, ratio=ratio)


# ---- 2. the residual cube is the renderer's
@pytest.mark.parametrize('prec', PRECS)
def test_residual_equals_render_subtract_bit_for_bit(ctx, prec):
    c = Q.cube(True)
    rows, pos, shifts, head, call, resid = _base(ctx, prec)
    assert call[2] >= 1 and np.abs(shifts - c['shift']).max() > 0.05
    for l in range(Q.NL):
        assert set(rows[l, :, 7]) == {0.0, 1.0, 2.0} and _same(resid[l], _render_of(ctx, c, l, rows, shifts))
    assert np.array_equal(np.isnan(resid), np.isnan(c['cube']))
    for kw in (dict(max_outer=0), dict(max_iter=1), dict(max_outer=2, max_iter=3)):
        r, p, sh, h, ca, d = _free(ctx, c, return_residual=True, **kw)
        assert all(_same(d[l], _render_of(ctx, c, l, r, sh)) for l in range(Q.NL)), kw
        assert all(np.all(np.isfinite(a)) for a in (r, p, sh, h, ca)), kw
        assert ca[6] == (1 if 'max_iter' in kw else 0), kw
    # without the residual cube the outputs are the same bits
    assert all(_same(x, y) for x, y in zip(_free(ctx, c), (rows, pos, shifts, head, call)))


# ---- 3. bits
@pytest.mark.parametrize('prec', PRECS)
def test_same_call_twice_gives_the_same_bits(ctx, prec):
    a = _base(ctx, prec)
    b = _free(ctx, Q.cube(True), return_residual=True)
    assert all(_same(x, y) for x, y in zip(a, b))


def test_mixed_gives_the_bits_of_f64(api):
    a, b = _base(_ctx(api, 'mixed'), 'mixed'), _base(_ctx(api, 'f64'), 'f64')
    assert all(_same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('prec', PRECS)
def test_device_pointers_give_the_bits_of_the_host_form(ctx, prec):
    import torch
    c = Q.cube(True)
    ny, nx = F.FRAME
    n, nl = c['n'], Q.NL
    dev = torch.device('cuda:0')
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev)
         for k in ('cube', 'var', 'psf', 'index', 'origin', 'shift', 'layer_shift')}

    def buf(*shape):
        return torch.full(shape, -1.0, dtype=torch.float64, device=dev)
    trow, thead, tpos, tsh, tcall, tres = buf(nl, n, 8), buf(nl, 8), buf(n, 8), buf(n, 2), buf(8), buf(nl, ny, nx)
    torch.cuda.synchronize()
    ctx.fit_cube_psf_free_device(nl, ny, nx, t['cube'].data_ptr(), n, 4, t['psf'].data_ptr(), t['origin'].data_ptr(),
                                 trow.data_ptr(), thead.data_ptr(), tpos.data_ptr(), tsh.data_ptr(), tcall.data_ptr(),
                                 var_ptr=t['var'].data_ptr(), shift_ptr=t['shift'].data_ptr(),
                                 layer_shift_ptr=t['layer_shift'].data_ptr(), psf_index_ptr=t['index'].data_ptr(),
                                 resid_ptr=tres.data_ptr())
    ctx.sync()
    got = tuple(x.cpu().numpy() for x in (trow, tpos, tsh, thead, tcall, tres))
    assert all(_same(x, y) for x, y in zip(got, _base(ctx, prec)))
    # shift_out is what the flux-only cube fit reads: a device chain without repacking
    trow8, thead8 = buf(nl, n, 8), buf(nl, 8)
    torch.cuda.synchronize()
    ctx.fit_cube_psf_device(nl, ny, nx, t['cube'].data_ptr(), n, 4, t['psf'].data_ptr(), t['origin'].data_ptr(),
                            trow8.data_ptr(), thead8.data_ptr(), var_ptr=t['var'].data_ptr(), shift_ptr=tsh.data_ptr(),
                            layer_shift_ptr=t['layer_shift'].data_ptr(), psf_index_ptr=t['index'].data_ptr())
    ctx.sync()
    # (the flux-only solve draws its discs around the refined centres, the free one around the start: another Omega,
    # and the star masked in layer 1 gets a few pixels back; what it must equal is the host form at the same shifts,
    # which section 25 pins bit for bit)
    want = ctx.fit_cube_psf(c['cube'], c['psf'], c['origin'], var=c['var'], shift=got[2], layer_shift=c['layer_shift'],
                            psf_index=c['index'])
    assert _same(trow8.cpu().numpy(), want[0]) and _same(thead8.cpu().numpy(), want[1])
    assert np.array_equal(want[0][0, :, 7], got[0][0, :, 7]) and np.all(want[1][:, 7] == 0)


@pytest.mark.parametrize('prec', PRECS)
def test_power_of_two_scaling_laws_hold_bit_for_bit(ctx, prec):
    c = Q.cube(True)
    rows, pos, shifts, head, call, resid = _base(ctx, prec)
    start = np.where(rows[:, :, 7] == 0, rows[:, :, 0] * 0.75, 0.0)
    r0, p0, s0, h0, c0, d0 = _free(ctx, c, scale0=start, return_residual=True)
    assert c0[2] >= 1
    # a power of two on var: chi2 and N_kk scale with 1 / var, nothing else moves
    r1, p1, s1, h1, c1, d1 = _free(ctx, dict(c, var=c['var'] * 16.0), return_residual=True)
    for k in (0, 1, 2, 3, 4, 5, 7):
        assert _same(r1[:, :, k], rows[:, :, k]), k
    assert _same(r1[:, :, 6] * 16.0, rows[:, :, 6]) and _same(s1, shifts) and _same(p1, pos) and _same(d1, resid)
    assert _same(h1[:, [0, 1, 3, 4, 5, 6, 7]], head[:, [0, 1, 3, 4, 5, 6, 7]]) and _same(h1[:, 2] * 16.0, head[:, 2])
    assert _same(c1[1:], call[1:]) and c1[0] * 16.0 == call[0]
    # 2^k on the data (and the start) with 4^k on var: the fluxes, their errors and b scale by 2^k
    for k in (3, -5):
        f = 2.0 ** k
        t = dict(c, cube=c['cube'] * f, var=c['var'] * f * f)
        r2, p2, s2, h2, c2, d2 = _free(ctx, t, scale0=start * f, return_residual=True)
        assert _same(r2[:, :, :4], r0[:, :, :4] * f) and _same(r2[:, :, [4, 5, 7]], r0[:, :, [4, 5, 7]])
        assert _same(r2[:, :, 6] * f * f, r0[:, :, 6]) and _same(p2, p0) and _same(s2, s0)
        assert _same(h2[:, :2], h0[:, :2] * f) and _same(h2[:, 2:], h0[:, 2:]) and _same(c2, c0) and _same(d2, d0 * f)


# ---- 4. agreement with the frame call
def _frame_as_cube(s, copies):
    return dict(cube=np.stack([s['image']] * copies), var=np.stack([s['var']] * copies),
                psf=np.ascontiguousarray(np.stack([s['psf']] * copies, axis=1)), index=s['index'], origin=s['origin'],
                shift=s['shift'], layer_shift=None, n=s['n'])


_COPIES = {}


@pytest.mark.parametrize('copies', [1, 3])
@pytest.mark.parametrize('prec', PRECS)
def test_identical_layers_agree_with_the_frame_call(ctx, prec, copies):
    # (the joint minimiser of identical layers is the single layer's; both runs end within their own bound of it)
    s = G.displaced_scene(False)
    c = _frame_as_cube(s, copies)
    conv_f = G.scene_converged(True, True, 8.0, False, max_outer=10)
    if copies not in _COPIES:
        _COPIES[copies] = R.converged(c['cube'], c['var'], c['psf'], c['index'], c['origin'], c['shift'], None, 8.0, True,
                                      max_outer=10)
    conv_c = _COPIES[copies]
    assert conv_f['rho'] < 0.5 and conv_c['rho'] < 0.5
    pos_tol = max(G.parity_pos_tol(conv_f, TOL, MAX_ITER), R.parity_pos_tol(conv_c, TOL, MAX_ITER))
    bf, _ = G.position_bounds(conv_f, pos_tol, TOL, MAX_ITER)
    bc, _ = R.position_bounds(conv_c, pos_tol, TOL, MAX_ITER)
    acc = conv_f['problem'].acc
    free_f, free_c = acc[conv_f['last']['free_idx']], conv_c['last']['free']
    assert np.array_equal(free_f, free_c)
    kw = dict(max_iter=MAX_ITER, tol=TOL, max_outer=10, pos_tol=pos_tol)
    rows, pos, shifts, head, call = _free(ctx, c, **kw)
    frows, fshifts, fhead = ctx.fit_frame_psf_free(s['image'], s['psf'], s['origin'], var=s['var'], shift=s['shift'],
                                                   psf_index=s['index'], **kw)
    assert np.all(np.abs(shifts[free_c] - fshifts[free_c]) <= bf + bc)
    assert call[6] == fhead[7] == 0 and np.array_equal(pos[:, 6], frows[:, 14])
    for l in range(copies):
        np.testing.assert_array_equal(rows[l, :, [5, 7]], frows[:, [5, 7]].T)
    assert all(_same(rows[l], rows[0]) for l in range(copies))


# ---- 5. edges
@pytest.mark.parametrize('prec', PRECS)
def test_a_dead_layer_and_the_others_blind_to_it(ctx, prec):
    c = Q.two_layers('nan')
    rows, pos, shifts, head, call, resid = _free(ctx, c, return_residual=True)
    assert head[1, 7] == 2 and not head[1, :3].any() and not rows[1, :, :7].any() and np.all(rows[1, :, 7] >= 1)
    assert np.all(np.isnan(resid[1])) and head[0, 7] == call[6] != 2 and call[2] >= 1
    one = dict(c, cube=c['cube'][:1], var=c['var'][:1], psf=np.ascontiguousarray(c['psf'][:, :1]),
               layer_shift=c['layer_shift'][:1])
    r1, p1, s1, h1, c1, d1 = _free(ctx, one, return_residual=True)
    assert _same(r1[0], rows[0]) and _same(p1, pos) and _same(s1, shifts) and _same(h1[0], head[0]) and _same(c1, call)
    assert _same(d1[0], resid[0])
    # the dead layer first: the same bits again
    back = dict(c, cube=c['cube'][::-1].copy(), var=c['var'][::-1].copy(), psf=np.ascontiguousarray(c['psf'][:, ::-1]),
                layer_shift=c['layer_shift'][::-1].copy())
    r2, p2, s2, h2, c2 = _free(ctx, back)
    assert _same(r2[1], rows[0]) and _same(p2, pos) and _same(s2, shifts) and _same(h2[1], head[0]) and _same(c2, call)
    assert h2[0, 7] == 2
    # every layer dead: status 2, the shifts echoed
    dead = dict(c, cube=np.full_like(c['cube'], np.nan))
    r3, p3, s3, h3, c3 = _free(ctx, dead)
    assert c3[6] == 2 and np.all(h3[:, 7] == 2) and _same(s3, c['shift']) and not p3[:, 2:].any() and not c3[:6].any()


@pytest.mark.parametrize('prec', PRECS)
def test_a_star_under_min_snr_in_one_layer_is_carried_by_the_other(ctx, prec):
    c = Q.two_layers('faint')
    ref = Q.run(c, max_outer=1)
    assert list(ref['carried'][:, Q.FAINT]) == [True, False]
    both = Q.run(c, max_outer=1, min_snr=0.0)
    assert list(both['carried'][:, Q.FAINT]) == [True, True]
    _, by, bx = R.inner_bounds(ref['last'], TOL, MAX_ITER, 2)
    bound = np.stack([by, bx], axis=1)
    free = ref['last']['free']
    j = int(np.flatnonzero(free == Q.FAINT)[0])
    # (the two rules differ for this star by more than the bound: the test can tell which layers carried it)
    assert np.abs(ref['shift'][Q.FAINT] - both['shift'][Q.FAINT]).max() > 4.0 * bound[j].max()
    rows, pos, shifts, head, call = _free(ctx, c, max_iter=MAX_ITER, tol=TOL, max_outer=1)
    assert np.all(np.abs(shifts[free] - ref['shift'][free]) <= bound)
    np.testing.assert_array_equal(pos[:, 7], ref['nfree'])
    np.testing.assert_array_equal(pos[:, 6], ref['flags'])
    np.testing.assert_allclose(pos[free, 2:4], ref['err_shift'][free], rtol=1e-6)
    assert rows[1, Q.FAINT, 7] == 0


def _layers(shape, pos, flux, index, ls, scale=(1.0, 0.5, 2.0)):
    """A noiseless cube of len(ls) layers of well separated stars: the case dict at the true positions, and the truth."""
    base = F.Y.models()
    nl = len(ls)
    psf = np.ascontiguousarray(np.stack([np.roll(base, l, axis=0) for l in range(nl)], axis=1))
    pos = np.asarray(pos, dtype=float)
    origin = (np.rint(pos) - NS // 2).astype(np.int32)
    shift = pos - (origin + NS // 2)
    index = np.asarray(index, dtype=np.int32)
    cube = np.stack([F.Y.render(None, np.ascontiguousarray(psf[:, l]), index, origin, shift + ls[l],
                                np.asarray(flux) * scale[l], shape=shape)[0] for l in range(nl)])
    return dict(cube=cube, var=None, psf=psf, index=index, origin=origin, shift=shift.copy(),
                layer_shift=np.asarray(ls, dtype=float), n=len(pos)), shift


TIGHT = dict(max_iter=200, tol=1e-12, max_outer=12, pos_tol=1e-9, background=False)
# (noiseless cubes of well separated stars: the joint minimiser is the truth, Gauss-Newton converges quadratically, the
# inner term kappa tol |y*| / sqrt(sum F^2 N_aa) with kappa of a few and tol 1e-12 is below 1e-10 px: 1e-8 px bounds the
# sum with a margin of ten over both, as in test_gpu_frame_free.py.)
EXACT = 1e-8
LS2 = [[0.0, 0.0], [0.11, -0.07]]


@pytest.mark.parametrize('prec', PRECS)
def test_the_clips_and_their_flags(ctx, prec):
    c, truth = _layers((40, 40), [[12.3, 13.4], [27.6, 25.2]], [1000.0, 800.0], [0, 2], LS2)
    start = truth + np.array([[0.3, 0.0], [0.0, 0.0]])
    c['shift'] = start
    # the unclipped call recovers the truth from both layers
    rows, pos, shifts, head, call = _free(ctx, c, with_var=False, **TIGHT)
    assert call[6] == 0 and np.abs(shifts - truth).max() <= EXACT and not pos[:, 6].any() and np.all(pos[:, 7] == call[2])
    np.testing.assert_allclose(rows[:, :, 0], np.outer([1.0, 0.5], [1000.0, 800.0]), rtol=1e-9)
    # max_move: star 0 comes to rest 0.2 px from its start, on the side of the truth; the loop cannot pass its test
    rows, pos, shifts, head, call = _free(ctx, c, with_var=False, **dict(TIGHT, max_move=0.2))
    assert shifts[0, 0] == start[0, 0] - 0.2 and int(pos[0, 6]) & G.BOUND and call[6] == 1 and call[2] == 12
    assert call[3] > 0.05 and not int(pos[1, 6]) & G.BOUND and np.abs(shifts[1] - truth[1]).max() < 5e-3
    # max_step: one step of 0.05 px, flagged; the other star's step is not
    rows, pos, shifts, head, call = _free(ctx, c, with_var=False, **dict(TIGHT, max_step=0.05, max_outer=1))
    assert shifts[0, 0] == start[0, 0] - 0.05 and int(pos[0, 6]) == G.CLIPPED and pos[1, 6] == 0
    assert (call[6], call[2]) == (1, 1) and 0.2 < call[3] < 0.4
    # nobody free: the call ends after the opening solve
    r0, p0, s0, h0, c0 = _free(ctx, c, with_var=False, **dict(TIGHT, max_outer=0))
    rows, pos, shifts, head, call = _free(ctx, c, with_var=False, **dict(TIGHT, min_snr=1e12))
    assert list(call[2:5]) == [0, 0, 0] and call[6] == 0 and _same(shifts, start)
    assert np.all(pos[:, 6] == G.HELD) and not pos[:, 7].any() and not pos[:, 2:6].any()
    np.testing.assert_allclose(rows[:, :, :7], r0[:, :, :7], rtol=1e-8, atol=1e-8)


@pytest.mark.parametrize('prec', PRECS)
def test_a_layer_shift_makes_the_bound_bind(ctx, prec):
    # the truth lies at shift 7.8 of this origin, the start at 7.3; layer 1 is offset by 0.5: 7.5 is as far as it goes
    ls = np.array([[0.0, 0.0], [0.5, 0.0]])
    base = F.Y.models()
    psf = np.ascontiguousarray(np.stack([base, np.roll(base, 1, axis=0)], axis=1))
    index = np.array([1], dtype=np.int32)
    cube = []
    for l in range(2):
        p = np.array([[37.8 + ls[l, 0], 30.0]])
        o = (np.rint(p) - NS // 2).astype(np.int32)
        cube.append(F.Y.render(None, np.ascontiguousarray(psf[:, l]), index, o, p - (o + NS // 2), [1000.0],
                               shape=(60, 60))[0])
    c = dict(cube=np.stack(cube), var=None, psf=psf, index=index, origin=np.array([[10, 10]], dtype=np.int32),
             shift=np.array([[7.3, 0.0]]), layer_shift=ls, n=1)
    lo, hi = R.shift_interval(ls)
    assert hi[0] == 7.5 and hi[1] == 8.0 and np.all(lo == -8.0)
    rows, pos, shifts, head, call = _free(ctx, c, with_var=False, **dict(TIGHT, max_move=4.0))
    assert shifts[0, 0] == 7.5 and int(pos[0, 6]) & G.BOUND and call[6] == 1 and abs(shifts[0, 1]) < 0.05
    assert np.all(rows[:, 0, 7] == 0) and np.all(np.isfinite(rows))
    # an offset whose bound is not a round number: the rounded sums stay inside
    odd = np.array([[0.0, 0.0], [0.1 + 0.2, -1.0 / 3.0]])
    lo, hi = R.shift_interval(odd)
    assert np.all(np.abs(hi + odd) <= 8.0) and np.all(np.abs(lo + odd) <= 8.0)
    rows, pos, shifts, head, call = _free(ctx, dict(c, layer_shift=odd), with_var=False, **dict(TIGHT, max_move=4.0))
    assert shifts[0, 0] == hi[0] and int(pos[0, 6]) & G.BOUND and np.all(rows[:, 0, 7] == 0)


@pytest.mark.parametrize('prec', PRECS)
def test_the_smallest_frames(ctx, prec):
    # 1 x 2 with one layer: two pixels carry one flux and no position; with three layers six pixels outnumber three
    # fluxes and one position -- the rule sets the star free
    psf1 = np.ascontiguousarray(np.stack([F.Y.models()[:1]] * 3, axis=1))
    cube = np.array([[[3.5, 2.5]], [[7.2, 4.9]], [[1.7, 1.3]]])
    c = dict(cube=cube, var=None, psf=psf1, index=np.zeros(1, dtype=np.int32), origin=np.array([[-20, -20]], dtype=np.int32),
             shift=np.array([[0.3, 0.4]]), layer_shift=None, n=1)
    one = dict(c, cube=cube[:1], psf=np.ascontiguousarray(psf1[:, :1]))
    rows, pos, shifts, head, call = _free(ctx, one, with_var=False, background=False, radius=1.0)
    assert (call[6], head[0, 3], call[2], call[4]) == (0, 2, 0, 0) and pos[0, 6] == G.HELD and _same(shifts, c['shift'])
    kw = dict(with_var=False, background=False, radius=1.0, max_outer=1, min_snr=0.0)
    ref = Q.run(c, **kw)
    rows, pos, shifts, head, call = _free(ctx, c, max_iter=MAX_ITER, tol=TOL, **kw)
    assert ref['nfree_last'] == 1 and (call[2], call[4]) == (1, 1) and pos[0, 7] == 1
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(pos)) and np.all(head[:, 3] == 2)
    # (the joint system is singular here -- on one row of two pixels the x column of a layer lies in the span of its
    # model and y columns, with the same coefficients in every layer -- so the step itself is not determined and is
    # not compared: the call has to follow the rule's counts, stay finite and inside its clips)
    assert np.all(np.abs(shifts - c['shift']) <= 0.5) and int(pos[0, 6]) & ~(G.CLIPPED | G.BOUND) == 0
    # 33 x 31: a star across the corner of the tile grid's first tile, two more; two layers with an offset
    p = np.array([[31.6, 29.8], [12.3, 8.9], [30.2, 3.1]])
    c, truth = _layers((33, 31), p, [900.0, 400.0, 1500.0], [0, 1, 3], LS2)
    c['shift'] = truth + np.array([[0.15, -0.2], [-0.1, 0.25], [0.2, 0.1]])
    rows, pos, shifts, head, call = _free(ctx, c, with_var=False, **TIGHT)
    assert call[6] == 0 and np.all(pos[:, 7] == call[2]) and np.abs(shifts - truth).max() <= 1e-6


@pytest.mark.parametrize('prec', PRECS)
def test_a_tile_list_longer_than_256(ctx, prec, api):
    c = dict(K.lattice(2))
    assert K.longest_tile_list(c['origin'], (80, 80)) > api.RENDER_SORT_CHUNK
    truth = c['shift']
    c['shift'] = truth + np.random.default_rng(6).uniform(-0.05, 0.05, truth.shape)
    kw = dict(with_var=False, radius=4.0, max_outer=1, min_snr=0.0)
    ref = Q.run(c, **kw)
    rows, pos, shifts, head, call, resid = _free(ctx, c, max_iter=1000, tol=TOL, return_residual=True, **kw)
    free = ref['last']['free']
    _, by, bx = R.inner_bounds(ref['last'], TOL, 1000, 2)
    err = np.abs(shifts[free] - ref['shift'][free])
    assert np.all(head[:, 6] == 289) and call[2] == 1 and call[4] == len(free) == ref['nfree_last'] == 289
    assert np.all(err <= np.stack([by, bx], axis=1))
    assert all(_same(resid[l], _render_of(ctx, c, l, rows, shifts)) for l in range(2))
    record_margin('cube_free', **{'lattice_%s' % prec: float(np.max(err / np.stack([by, bx], axis=1)))})


# ---- 6. refusals
def _raw(ctx, c, **override):
    """The C call on host pointers with sentinel outputs; returns (rc, the six outputs)."""
    n = c['n']
    nl, ny, nx = c['cube'].shape
    a = dict(nl=nl, ny=ny, nx=nx, cube=c['cube'], var=c['var'], nstar=n, npsf=len(c['psf']), psf=c['psf'],
             index=c['index'], origin=c['origin'], shift=c['shift'], layer_shift=c['layer_shift'], scale0=None, radius=8.0,
             flags=1, max_iter=100, tol=1e-10, max_outer=2, pos_tol=1e-3, max_step=0.5, max_move=2.0, min_snr=3.0,
             rows=np.full((nl, n, 8), -7.0), head=np.full((nl, 8), -7.0), pos=np.full((n, 8), -7.0),
             shifts=np.full((n, 2), -7.0), call=np.full(8, -7.0), resid=np.full((nl, ny, nx), -7.0), on_device=0)
    a.update(override)

    def p(v):
        return None if v is None else C.c_void_p(np.ascontiguousarray(v).ctypes.data)
    keep = {k: np.ascontiguousarray(a[k]) if a[k] is not None else None
            for k in ('cube', 'var', 'psf', 'index', 'origin', 'shift', 'layer_shift', 'scale0')}
    rc = ctx.lib.mpsfr_fit_cube_psf_free(
        ctx._h, a['nl'], a['ny'], a['nx'], p(keep['cube']), p(keep['var']), a['nstar'], a['npsf'], p(keep['psf']),
        p(keep['index']), p(keep['origin']), p(keep['shift']), p(keep['layer_shift']), p(keep['scale0']),
        float(a['radius']), a['flags'], a['max_iter'], float(a['tol']), a['max_outer'], float(a['pos_tol']),
        float(a['max_step']), float(a['max_move']), float(a['min_snr']), p(a['rows']), p(a['head']), p(a['pos']),
        p(a['shifts']), p(a['call']), p(a['resid']), a['on_device'])
    return rc, [a[k] for k in ('rows', 'head', 'pos', 'shifts', 'call', 'resid')]


def test_bad_arguments_are_refused_and_leave_the_outputs(api):
    ctx = _ctx(api, 'mixed')
    c = Q.cube(True)
    n, nl = c['n'], Q.NL
    far, nan, inf = c['shift'].copy(), c['shift'].copy(), np.zeros((nl, n))
    far[2, 1], nan[5, 0], inf[1, 1] = 8.25, np.nan, np.inf
    bad_index, bad_origin, neg_index = c['index'].copy(), c['origin'].copy(), c['index'].copy()
    bad_index[4], bad_origin[0, 0], neg_index[0] = 4, (1 << 30) + 1, -1
    ls_nan, ls_far = c['layer_shift'].copy(), c['layer_shift'].copy()
    ls_nan[1, 0], ls_far[2, 1] = np.nan, -7.9
    cases = [dict(nl=0), dict(nl=-1), dict(nl=4097), dict(ny=0), dict(nx=0), dict(ny=-1), dict(ny=16385), dict(nx=16385),
             dict(nstar=0), dict(nstar=-1), dict(nstar=(1 << 20) + 1), dict(npsf=0), dict(npsf=-1),
             dict(cube=None), dict(psf=None), dict(origin=None), dict(rows=None), dict(head=None), dict(pos=None),
             dict(shifts=None), dict(call=None),
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
             dict(scale0=inf), dict(scale0=np.full((nl, n), np.nan)), dict(layer_shift=ls_nan), dict(layer_shift=ls_far),
             dict(nl=4, ny=8192, nx=8192, layer_shift=None)]                      # 4 GiB of frames alone: above the budget
    for kw in cases:
        rc, outs = _raw(ctx, c, **kw)
        assert rc == -1, kw
        assert b'fit_cube_psf_free' in ctx.lib.mpsfr_last_error(), kw
        assert all(np.all(out == -7.0) for out in outs if out is not None), kw
    assert api.CUBE_FREE_WORK_BYTES == 4 << 30
    # their neighbours are legal, and var, shift, layer_shift, scale0 and resid_out are optional
    for kw in (dict(radius=1.0), dict(radius=20.0), dict(tol=1e-300, max_iter=2), dict(max_iter=1), dict(flags=0),
               dict(var=None), dict(shift=None), dict(layer_shift=None), dict(scale0=np.zeros((nl, n))), dict(resid=None),
               dict(max_outer=0), dict(max_outer=16, max_iter=2), dict(pos_tol=1e-300), dict(max_step=1.0),
               dict(max_move=4.0), dict(min_snr=0.0), dict(max_step=1e-300), dict(max_move=1e-300)):
        rc, outs = _raw(ctx, c, **kw)
        assert rc == 0 and np.all(outs[1][:, 6] >= 1) and np.all(outs[0][:, :, 7] != -7.0), kw
        assert all(np.all(out != -7.0) for out in outs[1:5]), kw
