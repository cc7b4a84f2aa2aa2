"""GPU: a call's result does not depend on what ran before it on the same context.

One Context serves every entry point, and they all share the per-lane workspaces of mpsfr_api.cpp (D0t, dlin, pre,
fin, band, mpart, ...; the audit is DESIGN.md "Call-order independence").  A *checked call* run right after a
*predecessor* on the same context must equal the same call on a fresh context with the same options, bit for bit:
stamps, stamp sums and fits.  The context runs the checked call once before the predecessor, as a user's context has,
so that the predecessor writes into workspaces already sized for the checked call (a reallocation would zero them).  The first row of every checked call is also held to the oracle (the tolerances of
tests/test_gpu_random.py), so that the two sides cannot share a bug.

Predecessors (each run to completion, options restored afterwards):
  P1 a row at L0 = 5 m (the full-size form of stage A writes the whole D0t half plane)
  P2 stage_a = 0 (the full-size form by option); the other consumers of D0t and the FFT-free convolutions by
     option (otf_mfma 0, mf_kernel 1, fft_conv 0), the series form without the support skip
  P4 psf_from_psd on a finite PSD whose transform overflows (non-finite D in the whole plane)
  P5 psf_from_psd on a PSD with a NaN pixel (refused before anything is queued)
  P6 layout shifts: more tasks per chunk, other direction counts, and the reverse
  P7 the other entry points: profile, field, band, convolve_stamps, the device elliptical fit, psd_to_psf
  P8 the device circular fit (fit_stamps_device)
  P10 psd_to_psf at a smaller transform length, and on a PSD with a NaN (its own workspaces left holding NaN)
  P9 the fifteen stamp, frame and cube calls of tests/stamp_history_cases.py in sequence (the staging buffer and the
     frame workspaces; the other direction is tests/test_gpu_stamp_call_history.py)
"""
import numpy as np
import pytest

import psd_to_psf_ref as PR
import psfr_oracle as O
from conftest import H, record_margin, rel_err

pytestmark = pytest.mark.gpu

LB = np.array([495.0, 690.0, 915.0])      # (>= 486 nm: the crop of the native 1280^2 grid)
SEE = np.array([0.9, 1.1, 0.7])
GL = np.array([0.6, 0.45, 0.8])
L0 = np.array([22.0, 13.0, 27.0])          # (9-29 m, like the bench rows: the series form of stage A)
THREE = np.array([0, 1, 0], np.uint8)
POS = [(0.0, 0.0), (25.0, -15.0)]
BANDS = [(LB[0], LB[-1]), (600.0, 800.0)]
TOL = {'mixed': 2e-5, 'f64': 1e-9}

# checked calls: name -> (dim, precision, options, kind, npsflin)
CHECKED = {
    'd512': (512, 'mixed', {}, 'psf', 1),
    'd512_f64': (512, 'f64', {}, 'psf', 1),
    'd512_rowfft': (512, 'mixed', {'otf_mfma': 0}, 'psf', 1),
    'd512_mf1': (512, 'mixed', {'mf_kernel': 1}, 'psf', 1),
    'd256_npl2': (256, 'mixed', {}, 'psf', 2),
    'd256': (256, 'mixed', {}, 'psf', 1),        # (one direction at 256^2: the full-size form of stage A)
    'd1280': (1280, 'mixed', {}, 'psf', 1),
    'field512': (512, 'mixed', {}, 'field', 1),
    'band512': (512, 'mixed', {}, 'band', 1),
    # mpsfr_reconstruct_profile on the three-layer profile of tests/golden/g9_profile.npz (case a, the reference's
    # cut-off masks) and mpsfr_psd_to_psf at the transform length 256 on the 512^2 grid, both precisions of the context
    'profile512': (512, 'mixed', {}, 'profile', 1),
    'profile512_f64': (512, 'f64', {}, 'profile', 1),
    'psd2psf512': (512, 'mixed', {}, 'p2p', 1),
    'psd2psf512_f64': (512, 'f64', {}, 'p2p', 1),
}
_GOLD = {}


@pytest.fixture(scope='module', autouse=True)
def _fixtures(golden, ref_masks):
    _GOLD.update(g9=golden('g9_profile'), masks=ref_masks)


_P2P = {}


def _p2p_inputs():
    """psd_to_psf as tests/test_gpu_psd_to_psf_inputs.py::test_sizes calls it at (512, 256), phased: an odd random
    pupil, the PSD without symmetry, a random static phase, two wavelengths."""
    if not _P2P:
        dimnum, lb = 256, 500e-9
        pup = PR.rand_pupil(dimnum // 2 - 3)
        _P2P.update(pup=pup, psd=PR.scaled_psd(PR.asym_psd(512), pup, 8.0, lb, dimnum, 10.0), dimnum=dimnum,
                    phase=PR.rand_phase(dimnum // 2 - 3, 1.0, lb), lbda=np.array([lb, 850e-9]))
    return _P2P


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _context(api, name):
    dim, prec, opts, _, _ = CHECKED[name]
    ctx = api.Context(dim=dim, pixscale=api.grid_pixscale(dim), precision=prec)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def _run(api, ctx, name, l0=L0, _async=False):
    dim, prec, opts, kind, npl = CHECKED[name]
    if kind == 'psf':
        return ctx.reconstruct(LB, SEE, GL, l0, THREE, H, npsflin=npl, _async=_async)
    if kind == 'field':
        return ctx.reconstruct_field(LB, SEE, GL, l0, THREE, H, POS, _async=_async)
    if kind == 'profile':
        g = _GOLD['g9']
        return ctx.reconstruct_profile(g['a_lbda'], [float(g['a_seeing'])], [float(g['a_gl'])], [float(g['a_L0'])],
                                       g['a_cn2'], g['a_h'], g['a_ws'], g['a_wd'], three_lgs=[int(g['a_three'])],
                                       npsflin=int(g['a_npsflin']), masks=_GOLD['masks'], _async=_async)
    if kind == 'p2p':
        a = _p2p_inputs()
        return dict(psf=ctx.psd_to_psf(a['psd'], a['pup'], 8.0, a['lbda'], phase_static=a['phase'],
                                       dimnum=a['dimnum'])[0])
    return ctx.reconstruct_band(LB, api.band_weights(LB, BANDS), SEE, GL, l0, THREE, H, _async=_async)


def _keys(a, b):
    assert sorted(a) == sorted(b) and ('psf' in a) and (len(a) == 1 or sorted(a) == ['fit', 'psf', 'psf_sum'])
    return sorted(a)                           # (psd_to_psf returns its planes alone)


def _same(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in _keys(a, b))


def _diff(a, b):
    return {k: (int(np.sum(a[k] != b[k])), int(np.sum(~np.isfinite(a[k])))) for k in _keys(a, b)}


def _hold_profile(name, r, prec):
    """Case a of tests/golden/g9_profile.npz as tests/test_gpu_profile.py holds it: the reference's final stamps and
    its Moffat fits, at that test's tolerances."""
    import test_gpu_profile as TP
    from muse_psfr_amd import grid_pixscale
    e = TP.check_final_stamps_and_fits(_GOLD['g9'], 'a', prec, grid_pixscale(512), r, 1)
    record_margin('call_history_vs_oracle', **{name: e})


def _hold_p2p(name, r):
    """Every plane against the fp64 yardstick tests/psd_to_psf_ref.py with the checks and the bound of
    tests/test_gpu_psd_to_psf_inputs.py."""
    import test_gpu_psd_to_psf_inputs as TI
    a = _p2p_inputs()
    TI._check('call_history_' + name, r['psf'], PR.psd_to_psf_ref(a['psd'], a['pup'], 8.0, a['lbda'], a['phase'],
                                                                 a['dimnum']))


_FRESH = {}


def _fresh(api, name):
    """The checked call on a fresh context, its first row held to the oracle (once per module)."""
    if name in _FRESH:
        return _FRESH[name]
    ctx = _context(api, name)
    r = _run(api, ctx, name)
    ctx.close()
    dim, prec, _, kind, npl = CHECKED[name]
    if kind in ('profile', 'p2p'):
        if kind == 'profile':
            _hold_profile(name, r, prec)
        else:
            _hold_p2p(name, r)
        assert all(np.all(np.isfinite(v)) for v in r.values()), name
        _FRESH[name] = r
        return r
    ps = api.grid_pixscale(dim)
    tabs = O.ao_tables(H, bool(THREE[0]), npl, exact_masks=True)
    ofit, ofin = O.compute_psf(LB, SEE[0], GL[0], L0[0], npl, H, bool(THREE[0]), dim=dim, pixscale=ps,
                               tables=tabs, fit=kind == 'psf' and dim == 512)
    if kind == 'psf':
        got = r['psf'][0]
    elif kind == 'field':
        got = r['psf'][0, 0]                   # (the centre position is the npsflin = 1 direction)
    else:
        w = api.band_weights(LB, BANDS)
        ofin = np.einsum('bl,lij->bij', w / w.sum(axis=1, keepdims=True), ofin)
        got = r['psf'][0]
    e = rel_err(got, ofin)
    record_margin('call_history_vs_oracle', **{name: e})
    assert e < TOL[prec], (name, e)
    if ofit is not None:
        well = ofit[:, 4] < 10
        dfw = np.abs(r['fit'][0][:, 5] * ps - ofit[:, 3])[well].max(initial=0.0)
        dbe = np.abs(r['fit'][0][:, 4] - ofit[:, 4])[well].max(initial=0.0)
        assert dfw < 1e-4 and dbe < 1e-4, (name, dfw, dbe)
    for k in ('psf', 'psf_sum', 'fit'):
        assert np.all(np.isfinite(r[k])), (name, k)
    _FRESH[name] = r
    return r


# ---- predecessors: fn(api, ctx, name), each restores the options it changed

def _npl(name):
    return CHECKED[name][4]


def p1_short_l0(api, ctx, name):
    ctx.reconstruct(LB, SEE, GL, np.array([22.0, 5.0, 27.0]), THREE, H, npsflin=_npl(name))


def p2_stage_a0(api, ctx, name):
    ctx.set_option('stage_a', 0)
    try:
        ctx.reconstruct(LB, SEE, GL, L0, THREE, H, npsflin=_npl(name))
    finally:
        ctx.set_option('stage_a', 1)


def _with_option(key, value, default):
    """A predecessor that runs the rows under another option (the per-wavelength tables it caches differ), then
    sets the option back."""
    def pred(api, ctx, name):
        ctx.set_option(key, value)
        try:
            ctx.reconstruct(LB, SEE, GL, L0, THREE, H, npsflin=_npl(name))
        finally:
            ctx.set_option(key, default)
    return pred


def _overflowing_psd(ctx, name):
    """A realistic PSD scaled until the sums of its transform overflow fp64: finite input, non-finite D."""
    psd = ctx.simul_psd(0.9, 0.6, 22.0, npsflin=_npl(name))
    psd = psd * (1.0e307 / psd.max())
    assert np.all(np.isfinite(psd))
    return psd


def p4_overflow(api, ctx, name):
    ctx.psf_from_psd(_overflowing_psd(ctx, name), LB)


def p4_overflow_4dir(api, ctx, name):
    """P4 with four directions: the non-finite plane reaches past the lines of a one-direction call, into what the
    padding lines behind its D read (the full-size form at 256^2 reads them too)."""
    psd = ctx.simul_psd(0.9, 0.6, 22.0, npsflin=2)
    ctx.psf_from_psd(psd * (1.0e307 / psd.max()), LB)


def p5_nan_pixel(api, ctx, name):
    psd = ctx.simul_psd(0.9, 0.6, 22.0, npsflin=_npl(name))
    psd[0, 3, 5] = np.nan
    with pytest.raises(api.MpsfrError):
        ctx.psf_from_psd(psd, LB)


def p6_more_tasks(api, ctx, name):
    n = 8
    ctx.reconstruct(LB, np.full(n, 0.8), np.full(n, 0.5), np.full(n, 18.0), np.zeros(n, np.uint8), H,
                    npsflin=_npl(name))


def p6_chunk1(api, ctx, name):
    ctx.set_option('chunk_tasks', 1)
    try:
        ctx.reconstruct(LB, SEE, GL, L0, THREE, H, npsflin=_npl(name))
    finally:
        ctx.set_option('chunk_tasks', 0)


def p6_npsflin3(api, ctx, name):
    ctx.reconstruct(LB, SEE[:2], GL[:2], L0[:2], THREE[:2], H, npsflin=3)


def p6_npsflin3_full(api, ctx, name):
    ctx.reconstruct(LB, SEE[:2], GL[:2], np.array([5.0, 20.0]), THREE[:2], H, npsflin=3)


def p7_profile(api, ctx, name):
    ctx.reconstruct_profile(LB, SEE, GL, L0, np.array([0.5, 0.3, 0.2]), np.array([0.0, 3000.0, 12000.0]),
                            np.array([8.0, 15.0, 25.0]), np.array([0.3, 1.2, 2.5]), THREE)


def p7_field(api, ctx, name):
    ctx.reconstruct_field(LB, SEE, GL, L0, THREE, H, [(10.0, 10.0), (-20.0, 5.0), (0.0, -30.0)])


def p7_band(api, ctx, name):
    ctx.reconstruct_band(LB, api.band_weights(LB, [(500.0, 700.0)]), SEE, GL, L0, THREE, H, npsflin=2)


def p7_convolve(api, ctx, name):
    rng = np.random.default_rng(5)
    ctx.convolve_stamps(LB, SEE, GL, L0, rng.uniform(0.0, 1.0e3, (SEE.size, LB.size, 40, 40)))


def p7_fit_ell_device(api, ctx, name):
    import torch
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(6)
    st = torch.tensor(rng.uniform(0.0, 1.0, (5, 40, 40)), dtype=torch.float64, device=dev)
    fe = torch.empty((5, api.NFIT_ELL), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_stamps_elliptical_device(5, st.data_ptr(), fe.data_ptr())
    ctx.sync()
    torch.cuda.synchronize()


def p8_fit_device(api, ctx, name):
    import torch
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(8)
    st = torch.tensor(rng.uniform(0.0, 1.0, (5, 40, 40)), dtype=torch.float64, device=dev)
    ft = torch.empty((5, api.NFIT), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fit_stamps_device(5, st.data_ptr(), ft.data_ptr())
    ctx.sync()
    torch.cuda.synchronize()


def p7_psd_to_psf(api, ctx, name):
    psd = ctx.simul_psd(0.9, 0.6, 22.0)
    n = ctx.dim // 4
    y, x = np.mgrid[:n, :n] - (n - 1) / 2
    pup = (np.hypot(x, y) <= n / 2).astype(float)
    ctx.psd_to_psf(psd, pup, 8.0, LB * 1e-9)


def p10_psd_to_psf_small(api, ctx, name):
    pup = PR.rand_pupil(61)
    ctx.psd_to_psf(PR.scaled_psd(PR.asym_psd(ctx.dim), pup, 8.0, 500e-9, 128, 10.0), pup, 8.0, np.array([500e-9]),
                   dimnum=128)


def p10_psd_to_psf_nan(api, ctx, name):
    """include/mpsfr.h: a PSD with a NaN is not refused, its planes are NaN in every pixel."""
    a = _p2p_inputs()
    psd = PR.scaled_psd(PR.asym_psd(ctx.dim), a['pup'], 8.0, 500e-9, a['dimnum'], 10.0)
    psd[200, 13] = np.nan
    out = ctx.psd_to_psf(psd, a['pup'], 8.0, a['lbda'], phase_static=a['phase'], dimnum=a['dimnum'])[0]
    assert np.isnan(out).all()


def p9_stamp_frame_cube_calls(api, ctx, name):
    import stamp_history_cases as S
    S.run_all(api, ctx)


PRED = {
    'P1_l0_5m': p1_short_l0,
    'P2_stage_a0': p2_stage_a0,
    'P2_otf_mfma0': _with_option('otf_mfma', 0, 1),
    'P2_mf_kernel1': _with_option('mf_kernel', 1, 2),
    'P2_fft_conv0': _with_option('fft_conv', 0, 1),
    'P2_support_skip0': _with_option('support_skip', 0, 1),
    'P4_psd_overflow': p4_overflow,
    'P4_psd_overflow_4dir': p4_overflow_4dir,
    'P5_psd_nan_pixel': p5_nan_pixel,
    'P6_more_tasks_per_chunk': p6_more_tasks,
    'P6_chunk_tasks_1': p6_chunk1,
    'P6_npsflin3': p6_npsflin3,
    'P6_npsflin3_full_size': p6_npsflin3_full,
    'P7_profile': p7_profile,
    'P7_field': p7_field,
    'P7_band': p7_band,
    'P7_convolve_stamps': p7_convolve,
    'P7_fit_ell_device': p7_fit_ell_device,
    'P7_psd_to_psf': p7_psd_to_psf,
    'P8_fit_device': p8_fit_device,
    'P9_stamp_frame_cube_calls': p9_stamp_frame_cube_calls,
    'P10_psd_to_psf_small': p10_psd_to_psf_small,
    'P10_psd_to_psf_nan': p10_psd_to_psf_nan,
}

CASES = ([(p, 'd512') for p in PRED]
         + [(p, c) for p in ('P1_l0_5m', 'P4_psd_overflow') for c in CHECKED if c != 'd512']
         + [('P4_psd_overflow_4dir', c) for c in ('d256', 'd512_f64')]
         + [('P9_stamp_frame_cube_calls', c) for c in ('d512_f64', 'band512')]
         # reconstruct_profile and psd_to_psf as checked calls: P1 and P4 come with the line above; the stage-A form
         # by option, the refused PSD, the layout shifts, the other entry points and the stamp, frame and cube calls
         + [(p, c) for c in ('profile512', 'profile512_f64', 'psd2psf512', 'psd2psf512_f64')
            for p in ('P2_stage_a0', 'P5_psd_nan_pixel', 'P6_more_tasks_per_chunk', 'P6_npsflin3', 'P7_profile',
                      'P7_field', 'P7_band', 'P7_convolve_stamps', 'P7_psd_to_psf', 'P9_stamp_frame_cube_calls',
                      'P10_psd_to_psf_small', 'P10_psd_to_psf_nan')])


@pytest.mark.parametrize('pred,checked', CASES)
def test_checked_call_after_predecessor_equals_fresh(api, pred, checked):
    want = _fresh(api, checked)
    ctx = _context(api, checked)
    _run(api, ctx, checked)
    PRED[pred](api, ctx, checked)
    got = _run(api, ctx, checked)
    ctx.close()
    assert _same(got, want), (pred, checked, _diff(got, want))


def test_reverse_layout_shifts(api):
    """A one-direction call first, then the wider layouts (and the direction count back)."""
    ctx = _context(api, 'd512')
    ctx.reconstruct(LB, SEE[:1], GL[:1], L0[:1], THREE[:1], H)
    p6_npsflin3(api, ctx, 'd512')
    ctx.reconstruct(LB, SEE[:1], GL[:1], L0[:1], THREE[:1], H)
    p6_more_tasks(api, ctx, 'd512')
    got = _run(api, ctx, 'd512')
    ctx.close()
    assert _same(got, _fresh(api, 'd512')), _diff(got, _fresh(api, 'd512'))


@pytest.mark.parametrize('pred', ['P1_l0_5m', 'P4_psd_overflow'])
def test_two_lanes_both_clean(api, pred):
    """streams = 2: the predecessor on both lanes (P1 as two asynchronous calls; psf_from_psd is synchronous and
    takes lane 0), then two asynchronous checked calls, one per lane."""
    def run(with_pred):
        ctx = _context(api, 'd512')
        ctx.set_option('streams', 2)
        [q.wait() for q in (_run(api, ctx, 'd512', _async=True), _run(api, ctx, 'd512', _async=True))]
        if with_pred:
            if pred == 'P1_l0_5m':
                a = ctx.reconstruct_async(LB, SEE, GL, np.array([22.0, 5.0, 27.0]), THREE, H)
                b = ctx.reconstruct_async(LB, SEE, GL, np.array([5.0, 13.0, 27.0]), THREE, H)
                a.wait()
                b.wait()
            else:
                p4_overflow(api, ctx, 'd512')
        p = [_run(api, ctx, 'd512', _async=True), _run(api, ctx, 'd512', l0=L0[::-1].copy(), _async=True)]
        out = [q.wait() for q in p]
        ctx.close()
        return out
    want, got = run(False), run(True)
    assert _same(want[0], _fresh(api, 'd512'))
    for k in range(2):
        assert _same(got[k], want[k]), (pred, k, _diff(got[k], want[k]))


def test_device_fits_wait_for_the_lanes(api):
    """include/mpsfr.h: a device-buffer fit is queued after every call queued so far on its context.  streams = 2, a
    device-output reconstruct_device into tensors filled with NaN, and with no synchronisation in between the device
    fit of the `psf` tensor: its rows equal, bit for bit, the host-buffer fit of the stamps read back after the sync
    (both run the same kernel on the same doubles).  The circular fit, and the elliptical one as a control.  A race
    cannot be made to fail reliably, so this pins the contract: it does not demonstrate that a fit without the wait
    reads unfinished stamps."""
    import torch
    dev = torch.device('cuda:0')
    ctx = _context(api, 'd512')
    ctx.set_option('streams', 2)
    n = SEE.size * LB.size
    psf = torch.empty((SEE.size, LB.size, 40, 40), dtype=torch.float64, device=dev)
    psum = torch.empty((LB.size, 40, 40), dtype=torch.float64, device=dev)
    fit = torch.empty((SEE.size, LB.size, api.NFIT), dtype=torch.float64, device=dev)
    for device_fit, host_fit, nfit in ((ctx.fit_stamps_device, ctx.fit_stamps, api.NFIT),
                                       (ctx.fit_stamps_elliptical_device, ctx.fit_stamps_elliptical, api.NFIT_ELL)):
        rows = torch.empty((n, nfit), dtype=torch.float64, device=dev)
        psf.fill_(float('nan'))
        torch.cuda.synchronize()
        ctx.reconstruct_device(LB, SEE, GL, L0, THREE, H, 12.0, 1, None, psf.data_ptr(), psum.data_ptr(),
                               fit.data_ptr())
        device_fit(n, psf.data_ptr(), rows.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        stamps = psf.cpu().numpy().reshape(n, 40, 40)
        assert np.all(np.isfinite(stamps))
        want = host_fit(stamps)
        got = rows.cpu().numpy()
        assert np.array_equal(got, want), (nfit, int(np.sum(got != want)))
    # the circular rows are those of the reconstruct's own fit
    assert np.array_equal(fit.cpu().numpy().reshape(n, api.NFIT), ctx.fit_stamps(stamps))
    ctx.close()


# ---- the refusals of the shared grid-or-positions check, made of the C entry points directly (the Python wrappers
# refuse the same arguments before the library is reached)
E_INVALID = -1
REFUSALS = ['npos_out_of_range', 'npsflin_with_positions', 'null_positions', 'non_finite', 'beyond_60_arcsec']
ENTRIES = ['field', 'band', 'profile', 'simul_psd_profile']


def _refused_call(api, ctx, entry, refusal):
    """The return code of `entry` called with positions that `refusal` makes invalid (all else valid)."""
    from muse_psfr_amd._lib import _dptr, _u8ptr
    pos = np.array(POS, dtype=np.float64)
    npos, npsflin = 2, 0
    if refusal == 'npos_out_of_range':
        pos, npos = np.zeros((26, 2)), 26
    elif refusal == 'npsflin_with_positions':
        npsflin = 1
    elif refusal == 'non_finite':
        pos[1, 0] = np.nan
    elif refusal == 'beyond_60_arcsec':
        pos[1, 1] = -60.5
    ppos = None if refusal == 'null_positions' else _dptr(pos)
    hh = np.array(H, dtype=np.float64)
    lay = [np.array(v) for v in ([0.0, 3000.0, 12000.0], [8.0, 15.0, 25.0], [0.3, 1.2, 2.5])]
    cn2 = np.tile([0.5, 0.3, 0.2], (SEE.size, 1))
    rows = (SEE.size, _dptr(SEE), _dptr(GL), _dptr(L0), _u8ptr(THREE))
    nt, nl, lib = SEE.size, LB.size, ctx.lib
    outs = [np.empty((nt, npos, nl, 40, 40)), np.empty((npos, nl, 40, 40)), np.empty((nt, npos, nl, api.NFIT))]
    vouts = [a.ctypes.data for a in outs]
    if entry == 'field':
        return lib.mpsfr_reconstruct_field(ctx._h, *rows, _dptr(hh), 12.0, npos, ppos, nl, _dptr(LB), None, None,
                                           *vouts, 0)
    if entry == 'band':
        w = np.ascontiguousarray(api.band_weights(LB, BANDS), dtype=np.float64)
        return lib.mpsfr_reconstruct_band(ctx._h, *rows, _dptr(hh), 12.0, npsflin, npos, ppos, nl, _dptr(LB),
                                          w.shape[0], _dptr(w), None, None, *vouts, 0)
    if entry == 'profile':
        return lib.mpsfr_reconstruct_profile(ctx._h, *rows, 3, _dptr(lay[0]), _dptr(lay[1]), _dptr(lay[2]), _dptr(cn2),
                                             npsflin, npos, ppos, nl, _dptr(LB), None, None, *vouts, 0)
    psd = np.empty((npos, ctx.dim, ctx.dim))
    return lib.mpsfr_simul_psd_profile(ctx._h, 0.9, 22.0, 0, 3, _dptr(lay[0]), _dptr(lay[1]), _dptr(lay[2]),
                                       _dptr(cn2[:1].copy()), npsflin, npos, ppos, None, None, _dptr(psd))


@pytest.mark.parametrize('entry,refusal', [(e, r) for e in ENTRIES for r in REFUSALS
                                           if (e, r) != ('field', 'npsflin_with_positions')])   # (it takes no npsflin)
def test_position_refusals_leave_the_context_usable(api, entry, refusal):
    want = _fresh(api, 'd512')
    ctx = _context(api, 'd512')
    _run(api, ctx, 'd512')
    assert _refused_call(api, ctx, entry, refusal) == E_INVALID
    assert ctx.lib.mpsfr_last_error()
    got = _run(api, ctx, 'd512')
    ctx.close()
    assert _same(got, want), (entry, refusal, _diff(got, want))


def test_dphi0_after_overflow_matches_fresh_and_header(api):
    """debug_fetch('dphi0') after P4 and a series call equals the fresh context's plane, bit for bit; on the pieces of
    a line that lie wholly outside the telescope OTF's support (the pieces the series form skips) it holds zero
    (include/mpsfr.h, "support_skip")."""
    dim = 512
    n, h1 = SEE.size, dim // 2 + 1

    def plane(with_pred):
        ctx = _context(api, 'd512')
        _run(api, ctx, 'd512')
        if with_pred:
            p4_overflow(api, ctx, 'd512')
        _run(api, ctx, 'd512')
        d = ctx.debug_fetch('dphi0', (n, h1, dim))
        tel = ctx.debug_fetch('tel', (h1, dim))
        ctx.close()
        return d, tel
    fresh, tel = plane(False)
    after, _ = plane(True)
    assert np.array_equal(after, fresh), int(np.sum(after != fresh))
    L = 32                                   # (columns of a piece at 512^2: series_lanes in stage_a2.hip)
    skipped = ~(tel.reshape(h1, dim // L, L) > 0).any(axis=2)
    assert skipped.any()
    pieces = after.reshape(n, h1, dim // L, L)
    assert np.all(pieces[:, skipped] == 0.0)
    assert np.all(np.isfinite(after))


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_psf_from_psd_refuses_non_finite(api, bad):
    ctx = _context(api, 'd512')
    _run(api, ctx, 'd512')
    psd = ctx.simul_psd(0.9, 0.6, 22.0)
    psd[0, 100, 200] = bad
    with pytest.raises(api.MpsfrError):
        ctx.psf_from_psd(psd, LB)
    # the refusal queued nothing: the context goes on as a fresh one
    got = _run(api, ctx, 'd512')
    ctx.close()
    assert _same(got, _fresh(api, 'd512'))


def _clears(ctx):
    return int(ctx.debug_fetch('d0t_clears', (1,))[0])


def test_clearing_path_only_after_a_writer(api):
    """The steady path -- the bench workload: 100 rows x 35 wavelengths at 512^2, L0 in 9-29 m, device and
    asynchronous calls on both lanes -- never clears D0t; a call that wrote outside the series form's part makes the
    next series call on its lane clear it once."""
    import torch
    ps = api.grid_pixscale(512)
    see, gl, l0 = api.synthetic_rows(100)
    three = np.zeros(100, np.uint8)
    lb = np.linspace(465.0, 930.0, 35)
    ctx = api.Context(dim=512, pixscale=ps, precision='mixed')
    dev = torch.device('cuda:0')
    psf = torch.empty((100, 35, 40, 40), dtype=torch.float64, device=dev)
    psum = torch.empty((35, 40, 40), dtype=torch.float64, device=dev)
    fit = torch.empty((100, 35, api.NFIT), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for _ in range(6):
        ctx.reconstruct_device(lb, see, gl, l0, three, H, 12.0, 1, None, psf.data_ptr(), psum.data_ptr(),
                               fit.data_ptr())
    ctx.sync()
    pend = [ctx.reconstruct_async(lb, see, gl, l0, three, H, want_psf=False) for _ in range(4)]
    [p.wait() for p in pend]
    ctx.reconstruct(lb, see, gl, l0, three, H, want_psf=False)
    assert _clears(ctx) == 0
    torch.cuda.synchronize()
    ctx.close()

    ctx = _context(api, 'd512')
    _run(api, ctx, 'd512')
    _run(api, ctx, 'd512')
    assert _clears(ctx) == 0
    p9_stamp_frame_cube_calls(api, ctx, 'd512')          # (no stamp, frame or cube call writes D0t)
    assert _same(_run(api, ctx, 'd512'), _fresh(api, 'd512'))
    assert _clears(ctx) == 0
    steps = [(p4_overflow, 1), (None, 1), (p1_short_l0, 2), (p2_stage_a0, 3), (None, 3)]
    for pred, want in steps:
        if pred is not None:
            pred(api, ctx, 'd512')
        got = _run(api, ctx, 'd512')
        assert _same(got, _fresh(api, 'd512'))
        assert _clears(ctx) == want, (pred, _clears(ctx), want)
    ctx.set_option('support_skip', 0)
    _run(api, ctx, 'd512')
    ctx.set_option('support_skip', 1)
    assert _same(_run(api, ctx, 'd512'), _fresh(api, 'd512'))
    assert _clears(ctx) == 4
    ctx.close()
