"""GPU: field-resolved PSFs (mpsfr_reconstruct_field, compute_field_psf, the PSF_FIELD / FIT_FIELD HDUs).

Tolerances are those of tests/test_gpu_parity.py (relative to the stamp maximum for stamps, absolute for the fit):
  f64 mode   : stamps 1e-9,  fwhm/beta 1e-6
  mixed mode : stamps 2e-5,  fwhm/beta 1e-4
Fits flagged MPSFR_FIT_ILL_CONDITIONED are checked on peak and centre only; on the 256^2 grid (the stamp narrower
than the PSF core) the stamps are checked and the fits are not, as in tests/test_gpu_parity.py.
"""
import ctypes as C

import numpy as np
import pytest

import psfr_oracle as O
from conftest import record_margin, H, rel_err

pytestmark = pytest.mark.gpu

TOL = {'f64': dict(stamp=1e-9, fit=1e-6), 'mixed': dict(stamp=2e-5, fit=1e-4)}


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


# ---- 1. one position at the centre is the existing call
@pytest.mark.parametrize('dim', [256, 512])
@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_centre_position_is_npsflin_1_bit_for_bit(api, dim, prec):
    ps = api.grid_pixscale(dim)
    lb = np.array([465.0, 600.0, 750.0, 930.0])
    see, gl, l0, three = np.array([1.0, 0.6]), np.array([0.7, 0.4]), np.array([25.0, 12.0]), np.array([0, 1])
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    for l0s in (l0, np.array([25.0, 5.0])):          # (L0 = 5 m: the full-size stage A)
        r = ctx.reconstruct(lb, see, gl, l0s, three, H, npsflin=1)
        f = ctx.reconstruct_field(lb, see, gl, l0s, three, H, [(0.0, 0.0)])
        assert _same(f['psf'][:, 0], r['psf'])
        assert _same(f['psf_sum'][0], r['psf_sum'])
        assert _same(f['fit'][:, 0], r['fit'])
    ctx.close()


# ---- 2 / 3. against the oracle
def _oracle_field(api, dim, prec, lb, cases, pos, npl, monkeypatch):
    ps = api.grid_pixscale(dim)
    monkeypatch.setattr(O, 'eval_directions', lambda npsflin, field_size=60: np.asarray(pos, dtype=float).T)
    tabs = {g: O.ao_tables(H, bool(g), npl, exact_masks=True) for g in (0, 1)}
    see, gl, l0, three = (np.array([c[k] for c in cases]) for k in range(4))
    ctx = api.Context(dim=dim, pixscale=ps, precision=prec)
    r = ctx.reconstruct_field(lb, see, gl, l0, three, H, pos)
    ctx.close()
    from muse_psfr_amd import FIT_ILL_CONDITIONED
    worst = dict(stamp=0.0, fwhm_arcsec=0.0, beta=0.0)
    for k, (s, g_, l, th) in enumerate(cases):
        psd = O.residual_psd([g_, 1 - g_], H, s, l, npl, dim, bool(th), tables=tabs[th])
        assert psd.shape[0] == len(pos)
        for d in range(len(pos)):
            ofin = O.convolve_final_psf(lb, s, g_, l, O.psf_stamps_refshaped(psd[d], lb, 40, ps), ps)
            e = rel_err(r['psf'][k, d], ofin)
            worst['stamp'] = max(worst['stamp'], e)
            assert e < TOL[prec]['stamp'], (k, d, e)
            if dim < 512:       # (as in test_gpu_parity: the stamp is narrower than the PSF core, the fit ill-posed)
                continue
            ofit = O.fit_psf_cube(ofin, ps)
            fit = r['fit'][k, d]
            ill = (fit[:, 14].astype(int) & FIT_ILL_CONDITIONED) != 0
            # (a flagged fit is held on peak and centre only)
            assert np.abs(fit[:, 1:3] - ofit[:, 1:3]).max() < 1e-3
            assert np.all(np.abs(fit[:, 0] / ofit[:, 0] - 1) < 1e-3)
            well = ~ill
            if well.any():
                dw = np.abs(fit[well, 5] * ps - ofit[well, 3]).max()
                db = np.abs(fit[well, 4] - ofit[well, 4]).max()
                worst['fwhm_arcsec'] = max(worst['fwhm_arcsec'], dw)
                worst['beta'] = max(worst['beta'], db)
                assert dw < TOL[prec]['fit'] and db < TOL[prec]['fit'], (k, d, dw, db)
    np.testing.assert_allclose(r['psf_sum'], r['psf'].sum(axis=0), rtol=1e-12, atol=1e-15)
    return worst


@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_grid_against_the_oracle(api, prec, monkeypatch):
    lb = np.array([465.0, 560.0, 650.0, 800.0, 930.0])
    cases = [(1.0, 0.7, 25.0, 0), (1.5, 0.3, 10.0, 1), (0.6, 0.9, 28.0, 0)]
    pos = O.eval_directions(3).T
    w = _oracle_field(api, 256, prec, lb, cases, pos, 3, monkeypatch)
    record_margin('field_grid_256_%s' % prec, **w)


@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_arbitrary_positions_against_the_oracle(api, prec, monkeypatch):
    lb = np.array([480.0, 700.0, 920.0])
    cases = [(0.9, 0.6, 20.0, 0), (1.3, 0.4, 15.0, 1)]
    pos = [(12.5, -7.0), (-29.0, 3.0), (0.0, 0.0), (21.2, 21.2)]
    w = _oracle_field(api, 512, prec, lb, cases, pos, 2, monkeypatch)
    record_margin('field_positions_512_%s' % prec, **w)


# ---- 4. positions are independent
def test_positions_are_independent(api):
    dim = 512
    ps = api.grid_pixscale(dim)
    lb = np.array([480.0, 620.0, 780.0, 920.0])
    see, gl, l0, three = np.array([1.0, 0.7, 1.4]), np.array([0.7, 0.5, 0.3]), np.array([25.0, 15.0, 20.0]), \
        np.array([0, 1, 0])
    pos = O.eval_directions(3).T + np.array([1.5, -2.0])
    ctx = api.Context(dim=dim, pixscale=ps, precision='mixed')
    full = ctx.reconstruct_field(lb, see, gl, l0, three, H, pos)
    for d in range(len(pos)):
        one = ctx.reconstruct_field(lb, see, gl, l0, three, H, pos[d:d + 1])
        assert _same(one['psf'][:, 0], full['psf'][:, d]), d
        assert _same(one['fit'][:, 0], full['fit'][:, d]), d
        peak = full['psf_sum'][d].max()
        assert np.abs(one['psf_sum'][0] - full['psf_sum'][d]).max() <= 1e-12 * peak
    rev = ctx.reconstruct_field(lb, see, gl, l0, three, H, pos[::-1])
    assert _same(rev['psf'], full['psf'][:, ::-1])
    assert _same(rev['fit'], full['fit'][:, ::-1])
    # the C entry refuses 26 positions (and touches nothing)
    p26 = np.zeros((26, 2))
    out = np.full((1, 26, 1, 40, 40), 7.0)
    d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    one = np.ones(1)
    rc = ctx.lib.mpsfr_reconstruct_field(ctx._h, 1, d(one), d(one * 0.5), d(one * 20), None,
                                         d(np.array([100.0, 10000.0])), 12.5, 26, d(p26), 1,
                                         d(np.array([600.0])), None, None, out.ctypes.data_as(C.c_void_p),
                                         None, None, 0)
    assert rc == -1 and np.all(out == 7.0)
    ctx.close()
    # 30 positions through Python equal the same positions called in groups
    rng = np.random.default_rng(11)
    p30 = np.round(rng.uniform(-40, 40, (30, 2)), 2)
    t, psf = api.compute_field_psf(lb, 1.1, 0.6, 18.0, positions=p30, verbose=False, dim=dim, pixscale=ps,
                                   cutoff_masks='exact')
    assert psf.shape == (30, lb.size, 40, 40) and len(t) == 30 * lb.size
    from muse_psfr_amd.psfrec import get_context
    c2 = get_context(dim, ps, 40, 'mixed', 0)
    for a, b in ((0, 25), (25, 30)):
        g = c2.reconstruct_field(lb, [1.1], [0.6], [18.0], [0], H, p30[a:b])
        assert _same(g['psf'][0], psf[a:b])
        np.testing.assert_array_equal(np.asarray(t['n']).reshape(30, -1)[a:b], g['fit'][0][..., 4])


# ---- 5. output modes
def test_device_ticket_and_async_outputs(api):
    import torch
    dim = 256
    ps = api.grid_pixscale(dim)
    lb = np.array([500.0, 700.0, 900.0])
    see, gl, l0, three = np.array([1.0, 0.8]), np.array([0.7, 0.5]), np.array([25.0, 20.0]), np.array([0, 1])
    pos = O.eval_directions(2).T
    ctx = api.Context(dim=dim, pixscale=ps, precision='mixed')
    ref = ctx.reconstruct_field(lb, see, gl, l0, three, H, pos)
    dev = torch.device('cuda:0')
    tp = torch.empty(ref['psf'].shape, dtype=torch.float64, device=dev)
    ts = torch.empty(ref['psf_sum'].shape, dtype=torch.float64, device=dev)
    tf = torch.empty(ref['fit'].shape, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.reconstruct_field_device(lb, see, gl, l0, three, H, 12.0, pos, None, tp.data_ptr(), ts.data_ptr(),
                                 tf.data_ptr())
    ctx.sync()
    assert _same(tp.cpu().numpy(), ref['psf'])
    assert _same(ts.cpu().numpy(), ref['psf_sum'])
    assert _same(tf.cpu().numpy(), ref['fit'])
    tk = ctx.reconstruct_field_async(lb, see, gl, l0, three, H, pos).wait()
    for k in ('psf', 'psf_sum', 'fit'):
        assert _same(tk[k], ref[k]), k
    # an asynchronous field call between two asynchronous reconstruct calls
    r1 = ctx.reconstruct(lb, see, gl, l0, three, H, npsflin=1)
    r3 = ctx.reconstruct(lb, see[::-1], gl[::-1], l0[::-1], three[::-1], H, npsflin=3)
    a1 = ctx.reconstruct_async(lb, see, gl, l0, three, H, npsflin=1)
    a2 = ctx.reconstruct_field_async(lb, see, gl, l0, three, H, pos)
    a3 = ctx.reconstruct_async(lb, see[::-1], gl[::-1], l0[::-1], three[::-1], H, npsflin=3)
    g3, g2, g1 = a3.wait(), a2.wait(), a1.wait()
    for k in ('psf', 'psf_sum', 'fit'):
        assert _same(g1[k], r1[k]) and _same(g2[k], ref[k]) and _same(g3[k], r3[k]), k
    ctx.close()


# ---- 6. no interference
@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_field_calls_leave_reconstruct_unchanged(api, prec):
    dim = 512
    ps = api.grid_pixscale(dim)
    lb = np.array([480.0, 700.0, 920.0])
    see, gl, l0, three = np.array([1.0, 0.8, 1.2]), np.array([0.7, 0.5, 0.6]), np.array([25.0, 20.0, 12.0]), \
        np.array([0, 1, 0])
    a = api.Context(dim=dim, pixscale=ps, precision=prec)
    a.reconstruct_field(lb, see, gl, l0, three, H, O.eval_directions(3).T)
    a.reconstruct_field(lb, see, gl, np.array([25.0, 5.0, 12.0]), three, H, [(10.0, -20.0), (0.0, 0.0)])
    ra = a.reconstruct(lb, see, gl, l0, three, H, npsflin=1)
    ra3 = a.reconstruct(lb, see, gl, l0, three, H, npsflin=3)
    a.close()
    b = api.Context(dim=dim, pixscale=ps, precision=prec)
    rb = b.reconstruct(lb, see, gl, l0, three, H, npsflin=1)
    b.close()
    b = api.Context(dim=dim, pixscale=ps, precision=prec)
    rb3 = b.reconstruct(lb, see, gl, l0, three, H, npsflin=3)
    b.close()
    for k in ('psf', 'psf_sum', 'fit'):
        assert _same(ra[k], rb[k]) and _same(ra3[k], rb3[k]), k


# ---- 7. SPARTA
def _sparta(api, nlines):
    from muse_psfr_amd import _minifits
    hdu = api.create_sparta_table(nlines=nlines, seeing=1.0, L0=20, GL=0.6)
    d = hdu.data
    rng = np.random.default_rng(2)
    for k in range(1, 5):               # rows that differ
        d['LGS%d_SEEING' % k] = 0.7 + 0.6 * rng.random(nlines)
        d['LGS%d_TUR_GND' % k] = 0.4 + 0.5 * rng.random(nlines)
        d['LGS%d_L0' % k] = 12 + 15 * rng.random(nlines)
    d['LGS4_L0'][0] = 50.0              # one row in three-laser mode
    return _minifits.HDUList([_minifits.PrimaryHDU(), hdu])


def test_sparta_field_hdus(api, tmp_path):
    from muse_psfr_amd import psfrec
    dim = 256
    ps = api.grid_pixscale(dim)
    kw = dict(nl=4, npsflin=3, dim=dim, pixscale=ps, device=0, verbose=False)
    base = api.compute_psf_from_sparta(_sparta(api, 3), **kw)
    out = api.compute_psf_from_sparta(_sparta(api, 3), field_positions='grid', **kw)
    names = [h.name for h in out]
    assert names[:len(base)] == [h.name for h in base] and names[len(base):] == ['PSF_FIELD', 'FIT_FIELD']
    for hb, ho in zip(base, out):
        if hb.data is not None:
            assert np.asarray(hb.data).tobytes() == np.asarray(ho.data).tobytes(), hb.name
    field = np.asarray(out['PSF_FIELD'].data)
    assert field.shape == (9, 4, 40, 40)
    # PSF_FIELD = the row mean of compute_field_psf's stamps
    fr = np.asarray(out['FIT_ROWS'].data)
    stats = np.stack([fr['SEEING'], fr['GL'], fr['L0']], axis=1)[::4]
    lbda = np.asarray(out['FIT_MEAN'].data['lbda'])
    three = [True, False, False]
    stamps = [api.compute_field_psf(lbda, s, g, l, npsflin=3, three_lgs_mode=t, verbose=False, dim=dim,
                                    pixscale=ps)[1] for (s, g, l), t in zip(stats, three)]
    mean = np.mean(stamps, axis=0)
    assert np.abs(field - mean).max() <= 1e-14 * np.abs(mean).max() * 10
    # FIT_FIELD = fit_stamps of PSF_FIELD
    ctx = psfrec.get_context(dim, ps, 40, 'mixed', 0)
    want = psfrec._field_columns(lbda, api.direction_perf(3).T, ctx.fit_stamps(field.reshape(-1, 40, 40)), ps)
    t = out['FIT_FIELD'].data
    for k in ('dir_idx', 'x', 'y', 'lbda', 'fwhm', 'n', 'peak', 'center'):
        np.testing.assert_array_equal(np.asarray(t[k]), want[k])
    assert out['FIT_FIELD'].header['SEEING'] == out['FIT_MEAN'].header['SEEING']
    # two contexts on one device
    two = api.compute_psf_from_sparta(_sparta(api, 3), field_positions='grid', devices=[0, 0],
                                      **{k: v for k, v in kw.items() if k != 'device'})
    f2 = np.asarray(two['PSF_FIELD'].data)
    assert np.abs(f2 - field).max() <= 1e-14 * np.abs(field).max()
    # the CLI
    from muse_psfr_amd import cli, _minifits
    path = str(tmp_path / 'field.fits')
    cli.main(['--values', '1.0,0.7,25', '--field', '3', '-o', path, '--logfile', str(tmp_path / 'log.txt')])
    back = _minifits.open(path)
    assert np.asarray(back['PSF_FIELD'].data).shape == (9, 3, 40, 40)
    assert len(np.asarray(back['FIT_FIELD'].data['x'])) == 27
