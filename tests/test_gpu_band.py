"""GPU: band-integrated PSFs (mpsfr_reconstruct_band, compute_band_psf, the FIT_BAND_ROWS / PSF_BAND / FIT_BAND HDUs).

A band stamp is sum_l w^_bl x the per-wavelength stamp, so every check compares with a NumPy reduction of stamps the
reference (the g5 fixture) or the per-wavelength call produced.  Tolerances, relative to the stamp maximum:
  against the reference's stamps : 2e-5 per row, 1e-5 for the row mean (those of tests/test_gpu_parity.py)
  against the per-wavelength call: f64 1e-12, mixed 1e-6 (mixed reduces its float stamps); fits of the same band
                                   within 1e-6 (f64) / 1e-4 (mixed) on FWHM and n
"""
import ctypes as C

import numpy as np
import pytest

from conftest import H, rel_err, record_margin

pytestmark = pytest.mark.gpu

LB = np.array([480.0, 520.0, 560.0, 600.0, 640.0, 700.0, 760.0, 820.0, 880.0, 930.0])
SEE, GL, L0 = np.array([1.0, 0.7, 1.3]), np.array([0.7, 0.5, 0.4]), np.array([25.0, 15.0, 20.0])
THREE = np.array([0, 1, 0])
BAND_TOL = {'f64': dict(stamp=1e-12, fit=1e-6), 'mixed': dict(stamp=1e-6, fit=1e-4)}


@pytest.fixture(scope='module')
def api():
    import muse_psfr_amd
    return muse_psfr_amd


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _norm(w):
    w = np.asarray(w, dtype=float)
    return w / w.sum(axis=1, keepdims=True)


def _weights(lbda):
    sed = (np.array([400.0, 1000.0]), np.array([2.0, 0.5]))        # a falling f_lambda
    curve = (np.array([550.0, 650.0, 800.0]), np.array([0.0, 1.0, 0.2]))
    return _norm(np.vstack([np.ones((1, lbda.size)),
                            _band_w(lbda, [(lbda[2], lbda[6])], sed),
                            _band_w(lbda, [curve], sed)]))


def _band_w(lbda, bands, sed):
    from muse_psfr_amd import band_weights
    return band_weights(lbda, bands, sed)


def _reduce(w, psf):
    """NumPy band of stamps (..., nl, 40, 40) with normalised weights (nband, nl)."""
    return np.einsum('bl,...lij->...bij', w, psf)


# ---- 1. against the reference's stamps
def test_against_the_reference_stamps(api, golden, ref_masks):
    g = golden('g5_sparta18')
    lb = g['lbda']
    sed = (np.array([450.0, 950.0]), np.array([1.0, 3.0]))
    w = api.band_weights(lb, [(lb[0], lb[-1]), (600.0, 700.0), (lb[20], lb[30])], sed=sed)
    wn = _norm(w)
    ctx = api.Context(dim=1280, pixscale=0.2, precision='mixed')
    r = ctx.reconstruct_band(lb, w, g['seeing'], g['gl'], g['l0'], g['three'].astype(np.uint8), H, masks=ref_masks)
    ctx.close()
    e0 = rel_err(r['psf'][0], _reduce(wn, g['fin_row0']))
    e17 = rel_err(r['psf'][17], _reduce(wn, g['fin_row17']))
    em = rel_err(r['psf_sum'] / 18, _reduce(wn, g['psf_mean']))
    record_margin('band_g5_mixed', stamp=max(e0, e17), mean=em)
    assert e0 < 2e-5 and e17 < 2e-5, (e0, e17)
    assert em < 1e-5, em
    assert r['fit'].shape == (18, 3, api.NFIT) and np.all(np.isfinite(r['fit'][:, :, 5]))


# ---- 2. against the per-wavelength call
@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_against_the_per_wavelength_call(api, prec):
    ps = api.grid_pixscale(512)
    w = _weights(LB)
    ctx = api.Context(dim=512, pixscale=ps, precision=prec)
    ref = ctx.reconstruct(LB, SEE, GL, L0, THREE, H, npsflin=2)
    b = ctx.reconstruct_band(LB, w * 3.0, SEE, GL, L0, THREE, H, npsflin=2)
    nb = _reduce(w, ref['psf'])
    es = max(rel_err(b['psf'][t], nb[t]) for t in range(SEE.size))
    esum = rel_err(b['psf_sum'], nb.sum(axis=0))
    assert es < BAND_TOL[prec]['stamp'] and esum < BAND_TOL[prec]['stamp'], (es, esum)
    want = ctx.fit_stamps(nb.reshape(-1, 40, 40)).reshape(b['fit'].shape)
    dw = np.abs(b['fit'][..., 5] - want[..., 5]).max() * ps
    dn = np.abs(b['fit'][..., 4] - want[..., 4]).max()
    record_margin('band_vs_per_wavelength_%s' % prec, stamp=es, fwhm_arcsec=dw, beta=dn)
    assert dw < BAND_TOL[prec]['fit'] and dn < BAND_TOL[prec]['fit'], (dw, dn)
    assert np.all(b['fit'][..., 14] == want[..., 14])
    # the band is not the PSF at its mean wavelength: the white-light FWHM lies inside the per-wavelength range
    fw = ref['fit'][..., 5]
    assert np.all(b['fit'][:, 0, 5] > fw.min(axis=1)) and np.all(b['fit'][:, 0, 5] < fw.max(axis=1))
    ctx.close()


# ---- 3. exactness
@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_one_wavelength_band_and_power_of_two_scale(api, prec):
    ps = api.grid_pixscale(512)
    ctx = api.Context(dim=512, pixscale=ps, precision=prec)
    w = _weights(LB)
    a = ctx.reconstruct_band(LB, w, SEE, GL, L0, THREE, H)
    s = ctx.reconstruct_band(LB, w * 4.0, SEE, GL, L0, THREE, H)
    for k in ('psf', 'psf_sum', 'fit'):
        assert _same(a[k], s[k]), k
    if prec == 'f64':
        ref = ctx.reconstruct(LB, SEE, GL, L0, THREE, H)
        one = np.zeros((3, LB.size))
        for b, l in enumerate((0, 4, 9)):
            one[b, l] = 1.0
        o = ctx.reconstruct_band(LB, one, SEE, GL, L0, THREE, H)
        assert _same(o['psf'], ref['psf'][:, [0, 4, 9]])
        assert _same(o['fit'], ref['fit'][:, [0, 4, 9]])
    ctx.close()


# ---- 4. field positions
@pytest.mark.parametrize('prec', ['mixed', 'f64'])
def test_field_positions(api, prec):
    ps = api.grid_pixscale(512)
    w = _weights(LB)
    pos = [(12.5, -7.0), (-29.0, 3.0), (0.0, 0.0)]
    ctx = api.Context(dim=512, pixscale=ps, precision=prec)
    ref = ctx.reconstruct_field(LB, SEE, GL, L0, THREE, H, pos)
    b = ctx.reconstruct_band(LB, w, SEE, GL, L0, THREE, H, positions=pos)
    assert b['psf'].shape == (3, 3, 3, 40, 40) and b['psf_sum'].shape == (3, 3, 40, 40)
    assert b['fit'].shape[:3] == (3, 3, 3)
    nb = _reduce(w, ref['psf'])
    es = max(rel_err(b['psf'][t, d], nb[t, d]) for t in range(3) for d in range(3))
    esum = max(rel_err(b['psf_sum'][d], nb[:, d].sum(axis=0)) for d in range(3))
    assert es < BAND_TOL[prec]['stamp'] and esum < BAND_TOL[prec]['stamp'], (es, esum)
    want = ctx.fit_stamps(nb.reshape(-1, 40, 40)).reshape(b['fit'].shape)
    assert np.abs(b['fit'][..., 5] - want[..., 5]).max() * ps < BAND_TOL[prec]['fit']
    assert np.abs(b['fit'][..., 4] - want[..., 4]).max() < BAND_TOL[prec]['fit']
    c = ctx.reconstruct_band(LB, w, SEE, GL, L0, THREE, H, npsflin=None, positions=[(0.0, 0.0)])
    n1 = ctx.reconstruct_band(LB, w, SEE, GL, L0, THREE, H, npsflin=1)
    for k in ('psf', 'fit'):
        assert _same(c[k][:, 0], n1[k]), k
    assert _same(c['psf_sum'][0], n1['psf_sum'])
    ctx.close()


# ---- 5. pipeline: chunks, lanes, device outputs, tickets, interleaving
def test_pipeline_modes(api):
    import torch
    ps = api.grid_pixscale(512)
    n = 18
    see, gl, l0 = api.synthetic_rows(n, seed=5)
    three = (np.arange(n) % 5 == 0).astype(np.uint8)
    w = _weights(LB)
    ctx = api.Context(dim=512, pixscale=ps, precision='mixed')
    ref = ctx.reconstruct_band(LB, w, see, gl, l0, three, H)
    for opts in ({'chunk_tasks': 7}, {'chunk_tasks': 7, 'streams': 1}, {'chunk_tasks': 5, 'streams': 2}):
        c2 = api.Context(dim=512, pixscale=ps, precision='mixed')
        for k, v in opts.items():
            c2.set_option(k, v)
        r = c2.reconstruct_band(LB, w, see, gl, l0, three, H)
        assert _same(r['psf'], ref['psf']) and _same(r['fit'], ref['fit']), opts
        # (chunked sums: per-chunk and per-lane partial sums, another order of additions)
        np.testing.assert_allclose(r['psf_sum'], ref['psf_sum'], rtol=1e-13, atol=1e-14 * ref['psf_sum'].max(),
                                   err_msg=str(opts))
        c2.close()
    # on_device = 1 into torch tensors, then the elliptical fit of the band stamps on the device
    dev = torch.device('cuda:0')
    tp = torch.empty(ref['psf'].shape, dtype=torch.float64, device=dev)
    ts = torch.empty(ref['psf_sum'].shape, dtype=torch.float64, device=dev)
    tf = torch.empty(ref['fit'].shape, dtype=torch.float64, device=dev)
    te = torch.empty((n * 3, api.NFIT_ELL), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.reconstruct_band_device(LB, w, see, gl, l0, three, H, 12.0, 1, None, None, tp.data_ptr(), ts.data_ptr(),
                                tf.data_ptr())
    ctx.fit_stamps_elliptical_device(n * 3, tp.data_ptr(), te.data_ptr())
    ctx.sync()
    torch.cuda.synchronize()
    assert _same(tp.cpu().numpy(), ref['psf'])
    assert _same(ts.cpu().numpy(), ref['psf_sum'])
    assert _same(tf.cpu().numpy(), ref['fit'])
    assert _same(te.cpu().numpy(), ctx.fit_stamps_elliptical(ref['psf']))
    # on_device = 2: four calls in flight, band and per-wavelength calls interleaved
    r1 = ctx.reconstruct(LB, see, gl, l0, three, H)
    w2 = _weights(LB)[::-1].copy()
    ref2 = ctx.reconstruct_band(LB, w2, see, gl, l0, three, H)
    pend = [ctx.reconstruct_band_async(LB, w, see, gl, l0, three, H),
            ctx.reconstruct_async(LB, see, gl, l0, three, H),
            ctx.reconstruct_band_async(LB, w2, see, gl, l0, three, H),
            ctx.reconstruct_band_async(LB, w, see, gl, l0, three, H)]
    got = [p.wait() for p in pend[::-1]][::-1]
    for k in ('psf', 'psf_sum', 'fit'):
        assert _same(got[0][k], ref[k]) and _same(got[3][k], ref[k]), k
        assert _same(got[1][k], r1[k]) and _same(got[2][k], ref2[k]), k
    r1b = ctx.reconstruct(LB, see, gl, l0, three, H)
    for k in ('psf', 'psf_sum', 'fit'):
        assert _same(r1b[k], r1[k]), k
    ctx.close()


# ---- 6. refusals
def test_refusals_leave_the_context_as_new(api):
    ps = api.grid_pixscale(256)
    ctx = api.Context(dim=256, pixscale=ps, precision='mixed')
    lb = np.array([500.0, 700.0, 900.0])
    d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    one = np.ones(2)
    out = np.full((2, 17, 40, 40), 7.0)
    fit = np.full((2, 17, api.NFIT), 7.0)
    pos = np.zeros((1, 2))

    def call(nband, weights, npsflin=1, npos=0):
        return ctx.lib.mpsfr_reconstruct_band(
            ctx._h, 2, d(one), d(one * 0.5), d(one * 20), None, d(np.array([100.0, 10000.0])), 12.5, npsflin, npos,
            d(pos) if npos else None, 3, d(lb), nband, d(np.ascontiguousarray(weights, dtype=float)), None, None,
            out.ctypes.data_as(C.c_void_p), None, fit.ctypes.data_as(C.c_void_p), 0)
    good = np.ones((1, 3))
    assert call(0, good) == -1
    assert call(17, np.ones((17, 3))) == -1
    assert call(1, [[1.0, np.nan, 1.0]]) == -1
    assert call(1, [[1.0, -1.0, 1.0]]) == -1
    assert call(2, [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]) == -1
    assert call(1, [[np.inf, 1.0, 1.0]]) == -1
    assert call(1, good, npsflin=1, npos=1) == -1
    assert call(1, good, npsflin=0, npos=0) == -1
    assert np.all(out == 7.0) and np.all(fit == 7.0)
    with pytest.raises(ValueError):                      # a wrong weights length is refused by the binding
        ctx.reconstruct_band(lb, np.ones((1, 4)), [1.0], [0.5], [20.0])
    w = np.array([[1.0, 2.0, 1.0], [0.0, 1.0, 3.0]])
    r = ctx.reconstruct_band(lb, w, [1.0, 0.8], [0.5, 0.6], [20.0, 25.0])
    ctx.close()
    fresh = api.Context(dim=256, pixscale=ps, precision='mixed')
    f = fresh.reconstruct_band(lb, w, [1.0, 0.8], [0.5, 0.6], [20.0, 25.0])
    fresh.close()
    for k in ('psf', 'psf_sum', 'fit'):
        assert _same(r[k], f[k]), k


# ---- 7. Python API, SPARTA HDUs, CLI
@pytest.mark.parametrize('circular', [True, False])
def test_compute_band_psf(api, circular):
    ps = api.grid_pixscale(512)
    bands = [(480.0, 930.0), (600.0, 700.0)]
    t, psf = api.compute_band_psf(LB, 1.0, 0.7, 25.0, bands, verbose=False, dim=512, pixscale=ps, circular=circular)
    assert psf.shape == (2, 40, 40) and len(t) == 2
    names = list(t.colnames)
    assert names[:4] == ['band', 'lbda_eff', 'lbda_min', 'lbda_max'] and names[-3:] == ['SEEING', 'GL', 'L0']
    assert ('rot' in names) != circular and 'lbda' not in names
    np.testing.assert_array_equal(np.asarray(t['band']), [0, 1])
    w = _norm(api.band_weights(LB, bands))
    np.testing.assert_allclose(np.asarray(t['lbda_eff']), w @ LB, rtol=1e-14)
    np.testing.assert_array_equal(np.asarray(t['lbda_min']), [480.0, 600.0])
    np.testing.assert_array_equal(np.asarray(t['lbda_max']), [930.0, 700.0])
    from muse_psfr_amd.psfrec import get_context, _resolve_masks
    ctx = get_context(512, ps, 40, 'mixed', 0)
    per = ctx.reconstruct(LB, [1.0], [0.7], [25.0], [0], H, masks=_resolve_masks('host'))['psf'][0]
    assert rel_err(psf, _reduce(w, per)) < 1e-6
    fit = ctx.fit_stamps(psf) if circular else ctx.fit_stamps_elliptical(psf)
    np.testing.assert_array_equal(np.asarray(t['n']), fit[:, 4 if circular else 5])
    # at field positions: rows (position, band)
    pos = [(10.0, 0.0), (0.0, -20.0)]
    tf, pf = api.compute_band_psf(LB, 1.0, 0.7, 25.0, bands, positions=pos, verbose=False, dim=512, pixscale=ps,
                                  circular=circular)
    assert pf.shape == (2, 2, 40, 40) and len(tf) == 4
    np.testing.assert_array_equal(np.asarray(tf['dir_idx']), [0, 0, 1, 1])
    np.testing.assert_array_equal(np.asarray(tf['band']), [0, 1, 0, 1])


def _sparta(api, nlines):
    from muse_psfr_amd import _minifits
    hdu = api.create_sparta_table(nlines=nlines, seeing=1.0, L0=20, GL=0.6)
    d = hdu.data
    rng = np.random.default_rng(4)
    for k in range(1, 5):
        d['LGS%d_SEEING' % k] = 0.7 + 0.6 * rng.random(nlines)
        d['LGS%d_TUR_GND' % k] = 0.4 + 0.5 * rng.random(nlines)
        d['LGS%d_L0' % k] = 12 + 15 * rng.random(nlines)
    d['LGS4_L0'][0] = 50.0
    return _minifits.HDUList([_minifits.PrimaryHDU(), hdu])


def test_sparta_band_hdus_and_cli(api, tmp_path):
    from muse_psfr_amd import psfrec, cli, _minifits
    ps = api.grid_pixscale(512)
    kw = dict(nl=4, dim=512, pixscale=ps, device=0, verbose=False)
    bands = [(490.0, 930.0), (600.0, 700.0)]
    blb = np.arange(490.0, 931.0, 10.0)
    base = api.compute_psf_from_sparta(_sparta(api, 3), **kw)
    out = api.compute_psf_from_sparta(_sparta(api, 3), bands=bands, band_lbda=blb, **kw)
    names = [h.name for h in out]
    assert names[:len(base)] == [h.name for h in base]
    assert names[len(base):] == ['FIT_BAND_ROWS', 'PSF_BAND', 'FIT_BAND']
    for hb, ho in zip(base, out):
        if hb.data is not None:
            assert np.asarray(hb.data).tobytes() == np.asarray(ho.data).tobytes(), hb.name
    pb = np.asarray(out['PSF_BAND'].data)
    assert pb.shape == (2, 40, 40)
    # PSF_BAND = the row mean of compute_band_psf's stamps; FIT_BAND_ROWS = their fits
    fr = np.asarray(out['FIT_ROWS'].data)
    stats = np.stack([fr['SEEING'], fr['GL'], fr['L0']], axis=1)[::4]
    three = [True, False, False]
    res = [api.compute_band_psf(blb, s, g, l, bands, three_lgs_mode=t, verbose=False, dim=512, pixscale=ps)
           for (s, g, l), t in zip(stats, three)]
    mean = np.mean([p for _, p in res], axis=0)
    assert np.abs(pb - mean).max() <= 1e-13 * np.abs(mean).max()
    rows = out['FIT_BAND_ROWS'].data
    np.testing.assert_array_equal(np.asarray(rows['row_idx']), [1, 1, 2, 2, 3, 3])
    np.testing.assert_array_equal(np.asarray(rows['band']), [0, 1, 0, 1, 0, 1])
    np.testing.assert_array_equal(np.asarray(rows['n']), np.concatenate([np.asarray(t['n']) for t, _ in res]))
    ctx = psfrec.get_context(512, ps, 40, 'mixed', 0)
    np.testing.assert_array_equal(np.asarray(out['FIT_BAND'].data['n']), ctx.fit_stamps(pb)[:, 4])
    assert out['FIT_BAND'].header['SEEING'] == out['FIT_MEAN'].header['SEEING']
    # the FITS round trip
    path = str(tmp_path / 'band.fits')
    out.writeto(path, overwrite=True)
    back = _minifits.open(path)
    assert np.array_equal(np.asarray(back['PSF_BAND'].data), pb)
    for name in ('FIT_BAND_ROWS', 'FIT_BAND'):
        for col in ('band', 'lbda_eff', 'fwhm', 'n'):
            np.testing.assert_array_equal(np.asarray(back[name].data[col]), np.asarray(out[name].data[col]))
    # the CLI
    path = str(tmp_path / 'cli.fits')
    cli.main(['--values', '1.0,0.7,25', '--band', '600:700', '--band', '490:930', '--band-step', '10', '-o', path,
              '--logfile', str(tmp_path / 'log.txt')])
    back = _minifits.open(path)
    assert np.asarray(back['PSF_BAND'].data).shape == (2, 40, 40)
    np.testing.assert_array_equal(np.asarray(back['FIT_BAND'].data['lbda_min']), [600.0, 490.0])
    assert len(np.asarray(back['FIT_BAND_ROWS'].data['n'])) == 2
