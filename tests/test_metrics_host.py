"""CPU: the fp64 NumPy reference of the PSF energy metrics (tests/metrics_ref.py) against facts that do not depend on
it, the argument validation of psf_metrics / metrics= (every refusal a ValueError, no GPU present) and the
metrics=None code paths."""
import inspect

import numpy as np
import pytest

import metrics_ref as R

RNG = np.random.default_rng(3)
CASES = [(19.5, 19.5, 0.3), (19.5, 19.5, 0.5), (20.0, 20.0, 0.7), (19.3, 20.8, 1.0), (18.1, 21.4, 2.5), (19.5, 19.5, 7.0),
         (20.2, 19.9, 12.345), (19.5, 19.5, 19.9)] + [(*RNG.uniform(17, 22, 2), RNG.uniform(0.1, 15)) for _ in range(12)]


@pytest.mark.parametrize('cp,cq,r', CASES)
def test_areas_sum_to_the_disc_and_lie_in_the_unit_interval(cp, cq, r):
    a = R.circle_overlap(cp, cq, r)
    assert a.min() >= 0.0 and a.max() <= 1.0
    # (the circle is inside the stamp: every case keeps r below the distance to the nearest stamp edge)
    assert min(cp + 0.5, 39.5 - cp, cq + 0.5, 39.5 - cq) > r
    assert abs(a.sum() - np.pi * r * r) <= 1e-12 * max(1.0, np.pi * r * r)


@pytest.mark.parametrize('cp,cq,r', CASES)
def test_pixels_wholly_inside_or_outside(cp, cq, r):
    a = R.circle_overlap(cp, cq, r)
    p, q = np.mgrid[0:40, 0:40].astype(float)
    far = np.hypot(np.abs(p - cp) + 0.5, np.abs(q - cq) + 0.5)
    near = np.hypot(np.maximum(np.abs(p - cp) - 0.5, 0), np.maximum(np.abs(q - cq) - 0.5, 0))
    assert np.all(np.abs(a[far <= r] - 1.0) <= 1e-13)
    assert np.all(a[near >= r] <= 1e-13)
    cut = (far > r) & (near < r)
    assert np.all(a[cut] > 0.0) and np.all(a[cut] < 1.0)


@pytest.mark.parametrize('cp,cq,r', CASES[:10])
def test_areas_against_a_supersampled_mask(cp, cq, r):
    """64 x 64 sub-pixels per pixel, each counted by its centre.  A sub-pixel is counted wrongly only if the circle
    passes through it; the circle crosses each of the 64 sub-rows of a pixel at most twice (it is convex), and of a
    row's sub-pixels it then cuts at most those between two crossings of the row's edges -- per pixel the error is
    bounded by the sub-pixels the arc visits, at most 2 * 64 + 2 * 64 (one per crossed sub-row or sub-column line),
    each of area 1 / 64^2: |error| <= 4 * 64 / 64^2 = 4 / 64 per boundary pixel, and the errors of all pixels sum to
    at most (boundary pixels) * 4 / 64.  Pixels the circle does not cut are exact."""
    n = 64
    a = R.circle_overlap(cp, cq, r)
    sub = (np.arange(40 * n) + 0.5) / n - 0.5
    mask = ((sub[:, None] - cp) ** 2 + (sub[None, :] - cq) ** 2 <= r * r)
    ss = mask.reshape(40, n, 40, n).sum(axis=(1, 3)) / float(n * n)
    cut = (a > 0) & (a < 1)
    assert np.all(np.abs(a - ss)[~cut] <= 1e-13)
    assert np.abs(a - ss).max() <= 4.0 / n
    assert abs((a - ss).sum()) <= cut.sum() * 4.0 / n
    # (in practice the centre rule is far better than the bound)
    assert np.abs(a - ss).max() <= 0.5 / n


def test_constant_stamp():
    st = np.full((40, 40), 0.37)
    c = (19.5, 19.5)
    for r in (0.3, 1.0, 4.2, 19.0):
        assert abs(R.EE(st, c, r) - np.pi * r * r / 1600.0) <= 1e-14
    for s in (0.3, 1.0, 2.5, 7.0, 39.0):
        assert abs(R.SQE(st, c, s) - s * s / 1600.0) <= 1e-14
    # off-centre too, while the aperture stays on the stamp
    assert abs(R.EE(st, (17.2, 21.9), 5.5) - np.pi * 5.5 ** 2 / 1600.0) <= 1e-14
    assert abs(R.SQE(st, (17.2, 21.9), 5.5) - 5.5 ** 2 / 1600.0) <= 1e-14
    assert abs(R.ee_radius(st, c, 0.25) - np.sqrt(0.25 * 1600 / np.pi)) <= 1e-10


def test_box_overlap_is_exact():
    b = R.box_overlap(19.5, 19.5, 1.0)
    assert b.sum() == 1.0 and np.count_nonzero(b) == 4 and np.all(b[19:21, 19:21] == 0.25)
    b = R.box_overlap(20.0, 20.0, 1.0)
    assert b[20, 20] == 1.0 and b.sum() == 1.0
    b = R.box_overlap(20.25, 19.0, 2.0)
    assert abs(b.sum() - 4.0) <= 1e-15 and b[20, 19] == 1.0 and abs(b[19, 19] - 0.25) <= 1e-15
    assert abs(b[21, 19] - 0.75) <= 1e-15 and abs(b[21, 18] - 0.375) <= 1e-15


def test_ee_is_monotone_and_reaches_one():
    import moffat_ell_ref as M
    st = M.stamp(1.0, 20.3, 18.9, 4.0, 0.7, 30.0, 2.5)
    c = R.centroid(st)
    rs = np.concatenate([np.linspace(0.05, 3, 60), np.linspace(3, 32, 60)])
    ee = np.array([R.EE(st, c, r) for r in rs])
    assert np.all(np.diff(ee) >= -1e-15)
    assert abs(R.EE(st, c, R.r_max(c) + 1e-9) - 1.0) <= 1e-14
    for f in (0.1, 0.5, 0.8, 0.95):
        assert abs(R.EE(st, c, R.ee_radius(st, c, f)) - f) <= 1e-12
    m = R.metrics(st, radii=(1.0,), boxes=(2.0,), fractions=(0.5,))
    assert (m['peak_p'], m['peak_q']) == (20, 19) and m['peak'] == st.max() and m['flux'] == st.sum()


# ---- argument validation: ValueError, and no GPU context is created (there is no GPU here: creating one raises
# MpsfrError, which is not a ValueError)
def _stamps(n=2):
    return np.ones((n, 40, 40))


@pytest.mark.parametrize('kw', [
    dict(radii=[0.0]), dict(radii=[-1.0]), dict(radii=[np.nan]), dict(radii=[np.inf]), dict(radii=[16.2]),
    dict(radii=np.ones(17) * 0.2), dict(radii=[[0.2, 0.4]]), dict(radii='abc'),
    dict(boxes=[0.0]), dict(boxes=[np.nan]), dict(boxes=[17.0]), dict(boxes=np.ones(17)),
    dict(fractions=[0.0]), dict(fractions=[1.0]), dict(fractions=[np.nan]), dict(fractions=np.full(17, 0.5)),
    dict(radii=(), boxes=(), fractions=()),
    dict(center='peak'), dict(center=None), dict(center=[[19.5, 19.5]]), dict(center=[[19.5, np.nan], [1.0, 2.0]]),
    dict(center=np.zeros((2, 3))), dict(pixscale=0.0), dict(pixscale=-0.2), dict(precision='fp16'),
])
def test_psf_metrics_refusals(kw):
    from muse_psfr_amd import psf_metrics
    with pytest.raises(ValueError):
        psf_metrics(_stamps(), **kw)


@pytest.mark.parametrize('st', [np.ones((40, 39)), np.ones((3, 41, 41)), np.ones(40), np.ones((0, 40, 40)), 'stamps'])
def test_psf_metrics_refuses_other_shapes(st):
    from muse_psfr_amd import psf_metrics
    with pytest.raises(ValueError):
        psf_metrics(st)


@pytest.mark.parametrize('metrics', [dict(radii=[-1.0]), dict(radius=[1.0]), 'yes', 3, dict(center='middle'),
                                     dict(fractions=[1.5])])
def test_metrics_argument_refusals(metrics):
    import muse_psfr_amd as api
    lb = [500.0, 700.0]
    with pytest.raises(ValueError):
        api.compute_psf(lb, 1.0, 0.7, 25.0, verbose=False, metrics=metrics)
    with pytest.raises(ValueError):
        api.compute_field_psf(lb, 1.0, 0.7, 25.0, verbose=False, metrics=metrics)
    with pytest.raises(ValueError):
        api.compute_band_psf(lb, 1.0, 0.7, 25.0, [(480, 720)], verbose=False, metrics=metrics)
    with pytest.raises(ValueError):
        api.compute_profile_psf(lb, 1.0, 25.0, [0.7, 0.3], [100.0, 10000.0], verbose=False, metrics=metrics)
    with pytest.raises(ValueError):
        api.compute_psf_from_sparta([], metrics=metrics)


def test_metrics_defaults_to_none_everywhere():
    import muse_psfr_amd as api
    for f in (api.compute_psf, api.compute_field_psf, api.compute_band_psf, api.compute_profile_psf,
              api.compute_psf_from_sparta):
        p = inspect.signature(f).parameters['metrics']
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, f.__name__


def test_metrics_none_leaves_the_columns_alone():
    from muse_psfr_amd import psfrec
    assert psfrec._metrics_request(None, 0.2) is None
    req = psfrec._metrics_request(True, 0.2)
    assert req == dict(radii=psfrec.METRIC_RADII, boxes=psfrec.METRIC_BOXES, fractions=psfrec.METRIC_FRACTIONS,
                       center='centroid')
    assert psfrec._metrics_request(dict(radii=[0.5]), 0.2)['radii'] == [0.5]
    # the fit column builders are what they were: no metric column without a request
    fit = np.abs(np.random.default_rng(1).normal(1.0, 0.1, (3, 16))) + 1.0
    assert tuple(psfrec._fit_columns(np.arange(3.0), fit, 0.2)) == psfrec._FIT_COLS
    fe = np.abs(np.random.default_rng(1).normal(1.0, 0.1, (3, 24))) + 1.0
    assert tuple(psfrec._fit_columns_ell(np.arange(3.0), fe, 0.2)) == psfrec._FIT_COLS_ELL
    assert not set(psfrec._METRIC_COLS) & (set(psfrec._FIT_COLS) | set(psfrec._FIT_COLS_ELL))


def test_metric_columns_and_meta():
    from muse_psfr_amd import _lib, psfrec
    rows = np.arange(2 * (8 + 2 + 1 + 3), dtype=float).reshape(2, -1)
    cols = psfrec._metric_columns(rows, 2, 1, 3, 0.2)
    assert list(cols) == ['flux', 'peak', 'center', 'ee', 'sqe', 'r_ee', 'status']
    assert cols['ee'].shape == (2, 2) and cols['sqe'].shape == (2, 1) and cols['r_ee'].shape == (2, 3)
    assert np.array_equal(cols['center'], rows[:, 4:6]) and np.array_equal(cols['r_ee'], rows[:, 11:14] * 0.2)
    meta = psfrec._metric_meta([0.2, 0.4], [0.2], [0.5, 0.8, 0.9], 'centroid')
    assert meta == dict(MRAD1=0.2, MRAD2=0.4, MBOX1=0.2, MFRAC1=0.5, MFRAC2=0.8, MFRAC3=0.9, MCENTER='centroid')
    rad, box, frac = _lib.metric_parameters([1.0, 2.0], None, 0.5)
    assert rad.tolist() == [1.0, 2.0] and box.size == 0 and frac.tolist() == [0.5]


def test_metrics_hdu_through_minifits_and_back(tmp_path):
    """The 2-D columns of a METRICS_* table survive the package's own FITS writer and reader."""
    from muse_psfr_amd import _minifits
    cols = dict(lbda=np.array([500.0, 700.0]), ee=np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]]),
                sqe=np.array([[0.7, 0.75], [0.8, 0.85]]), status=np.array([0, 2], dtype=np.int64))
    hdr = _minifits.Header()
    hdr['MRAD1'] = 0.2
    hdr['MCENTER'] = 'centroid'
    hdu = _minifits.BinTableHDU.from_columns(cols, hdr, 'METRICS_MEAN')
    path = str(tmp_path / 'm.fits')
    _minifits.HDUList([_minifits.PrimaryHDU(), hdu]).writeto(path, overwrite=True)
    back = _minifits.open(path)['METRICS_MEAN']
    for k, v in cols.items():
        assert np.array_equal(np.asarray(back.data[k]), v), k
    assert back.header['MRAD1'] == 0.2 and back.header['MCENTER'] == 'centroid'
