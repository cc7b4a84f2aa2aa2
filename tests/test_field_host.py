"""CPU: the field-resolved entry points (compute_field_psf, compute_psf_from_sparta(field_positions=...)) refuse
bad positions before any GPU context exists, assemble the FIT_FIELD columns from fit rows, and the 4-D PSF_FIELD
image survives a FITS round trip without astropy."""
import numpy as np
import pytest

from muse_psfr_amd import _lib, _minifits, psfrec


@pytest.fixture
def no_context(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('a GPU context was requested before the arguments were checked')
    monkeypatch.setattr(psfrec, 'get_context', refuse)


BAD_POSITIONS = [
    np.zeros((0, 2)),                   # empty
    [[0.0, 0.0, 0.0]],                  # not (n, 2)
    [1.0, 2.0],                         # 1-D
    np.zeros((2, 2, 2)),                # 3-D
    [[np.nan, 0.0]],
    [[0.0, np.inf]],
    [[60.5, 0.0]],                      # |x| > 60
    [[0.0, -61.0]],                     # |y| > 60
    [['a', 'b']],
]


@pytest.mark.parametrize('pos', BAD_POSITIONS)
def test_compute_field_psf_refuses_bad_positions_before_any_context(no_context, pos):
    with pytest.raises(ValueError):
        psfrec.compute_field_psf([600.0], 1.0, 0.7, 25.0, positions=pos, verbose=False)


@pytest.mark.parametrize('kwargs', [dict(npsflin=0), dict(npsflin=6), dict(npsflin=2.5), dict(seeing=-1.0),
                                    dict(GL=1.5), dict(L0=0.0), dict(lbda=[]), dict(lbda=[-600.0]),
                                    dict(h=(100, 1000, 10000)), dict(precision='f32')])
def test_compute_field_psf_refuses_bad_arguments_before_any_context(no_context, kwargs):
    args = dict(lbda=[600.0], seeing=1.0, GL=0.7, L0=25.0, verbose=False)
    args.update(kwargs)
    with pytest.raises(ValueError):
        psfrec.compute_field_psf(**args)


@pytest.mark.parametrize('fp', ['grids', [[0.0, 99.0]], np.zeros((0, 2)), [[np.nan, 1.0]]])
def test_sparta_refuses_bad_field_positions_before_any_context(no_context, fp):
    hdu = psfrec.create_sparta_table(nlines=2)
    hdul = _minifits.HDUList([_minifits.PrimaryHDU(), hdu])
    with pytest.raises(ValueError):
        psfrec.compute_psf_from_sparta(hdul, nl=3, field_positions=fp, verbose=False)


def test_field_positions_accepts_the_edges_and_caps_one_call():
    pos = _lib.field_positions([[60.0, -60.0], [0.0, 0.0]])
    assert pos.shape == (2, 2) and pos.dtype == np.float64 and pos.flags.c_contiguous
    assert _lib.field_positions(np.zeros((25, 2))).shape == (25, 2)
    with pytest.raises(ValueError):
        _lib.field_positions(np.zeros((26, 2)))
    assert _lib.field_positions(np.zeros((30, 2)), max_n=None).shape == (30, 2)


def test_grid_request_is_direction_perf():
    for n in range(1, 6):
        pos = psfrec._field_request(None, n)
        np.testing.assert_array_equal(pos, psfrec.direction_perf(n).T)
    # the reference's grid for npsflin = 2 is {-30, 0}
    assert set(psfrec._field_request(None, 2).ravel()) == {-30.0, 0.0}
    assert psfrec._field_groups(30) == [(0, 25), (25, 30)]
    assert psfrec._field_groups(25) == [(0, 25)]


def test_fit_field_columns_from_a_synthetic_fit_array():
    rng = np.random.default_rng(3)
    pos = np.array([[12.5, -7.0], [-29.0, 3.0], [0.0, 0.0]])
    lbda = np.array([500.0, 700.0])
    fit = rng.random((3, 2, _lib.NFIT)) + 1.5
    cols = psfrec._field_columns(lbda, pos, fit, 0.2)
    assert list(cols) == ['dir_idx', 'x', 'y'] + list(psfrec._FIT_COLS)
    np.testing.assert_array_equal(cols['dir_idx'], [0, 0, 1, 1, 2, 2])
    np.testing.assert_array_equal(cols['x'], [12.5, 12.5, -29.0, -29.0, 0.0, 0.0])
    np.testing.assert_array_equal(cols['y'], [-7.0, -7.0, 3.0, 3.0, 0.0, 0.0])
    np.testing.assert_array_equal(cols['lbda'], np.tile(lbda, 3))
    # the fit columns are those of _fit_columns on the rows in (position, wavelength) order
    ref = psfrec._fit_columns(np.tile(lbda, 3), fit.reshape(6, -1), 0.2)
    for k in psfrec._FIT_COLS:
        np.testing.assert_array_equal(cols[k], ref[k])
    np.testing.assert_array_equal(cols['fwhm'][:, 0], fit[:, :, 5].ravel() * 0.2)
    np.testing.assert_array_equal(cols['n'], fit[:, :, 4].ravel())


def test_psf_field_minifits_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    cube = rng.random((9, 3, 40, 40))
    cols = psfrec._field_columns([500.0, 700.0, 900.0], psfrec.direction_perf(3).T,
                                 rng.random((9, 3, _lib.NFIT)) + 1.5, 0.2)
    hdr = _minifits.Header()
    hdr['SEEING'] = 1.0
    hdul = _minifits.HDUList([_minifits.PrimaryHDU(), _minifits.ImageHDU(data=cube, name='PSF_FIELD'),
                              _minifits.BinTableHDU.from_columns(cols, hdr, 'FIT_FIELD')])
    path = str(tmp_path / 'field.fits')
    hdul.writeto(path)
    back = _minifits.open(path)
    got = np.asarray(back['PSF_FIELD'].data)
    assert got.shape == (9, 3, 40, 40)
    np.testing.assert_array_equal(got, cube)
    t = back['FIT_FIELD'].data
    np.testing.assert_array_equal(np.asarray(t['x']), cols['x'])
    np.testing.assert_array_equal(np.asarray(t['n']), cols['n'])
    np.testing.assert_array_equal(np.asarray(t['dir_idx']), cols['dir_idx'])
