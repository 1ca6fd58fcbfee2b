"""The plate solver's rule (F21) in its NumPy form, tests/astrometry_model.py, against planted WCSs; and the host side of
the feature that needs no GPU: the SIP header writer, the hints, the script's parser, the argument checks of the two entry points and
what ApAstrometry does with its files.

The bound on a recovered WCS is the one of tests/test_gpu_register.py::test_image_round_trip_512: the largest corner error of a
least-squares map of p parameters through n pairs of per-axis noise sigma is held to 5 sigma sqrt((p + 1) / n) - 7 for the six of a
TAN fit, 13 for the twelve with SIP order 2.
"""
import ctypes as C
import os

import numpy as np
import pytest

from astrophotography_amd import fitsio, wcs
from tests import astrometry_model as am

pytestmark = pytest.mark.filterwarnings('ignore::RuntimeWarning')

_SOLVED = {}


def solved(i):
    """The model's solution of FIELDS[i], computed once (tests/test_gpu_astrometry.py compares the device with it)."""
    if i not in _SOLVED:
        f = am.field(am.FIELDS[i])
        _SOLVED[i] = (f,) + am.solve_field(f['xy'], f['shape'], f['cat'], f['centre'], f['s0'], 1.3, f['R'])
    return _SOLVED[i]


@pytest.mark.parametrize('i', range(len(am.FIELDS)))
def test_model_recovers_the_planted_wcs(i):
    """Both parities, true / nominal scale 0.85, 1.0 and 1.28, a 768 x 512 frame, a hint one field width off (field 5: 0.7 of the
    width on either axis); sigma = 0.1 px, 80 % of the stars detected, 10 % spurious; 75 cells."""
    f, out, margin = solved(i)
    seed, shape, factor, rot, mirror, off = am.FIELDS[i]
    assert len(out['peak_votes']) <= 75
    assert out['status'] == am.NOMINAL
    n = out['n_matched']
    corner = am.corner_error(out['wcs'], f['truth'], shape)
    print('field %d: %d of %d stars matched, rms %.4f px, corner error %.4f px (bound %.4f), cell %d of %d, scale %.5f, margin %.3g'
          % (seed, n, len(f['xy']), out['rms'], corner, 5.0 * am.SIGMA * np.sqrt(7.0 / n), out['cell'], len(out['peak_votes']), out['cell_scale'], margin))
    assert corner <= 5.0 * am.SIGMA * np.sqrt(7.0 / n)
    assert margin >= 1e-9
    assert out['parity'] == (-1 if mirror else 1)
    assert abs(out['cell_scale'] - factor) <= 1e-3 and abs(out['scale'] - factor * f['s0']) <= 1e-3 * f['s0']
    # the pairs are true: an image star that came from the catalogue is paired with its own row
    truth = f['rows'][out['pairs'][:, 0]]
    assert np.array_equal(truth[truth >= 0], out['pairs'][truth >= 0, 1])


def test_an_unrelated_list_has_no_solution():
    f = am.field(am.FIELDS[0])
    out, _ = am.solve_field(am.unrelated_list(7, f['shape']), f['shape'], f['cat'], f['centre'], f['s0'], 1.3, f['R'])
    assert out['status'] == am.NO_SOLUTION and out['wcs'] is None and out['n_matched'] == 0
    assert out['candidates'] and not any(c['counted'] for c in out['candidates'])
    assert out['peak_votes'].max() < solved(0)[1]['peak_votes'].max()


def test_a_too_small_scale_err_ratio_fails_the_scale_test():
    """True scale 1.28 of the nominal, ratio 1.1: cells are registered, at scale 1.28, and the scale test refuses them."""
    f = am.field(am.FIELDS[2])
    out, _ = am.solve_field(f['xy'], f['shape'], f['cat'], f['centre'], f['s0'], 1.1, 0.38)
    assert len(out['peak_votes']) <= 75
    assert out['status'] == am.NO_SOLUTION and out['wcs'] is None
    ok = [c for c in out['candidates'] if c['ok']]
    assert ok and all(abs(c['scale'] - 1.28) < 1e-3 and not c['counted'] for c in ok)


def test_cells_and_levels():
    assert np.allclose(am.scale_levels(1.3), [1 / 1.3, 1.0, 1.3]) and am.scale_levels(1.0) == [1.0]
    assert len(am.scale_levels(1.5)) == 5 and np.isclose(am.scale_levels(1.5)[0], 1 / 1.5) and np.isclose(am.scale_levels(1.5)[-1], 1.5)
    cells = am.make_cells((512, 768), 2.0, 1.3, 0.2)                   # R = 360 nominal pixels: two strides at every level
    assert len(cells) == 75
    for k, f in enumerate(am.scale_levels(1.3)):
        level = cells[25 * k:25 * k + 25]
        stride = f * 512 / 2.0
        assert np.all(level[:, 2] == stride)
        assert np.array_equal(level[:5, 0], stride * np.arange(-2, 3)) and np.array_equal(level[::5, 1], stride * np.arange(-2, 3))
    from astrophotography_amd import ops
    got, cos_rc = ops.astrometry_cells((512, 768), 2.0, 1.3, 0.2)
    assert np.array_equal(got, cells) and cos_rc == am.search_radius_cos((512, 768), 1.3, 0.2, 2.0)


def test_sip_writer_round_trips_through_from_header():
    f = am.sip_field(1)
    out, _ = am.solve_field(f['xy'], f['shape'], f['cat'], f['centre'], f['s0'], 1.3, f['R'], use_sip=True)
    w = out['wcs']
    assert isinstance(w, wcs.SipWcs) and w.ap is not None
    hdr = fitsio.Header()
    for k, v in w.header_cards().items():
        hdr[k] = v
    back = wcs.from_header(fitsio.Header.fromstring(hdr.tostring()))
    assert isinstance(back, wcs.SipWcs)
    assert hdr['CTYPE1'] == 'RA---TAN-SIP' and hdr['CTYPE2'] == 'DEC--TAN-SIP' and hdr['A_ORDER'] == 2 and hdr['BP_ORDER'] == 2
    gx, gy = np.meshgrid(np.linspace(0, 1023, 9), np.linspace(0, 1023, 9))
    ra, dec = w.pix2sky(gx, gy)
    ra2, dec2 = back.pix2sky(gx, gy)
    assert np.abs(ra - ra2).max() <= 1e-12 and np.abs(dec - dec2).max() <= 1e-12
    px, py = w.sky2pix(ra, dec)
    px2, py2 = back.sky2pix(ra, dec)
    assert np.abs(px - px2).max() <= 1e-12 and np.abs(py - py2).max() <= 1e-12
    assert np.abs(px - gx).max() <= 1e-9 and np.abs(py - gy).max() <= 1e-9
    # a plain TAN object writes what it always wrote
    assert 'A_ORDER' not in w.tan().header_cards() and w.tan().header_cards()['CTYPE1'] == 'RA---TAN'


def test_hints_follow_the_reference():
    """Hand-written headers through the reference's arithmetic (core/ApAstrometry.py _generate_hints)."""
    from astrophotography_amd.core.ApAstrometry import generate_hints
    h = generate_hints({'APRX_RA': 10.0, 'APRX_DEC': -5.0, 'RA-OBJ': 83.5, 'DEC-OBJ': 22.25, 'APRX_FOV': 0.9, 'APRX_XPS': 1.5, 'APRX_YPS': 2.0})
    assert (h['ra'], h['dec']) == (83.5, 22.25)                          # RA-OBJ / DEC-OBJ before APRX_RA / APRX_DEC
    assert h['scale'] == np.sqrt((1.5 * 1.5 + 2.0 * 2.0) / 2) and h['ratio'] == 1.3
    assert h['radius'] == 2 and h['scale_lower'] == h['scale'] / 1.3 and h['scale_upper'] == h['scale'] * 1.3     # ceil(0.9 * 1.5 * 1.3 = 1.755)
    h = generate_hints({'APRX_RA': 10.0, 'APRX_DEC': -5.0, 'APRX_XPS': 2.0, 'APRX_YPS': 2.0}, scale_err_ratio=1.5)
    assert (h['ra'], h['dec'], h['scale']) == (10.0, -5.0, 2.0) and h['radius'] == 9            # the 4 degree fallback: ceil(4 * 1.5 * 1.5)
    h = generate_hints({'APRX_RA': 10.0, 'APRX_DEC': -5.0, 'APRX_FOV': 0.9, 'APRX_XPS': 1.5, 'APRX_YPS': 2.0, 'IMG_COLS': 3000, 'IMG_ROWS': 2000},
                       user_scale=1.2)
    fov = np.hypot(3000 * 1.2 / 3600.0, 2000 * 1.2 / 3600.0)
    assert h['scale'] == 1.2 and h['radius'] == int(np.ceil(fov * 1.5 * 1.3)) == 3             # user_scale: the list's estimates are not looked at
    h = generate_hints({'APRX_XPS': 1.5, 'APRX_YPS': 2.0}, user_scale=2.0)
    assert h['ra'] is None and h['radius'] is None and h['scale'] == 2.0
    h = generate_hints({'RA-OBJ': 1.0, 'DEC-OBJ': 2.0, 'APRX_XPS': 1.5})
    assert h['scale'] is None and h['radius'] == 8


def test_script_accepts_the_reference_command_lines():
    from astrophotography_amd.scripts import ap_astrometry as s
    a = s.command_line_opts(['img.fits', 'stars.fits', 'out.fits', '--catalog', 'cat.fits'])
    assert (a.inp_image, a.source_list, a.out_image, a.catalog) == ('img.fits', 'stars.fits', 'out.fits', 'cat.fits')
    assert a.key is None and a.loglevel == 'INFO' and a.image_extension == 0 and a.xy_extension == 'AP_XYPOS' and not a.use_sip
    assert a.user_scale is None and a.scale_err_ratio is None and a.catalog_ext == 'CATALOG' and (a.ra_col, a.dec_col, a.mag_col) == ('ra', 'dec', 'mag')
    assert a.ra is None and a.dec is None and a.radius is None and a.nbright == 40 and a.match_radius == 3.0 and a.min_matched == 10
    a = s.command_line_opts(['img.fits', 'stars.fits', 'out.fits', '--key', 'abcdef', '-l', 'DEBUG', '--image_extension', '0', '--xy_extension', 'XY',
                             '--use-sip', '--user_scale', '1.9', '--scale_err_ratio', '1.5', '--catalog', 'c.fits', '--catalog_ext', 'GAIA',
                             '--ra_col', 'RA_ICRS', '--dec_col', 'DE_ICRS', '--mag_col', 'Gmag', '--ra', '83.6', '--dec', '22', '--radius', '0.5',
                             '-K', '30', '--match_radius', '2', '--min_matched', '20'])
    assert a.key == 'abcdef' and a.loglevel == 'DEBUG' and a.xy_extension == 'XY' and a.use_sip and a.user_scale == 1.9 and a.scale_err_ratio == 1.5
    assert (a.catalog_ext, a.ra_col, a.dec_col, a.mag_col, a.ra, a.dec, a.radius, a.nbright, a.match_radius, a.min_matched) == \
        ('GAIA', 'RA_ICRS', 'DE_ICRS', 'Gmag', 83.6, 22.0, 0.5, 30, 2.0, 20)
    for bad in (['img.fits', 'stars.fits', 'out.fits'], ['img.fits', 'stars.fits', 'out.fits', '--catalog', 'c.fits', '--ra', '1']):
        with pytest.raises(SystemExit):
            s.command_line_opts(bad)


def test_class_is_exported_lazily():
    import astrophotography_amd as ap
    assert 'ApAstrometry' in ap.__all__
    cls = ap.ApAstrometry
    assert (cls.NOMINAL, cls.INPUT_ERROR, cls.NO_SOLUTION) == (0, 1, 2)


def test_capi_rejects_bad_arguments_before_device_work():
    from astrophotography_amd import _lib
    lib = _lib.load()
    d = C.c_void_p(64)                         # never dereferenced: validation comes first
    odd = C.c_void_p(68)
    E = _lib.E_INVAL
    ok = (0.0, 10.0, 0.5)
    assert lib.apgpu_sky_project(None, None, 0, *ok, None, None, None, None) == 0          # n = 0 returns at once
    assert lib.apgpu_sky_project(None, d, 5, *ok, d, d, d, None) == E
    assert lib.apgpu_sky_project(d, d, 5, *ok, None, d, d, None) == E
    assert lib.apgpu_sky_project(d, d, -1, *ok, d, d, d, None) == E
    assert lib.apgpu_sky_project(d, d, 2 ** 31, *ok, d, d, d, None) == E
    assert lib.apgpu_sky_project(odd, d, 5, *ok, d, d, d, None) == E
    assert lib.apgpu_sky_project(d, d, 5, float('nan'), 10.0, 0.5, d, d, d, None) == E
    assert lib.apgpu_sky_project(d, d, 5, 0.0, 91.0, 0.5, d, d, d, None) == E
    assert lib.apgpu_sky_project(d, d, 5, 0.0, 10.0, 1.5, d, d, d, None) == E
    assert lib.apgpu_sky_project(d, d, 5, 0.0, 10.0, float('nan'), d, d, d, None) == E
    assert b'sky_project' in lib.apgpu_last_error()
    assert lib.apgpu_cell_select(None, None, 0, None, 0, 8, None, None, None, None) == 0   # no cells: returns at once
    assert lib.apgpu_cell_select(d, d, 5, d, 0, 8, None, None, None, None) == 0
    assert lib.apgpu_cell_select(None, d, 5, d, 3, 8, d, d, d, None) == E
    assert lib.apgpu_cell_select(d, d, 5, None, 3, 8, d, d, d, None) == E
    assert lib.apgpu_cell_select(d, d, 5, d, 3, 8, None, d, d, None) == E
    assert lib.apgpu_cell_select(d, d, 5, d, 3, 8, d, d, None, None) == E
    assert lib.apgpu_cell_select(d, d, -1, d, 3, 8, d, d, d, None) == E
    assert lib.apgpu_cell_select(d, d, 2 ** 31, d, 3, 8, d, d, d, None) == E
    assert lib.apgpu_cell_select(d, d, 5, d, -1, 8, d, d, d, None) == E
    assert lib.apgpu_cell_select(d, d, 5, d, 3, 0, d, d, d, None) == E
    assert lib.apgpu_cell_select(d, d, 5, d, 3, _lib.CELL_MAX_CAPACITY + 1, d, d, d, None) == E
    assert lib.apgpu_cell_select(d, d, 5, d, 2 ** 20, 4096, d, d, d, None) == E            # 2^32 slots
    assert lib.apgpu_cell_select(d, odd, 5, d, 3, 8, d, d, d, None) == E
    assert lib.apgpu_cell_select(d, d, 5, d, 3, 8, C.c_void_p(66), d, d, None) == E
    assert b'cell_select' in lib.apgpu_last_error()


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def _write_inputs(tmp_path, mag_name='mag'):
    img, src, cat = str(tmp_path / 'img.fits'), str(tmp_path / 'stars.fits'), str(tmp_path / 'cat.fits')
    hdr = fitsio.Header()
    fitsio.write(img, np.zeros((64, 96), np.float32), hdr)
    x = np.linspace(5.0, 90.0, 12)
    y = np.linspace(60.0, 4.0, 12)
    pri = {'IMG_FILE': 'img.fits', 'IMG_COLS': 96, 'IMG_ROWS': 64, 'APRX_RA': 83.6, 'APRX_DEC': 22.0, 'APRX_FOV': 0.06, 'APRX_XPS': 2.0, 'APRX_YPS': 2.0}
    phot = {'id': np.arange(1, 13, dtype=np.int32), 'xcenter': x - 1.0, 'ycenter': y - 1.0, 'adu': np.linspace(9e4, 1e3, 12)}
    fitsio.write_table(src, [('AP_XYPOS', {'X': x, 'Y': y}, {'X': 'pix', 'Y': 'pix'}, [('COMMENT', 'Uses FITS 1-based pixel coordinate system.')]),
                             ('AP_L1MAG', phot, {'xcenter': 'pix', 'ycenter': 'pix'}, [('COMMENT', 'Uses python 0-based pixel coordinate system.')])],
                       header=pri)
    rng = np.random.default_rng(3)
    fitsio.write_table(cat, [('CATALOG', {'RA': 83.6 + rng.uniform(-0.2, 0.2, 50), 'Dec': 22.0 + rng.uniform(-0.2, 0.2, 50), mag_name: rng.uniform(8, 14, 50)},
                              None, None)])
    return img, src, cat


def test_class_refuses_bad_inputs_without_touching_files(tmp_path):
    from astrophotography_amd.core.ApAstrometry import ApAstrometry
    img, src, cat = _write_inputs(tmp_path)
    out = str(tmp_path / 'out.fits')
    before = open(src, 'rb').read()
    assert ApAstrometry(img, 0, src, 'AP_XYPOS', img, None, False, loglevel='CRITICAL', catalog=cat).status() == ApAstrometry.INPUT_ERROR     # output == input
    assert ApAstrometry(img, 0, src, 'AP_XYPOS', out, None, False, loglevel='CRITICAL', catalog=str(tmp_path / 'none.fits')).status() == 1
    assert ApAstrometry(str(tmp_path / 'none.fits'), 0, src, 'AP_XYPOS', out, None, False, loglevel='CRITICAL', catalog=cat).status() == 1
    assert ApAstrometry(img, 0, str(tmp_path / 'none.fits'), 'AP_XYPOS', out, None, False, loglevel='CRITICAL', catalog=cat).status() == 1
    assert ApAstrometry(img, 0, src, 'NO_SUCH_EXT', out, None, False, loglevel='CRITICAL', catalog=cat).status() == 1
    assert ApAstrometry(img, 0, src, 'AP_XYPOS', out, None, False, loglevel='CRITICAL', catalog=cat, catalog_ext='GAIA').status() == 1
    assert ApAstrometry(img, 0, src, 'AP_XYPOS', out, None, False, loglevel='CRITICAL', catalog=cat, mag_col='Gmag').status() == 1      # a missing column
    assert ApAstrometry(img, 0, img, 'AP_XYPOS', out, None, False, loglevel='CRITICAL', catalog=cat).status() == 1                      # not a source list
    _, _, cat2 = _write_inputs(tmp_path, mag_name='Gmag')
    assert ApAstrometry(img, 0, src, 'AP_XYPOS', out, None, False, loglevel='CRITICAL', catalog=cat2).status() == 1
    assert not os.path.exists(out) and open(src, 'rb').read() == before


def test_class_writes_nothing_without_a_solution_and_both_files_with_one(tmp_path, monkeypatch):
    """The solver replaced by a stand-in (the real one needs the device: tests/test_gpu_astrometry.py): what reaches it, and what the
    class does with either answer."""
    from astrophotography_amd import ops
    from astrophotography_amd.core.ApAstrometry import ApAstrometry
    img, src, cat = _write_inputs(tmp_path)
    out = str(tmp_path / 'out.fits')
    before = open(src, 'rb').read()
    seen = {}

    def no_solution(xy, shape, catalogue, centre, scale, ratio, radius, **kw):
        seen.update(xy=xy, shape=shape, catalogue=catalogue, centre=centre, scale=scale, ratio=ratio, radius=radius, kw=kw)
        return dict(status=ops.SOLVE_NO_SOLUTION, wcs=None, n_matched=0)
    monkeypatch.setattr(ops, 'solve_field', no_solution)
    a = ApAstrometry(img, 0, src, 'AP_XYPOS', out, 'ignored-key', False, None, 1.25, 'CRITICAL', catalog=cat, mag_col='MAG', K=30, min_matched=12)
    assert a.status() == ApAstrometry.NO_SOLUTION
    assert not os.path.exists(out) and open(src, 'rb').read() == before
    assert seen['shape'] == (64, 96) and seen['centre'] == (83.6, 22.0) and seen['scale'] == 2.0 and seen['ratio'] == 1.25
    assert seen['radius'] == 1 and seen['kw'] == dict(K=30, match_radius=3.0, min_matched=12, use_sip=False)
    assert np.array_equal(seen['xy'][:, 0], np.linspace(5.0, 90.0, 12) - 1.0) and np.array_equal(seen['xy'][:, 1], np.linspace(60.0, 4.0, 12) - 1.0)
    assert sorted(seen['catalogue']) == ['dec', 'mag', 'ra'] and len(seen['catalogue']['ra']) == 50

    w = wcs.SipWcs((48.5, 32.5), (83.61, 22.02), [[-5.5e-4, 1e-5], [1e-5, 5.5e-4]], {(2, 0): 1e-6}, {(1, 1): -2e-6}, {(0, 0): 1e-4, (2, 0): -1e-6}, {(1, 1): 2e-6})
    monkeypatch.setattr(ops, 'solve_field', lambda *a, **k: dict(status=ops.SOLVE_NOMINAL, wcs=w, n_matched=11, rms=0.21, scale=1.98, parity=1, cell=4))
    a = ApAstrometry(img, 0, src, 'AP_XYPOS', out, None, True, loglevel='CRITICAL', catalog=cat, centre=(83.7, 22.1), radius=0.5)
    assert a.status() == ApAstrometry.NOMINAL
    data, hdr = fitsio.read(out)
    assert data.shape == (64, 96) and data.dtype == np.float32
    back = wcs.from_header(hdr)
    assert isinstance(back, wcs.SipWcs) and back.a == w.a and back.bp == w.bp and np.array_equal(back.cd, w.cd) and np.array_equal(back.crval, w.crval)
    assert (hdr['ASTNMAT'], hdr['ASTRMS'], hdr['ASTSCALE'], hdr['ASTPARIT'], hdr['ASTCAT']) == (11, 0.21, 1.98, 1, 'cat.fits')
    assert abs(hdr['ASTROT'] - np.degrees(np.arctan2(1e-5, 5.5e-4))) < 1e-12
    cols, eh, prim = fitsio.read_table(src, 'AP_L1MAG')
    assert list(cols) == ['id', 'xcenter', 'ycenter', 'adu', 'ra', 'dec']
    ra, dec = w.pix2sky(cols['xcenter'], cols['ycenter'])
    assert np.array_equal(cols['ra'], ra) and np.array_equal(cols['dec'], dec)
    assert eh['TUNIT2'] == 'pix' and prim['APRX_RA'] == 83.6 and prim['IMG_FILE'] == 'img.fits'
    xy, _, _ = fitsio.read_table(src, 'AP_XYPOS')
    assert np.array_equal(xy['X'], np.linspace(5.0, 90.0, 12))
    # AP_XYPOS and the primary header are the same bytes as before
    assert open(src, 'rb').read()[:2 * 2880 + 2880] == before[:2 * 2880 + 2880]
    # a second run replaces the columns instead of adding to them
    assert ApAstrometry(img, 0, src, 'AP_XYPOS', out, None, True, loglevel='CRITICAL', catalog=cat).status() == 0
    assert list(fitsio.read_table(src, 'AP_L1MAG')[0]) == ['id', 'xcenter', 'ycenter', 'adu', 'ra', 'dec']
