"""ApMeasureStars on the host (no GPU): candidate selection, boxes and the FWHM statistics against the reference class's own
results (G17, tests/golden/make_golden_measurestars.py), the quality report, the script's flags and the C entry point's
argument checks."""
import logging

import numpy as np
import pytest

from tests import measurestars_model as mm


def host_object(c):
    """An ApMeasureStars up to (not including) the fits: the constructor's host part."""
    from astrophotography_amd.core.ApMeasureStars import ApMeasureStars, _DROPPED
    m = ApMeasureStars.__new__(ApMeasureStars)
    m._logger = logging.getLogger('test_measurestars')
    m._init_fwhm, m._num_per_reg, m._skip_brightest = c['init_fwhm'], 5, 0
    m._rows, m._cols = c['img'].shape
    m._full_srcs = {k: v for k, v in c['full'].items() if k not in _DROPPED}
    keep = ~c['src']['psbl_sat']
    m._init_srcs = {k: v[keep] for k, v in c['src'].items() if k not in _DROPPED}
    m._fit_box_initialization()
    return m


@pytest.mark.parametrize('fwhm, box, edge', [(1.5, 12, 6), (0.5, 12, 6), (2.0, 12, 6), (2.2, 12, 6), (2.4, 14, 8), (3.0, 18, 10),
                                             (5.0, 30, 16), (12.0, 72, 36), (3.9, 22, 12)])
def test_box_and_edge_numbers(fwhm, box, edge):
    from astrophotography_amd import ops
    assert ops.fit_box_width(fwhm) == (box, edge)


@pytest.mark.parametrize('k', mm.fitted_cases())
def test_selection_matches_the_reference(k):
    c = mm.case(k)
    m = host_object(c)
    assert (m._box_width_pix, m._edge_excl_pix) == (c['meta']['box_width'], c['meta']['edge_excl'])
    src_before = {key: v.copy() for key, v in c['src'].items()}
    t = m._select_candidates()
    assert np.array_equal(m._init_srcs['id'], c['trim']['id'])
    assert np.array_equal(m._init_srcs['nn_dist'], c['trim']['nn_dist'])        # sqrt of the same float64 sums
    assert np.array_equal(m._init_srcs['region'], c['trim']['region'])
    m._fit_table = t
    m._calculate_boxes()
    ref = c['res']
    assert np.array_equal(t['id'], ref['id'])
    assert np.array_equal(t['region'], ref['region'])
    for col in ('xmin', 'xmax', 'ymin', 'ymax', 'dx', 'dy', 'radius', 'nn_dist', 'xcenter', 'ycenter', 'peak_adu', 'magnitude'):
        assert np.array_equal(t[col], ref[col]), col
    assert all(np.array_equal(c['src'][key], src_before[key]) for key in src_before)      # the caller's table is untouched
    assert sorted(c['src']) == sorted(src_before)


def test_designed_rows_of_the_first_case():
    """The named stars of c0: close pairs either side of the box width, the four edge limits, the saturated star."""
    c = mm.case(0)
    names = c['meta']['named_stars']
    m = host_object(c)
    t = m._select_candidates()
    trimmed, fitted = set(m._init_srcs['id'].tolist()), set(t['id'].tolist())
    assert names['pair_under_a'] not in trimmed and names['neighbour_of_sat'] not in trimmed and names['psbl_sat'] not in trimmed
    assert names['pair_over_a'] in trimmed
    for side in ('left', 'right', 'bottom', 'top'):
        assert names[side + '_out'] in trimmed and names[side + '_out'] not in fitted, side
        assert names[side + '_in'] in fitted, side


def test_regions_with_three_and_with_no_candidates(caplog):
    c = mm.case(2)
    m = host_object(c)
    with caplog.at_level(logging.WARNING, logger='test_measurestars'):
        t = m._select_candidates()
    counts = {r: int((t['region'] == r).sum()) for r in ('CN', 'TL', 'TR', 'BR', 'BL')}
    assert counts['TL'] == 3 and counts['TR'] == 3 and counts['BR'] == 0
    assert 'no candidates in the BR region' in caplog.text
    assert list(t['region']) == sorted(t['region'], key=('CN', 'TL', 'TR', 'BR', 'BL').index)


def test_no_candidate_survives_in_a_frame_corner():
    g, meta = mm.golden()
    k = [i for i, m in enumerate(meta['cases']) if m['reference_raises']][0]
    assert any(meta['cases'][k]['name'] in d for d in meta['designed_failures'])
    c = mm.case(k)
    m = host_object(c)
    t = m._select_candidates()
    assert len(t['id']) == 0 and set(('region', 'nn_dist', 'dx')) <= set(t)
    m._fit_table = t
    m._calculate_boxes()
    assert len(t['xmin']) == 0


@pytest.mark.parametrize('k', mm.fitted_cases())
@pytest.mark.parametrize('direction', ['both', 'x', 'y'])
def test_median_fwhm_of_the_golden_columns(k, direction):
    from astrophotography_amd.core.ApMeasureStars import ApMeasureStars
    c = mm.case(k)
    m = ApMeasureStars.__new__(ApMeasureStars)
    m._fit_table = c['res']
    med, mad, n = m.median_fwhm(direction)
    ref = c['medians'][direction]
    assert n == int(ref[2])
    assert abs(med - ref[0]) <= 4 * np.spacing(ref[0]) and abs(mad - ref[1]) <= 4 * np.spacing(ref[1])


def test_sigma_clip_drops_an_outlier_and_is_circular_divides_by_yerr_only():
    from astrophotography_amd.core.ApMeasureStars import ApMeasureStars, sigma_clipped, mad_std
    v = np.r_[np.full(20, 3.0) + np.linspace(-0.1, 0.1, 20), 30.0]
    assert len(sigma_clipped(v)) == 20 and np.isnan(mad_std([]))
    assert ApMeasureStars.is_circular(3.0, 3.2, 1e-9, 0.1) is True
    assert ApMeasureStars.is_circular(3.0, 3.4, 10.0, 0.1) is False
    assert ApMeasureStars.is_circular(3.0, 3.4, 0.1, 0.0) is False


def hand_filled(platescale):
    import astrophotography_amd as ap
    obj = ap.ApFindStars.__new__(ap.ApFindStars)
    obj._configure('frame.fits', 0, 3.0, 7.0, 16, None, False, 0.8, 'ERROR', None, True)
    obj._hdr = {'NAXIS1': 176, 'NAXIS2': 144, 'EXPOSURE': 30.0, 'OBJECT': 'M 1'}
    if platescale:
        obj._hdr.update(FOCALLEN=1000.0, XPIXSZ=5.0, YPIXSZ=6.0)
    obj._bg_median, obj._bg_stddev = 100.25, 10.5
    obj._nsrcs_detected, obj._nsrcs_photom, obj._nsrcs_fitted, obj._nsrcs_saturated = 40, 38, 25, 1
    obj._phot_table = {'id': np.arange(3), 'psbl_sat': np.array([True, False, False])}
    obj._phot_stats = ((900.0, 0), (50.0, 19), (2.5, 37))
    obj._psf_table = {'id': np.arange(25)}
    obj._fwhm_both, obj._fwhm_x, obj._fwhm_y = (3.3, 0.02, 50), (3.1, 0.03, 25), (3.5, 0.04, 25)
    return obj


@pytest.mark.parametrize('platescale', [True, False])
def test_quality_report_yaml(tmp_path, platescale):
    yaml = pytest.importorskip('yaml')
    import math
    obj = hand_filled(platescale)
    path = tmp_path / 'q.yaml'
    obj.write_quality_report(str(path))
    text = path.read_text()
    rep = yaml.safe_load(text)
    assert list(rep) == ['image_info', 'background_info', 'source_info', 'saturation_info', 'psf_info']
    assert rep['image_info']['file'] == 'frame.fits' and rep['image_info']['ncols'] == 176 and rep['image_info']['exposure'] == 30.0
    assert rep['background_info'] == {'median': 100.25, 'stddev': 10.5}
    assert rep['source_info'] == {'num_detected': 40, 'num_with_photometry': 38, 'search_nsigma': 7.0, 'adups_brightest': 900.0,
                                  'adups_median': 50.0, 'adups_faintest': 2.5}
    assert rep['saturation_info'] == {'num_saturated_in_image': 1, 'num_saturated_in_photometry': 1}
    psf = rep['psf_info']
    assert psf['num_fit'] == 25 and psf['circular_psf'] is False              # |3.5 - 3.1| / 0.04 = 10 sigma
    assert 'median: 100.250000' in text                                       # six decimals
    if platescale:
        xps = 3600.0 * math.degrees(5.0e-6 / 1.0)
        yps = 3600.0 * math.degrees(6.0e-6 / 1.0)
        assert psf['fwhm_x']['fwhm_val_arcs'] == pytest.approx(3.1 * xps, abs=1e-6)
        assert psf['fwhm_y']['fwhm_err_arcs'] == pytest.approx(0.04 * yps, abs=1e-6)
        assert psf['fwhm_xandy']['fwhm_val_arcs'] == pytest.approx(3.3 * math.sqrt(0.5 * (xps ** 2 + yps ** 2)), abs=1e-6)
        assert 'approx_xpixsiz_arcs' in rep['image_info']
    else:
        assert psf['fwhm_x'] == {'fwhm_val_pix': 3.1, 'fwhm_err_pix': 0.03, 'fwhm_val_arcs': pytest.approx(-999 * 3.1),
                                 'fwhm_err_arcs': pytest.approx(-999 * 0.03), 'num_data_pts': 25}
        assert 'approx_xpixsiz_arcs' not in rep['image_info']
    kw = obj._build_keyword_dictionary('frame.fits', obj._hdr, 1.0, 2.0)
    assert kw['AP_FWHM'][0] == 3.3 and kw['AP_EFWHM'][0] == 0.02 and kw['AP_NFIT'][0] == 25


def test_report_and_plot_refusals():
    import astrophotography_amd as ap
    assert 'ApMeasureStars' in ap.__all__
    obj = ap.ApFindStars.__new__(ap.ApFindStars)
    with pytest.raises(NotImplementedError):
        obj.measure_fwhm('p.png')
    with pytest.raises(NotImplementedError, match=r'measure_fwhm\(None\)'):
        obj.write_quality_report('q.yaml')
    with pytest.raises(NotImplementedError):
        ap.ApMeasureStars(np.zeros((20, 20), np.float32), {}, 3.0, 0.0, {}, 'fits.png', None, 'ERROR', True)


def test_script_flags():
    from astrophotography_amd.scripts import ap_find_stars as s
    a = s.command_line_opts(['i.fits', 'o.fits'])
    assert a.fit_fwhm is False and a.quality_report is None
    a = s.command_line_opts(['i.fits', 'o.fits', '--fit_fwhm'])
    assert a.fit_fwhm is True and a.quality_report is None
    a = s.command_line_opts(['i.fits', 'o.fits', '--quality_report', 'q.yaml', '--fwhm_plot', 'f.png'])
    assert a.quality_report == 'q.yaml' and a.fwhm_plot == 'f.png'


def test_capi_rejects_bad_arguments_before_device_work():
    import ctypes as C
    from astrophotography_amd import _lib
    lib = _lib.load()
    d = C.c_void_p(16)                         # never dereferenced: validation comes first
    E, U = _lib.E_INVAL, _lib.E_UNSUPPORTED
    fit = lib.apgpu_gauss2d_fit_f32
    assert fit(d, 100, 100, d, d, d, 0, 12, 500, d, d, None) == 0              # nothing to do
    assert fit(None, 100, 100, d, d, d, 2, 12, 500, d, d, None) == E
    assert fit(d, 100, 100, None, d, d, 2, 12, 500, d, d, None) == E
    assert fit(d, 100, 100, d, d, None, 2, 12, 500, d, d, None) == E
    assert fit(d, 100, 100, d, d, d, 2, 12, 500, d, None, None) == E
    assert fit(d, 100, 100, d, d, d, -1, 12, 500, d, d, None) == E
    assert fit(d, 100, 100, d, d, d, 2, 13, 500, d, d, None) == E
    assert fit(d, 100, 100, d, d, d, 2, 10, 500, d, d, None) == E
    assert fit(d, 100, 100, d, d, d, 2, 12, 0, d, d, None) == E
    assert fit(d, 11, 100, d, d, d, 2, 12, 500, d, d, None) == E               # no box fits the image
    assert fit(d, 100, 100, d, d, d, 2, _lib.GAUSS2D_MAX_BOX + 2, 500, d, d, None) == U
    assert b'FWHM too large' in lib.apgpu_last_error()
    assert _lib.GAUSS2D_MAX_BOX >= 72 and lib.apgpu_version() == 130
