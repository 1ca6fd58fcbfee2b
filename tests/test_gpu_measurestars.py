"""F7 Gaussian PSF fits on the GPU: ops.gauss2d_fit against the reference class's own fits (G17: astropy 4.3.1's
LevMarLSQFitter through ApMeasureStars), a reference-free check of the minimum, batch and edge cases, and ApFindStars.measure_fwhm
/ ap_find_stars --fit_fwhm --quality_report end to end.

Bounds: G17 records how far astropy's end point is from a tightly polished minimum (d_par in units of astropy's own error, the
relative chi^2 difference, the error ratio's distance from 1), maxima over all golden fits.  The device stops four orders
tighter, so it is held to 10 x those maxima - the factor covers star-to-star spread beyond the recorded sample.  Fits are
compared in the canonical form of tests/measurestars_model.py; the angle of a star whose axes differ by less than 3 of their
own sigma is left out."""
import math

import numpy as np
import pytest

from tests import measurestars_model as mm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
_fits = {}


def device_fit(k):
    """ops.gauss2d_fit on the golden boxes of case k: computed once, shared, not modified."""
    if k not in _fits:
        from astrophotography_amd import ops
        c = mm.case(k)
        r = c['res']
        _fits[k] = ops.gauss2d_fit(torch.from_numpy(c['img']).cuda(), r['xcenter'], r['ycenter'], r['peak_adu'], r['bgmed_per_pix'],
                                   c['init_fwhm'])
    return _fits[k]


def bounds():
    meta = mm.golden()[1]
    return 10 * meta['d_par_max'], 10 * meta['d_chi2_max'], 10 * meta['d_err_max'], meta['d_par_max']


@pytest.mark.parametrize('k', mm.fitted_cases())
def test_fits_match_the_reference(k):
    c = mm.case(k)
    ref, got = c['res'], device_fit(k)
    b_par, b_chi2, b_err, _ = bounds()
    print('case', c['meta']['name'], 'iterations per stage (max)', got['niter'].max(axis=0))
    assert np.array_equal(got['fit_ok'], ref['fit_ok'])
    for col in ('xmin', 'xmax', 'ymin', 'ymax'):
        assert np.array_equal(got[col], ref[col])
    worst = dict(par=0.0, chi2=0.0, err=0.0)
    same_labels = True
    for i in np.nonzero(ref['fit_ok'])[0]:
        x0, y0 = ref['xmin'][i], ref['ymin'][i]
        pr, er, sr = mm.canonical(*mm.params(ref, i, x0, y0))
        pg, eg, sg = mm.canonical(*mm.params(got, i, x0, y0))
        same_labels = same_labels and (sr == sg)
        d = np.abs(pg - pr) / er
        round_star = (pr[3] - pr[4]) < 3.0 * math.hypot(er[3], er[4])
        d[5] = 0.0 if round_star else mm.angle_diff(pg[5], pr[5]) / er[5]
        de = np.abs(eg / er - 1.0)
        if round_star:
            de[5] = 0.0
        dc = abs(got['rchisq'][i] - ref['rchisq'][i]) / ref['rchisq'][i]
        worst = dict(par=max(worst['par'], d.max()), chi2=max(worst['chi2'], dc), err=max(worst['err'], de.max()))
        assert d.max() <= b_par, (i, d)
        assert dc <= b_chi2, (i, dc)
        assert de.max() <= b_err, (i, de)
        assert got['circular'][i] == ref['circular'][i]
        assert abs(got['axrat'][i] - ref['axrat'][i]) <= b_par * ref['axrat_err'][i]
    print('worst: d_par %.2e (bound %.2e)  d_chi2 %.2e (%.2e)  d_err %.2e (%.2e)' % (worst['par'], b_par, worst['chi2'], b_chi2,
                                                                                    worst['err'], b_err))
    # the medians: 'both' does not depend on the labelling, 'x' and 'y' do
    from astrophotography_amd.core.ApMeasureStars import ApMeasureStars
    m = ApMeasureStars.__new__(ApMeasureStars)
    m._fit_table = got
    ok = ref['fit_ok']
    scale = float(np.max(np.r_[ref['fwhm_x_err'][ok], ref['fwhm_y_err'][ok]]))
    for direction in ('both',) + (('x', 'y') if same_labels else ()):
        med, mad, n = m.median_fwhm(direction)
        rmed, rmad, rn = c['medians'][direction]
        assert n == int(rn) and abs(med - rmed) <= b_par * scale and abs(mad - rmad) <= 2 * b_par * scale, direction


@pytest.mark.parametrize('k', mm.fitted_cases())
def test_device_answer_is_at_the_minimum(k):
    """Reference-free: the Gauss-Newton step at the device's answer, computed on the host in float64, is no larger than
    astropy's recorded distance from the minimum (in sigma)."""
    c = mm.case(k)
    got = device_fit(k)
    d_par_max = bounds()[3]
    Wb = c['meta']['box_width']
    worst = 0.0
    for i in np.nonzero(got['fit_ok'])[0]:
        x0, y0 = int(got['xmin'][i]), int(got['ymin'][i])
        p, _ = mm.params(got, i, x0, y0)
        step, err = mm.gauss_newton_step(p, c['img'][y0:y0 + Wb, x0:x0 + Wb])
        worst = max(worst, float(np.max(np.abs(step) / err)))
    print('largest Gauss-Newton step at the device answer: %.2e sigma (astropy: %.2e)' % (worst, d_par_max))
    assert worst <= d_par_max


def test_batches_and_empty_input():
    from astrophotography_amd import ops
    c = mm.case(0)
    img = torch.from_numpy(c['img']).cuda()
    r = c['res']
    empty = ops.gauss2d_fit(img, [], [], [], [], 3.0)
    assert all(len(empty[k]) == 0 for k in ops.GAUSS2D_COLUMNS) and empty['niter'].shape == (0, 3)
    one = ops.gauss2d_fit(img, r['xcenter'][3:4], r['ycenter'][3:4], r['peak_adu'][3:4], r['bgmed_per_pix'][3:4], 3.0)
    rep = np.arange(70) % len(r['id'])
    rep[41] = 3
    many = ops.gauss2d_fit(img, r['xcenter'][rep], r['ycenter'][rep], r['peak_adu'][rep], r['bgmed_per_pix'][rep], 3.0)
    full = device_fit(0)
    for col in ops.GAUSS2D_COLUMNS + ('bg_fit', 'niter'):
        assert np.array_equal(one[col][0], many[col][41]) and np.array_equal(one[col][0], full[col][3]), col
        assert np.array_equal(many[col][:25], full[col]), col


def synthetic(H, W, cy, cx, fwhm, ampl=4000.0, bg=50.0, seed=5):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    s = fwhm / mm.S2F
    return rng.poisson(bg + ampl * np.exp(-0.5 * ((xx - cx) ** 2 + (yy - cy) ** 2) / s ** 2)).astype(np.float32)


def test_box_sizes_corner_cap_and_empty_box():
    from astrophotography_amd import _lib, ops
    # a 12-pixel box that touches the image corner, on a frame no larger than the box
    img = synthetic(12, 12, 6.2, 5.7, 2.0)
    r = ops.gauss2d_fit(torch.from_numpy(img).cuda(), [5.7], [6.2], [4000.0], [50.0], 1.5)
    assert (r['xmin'][0], r['ymax'][0]) == (0, 12) and r['fit_ok'][0]
    assert abs(r['fwhm_x'][0] - 2.0) < 0.1 and abs(r['fwhm_y'][0] - 2.0) < 0.1
    assert abs(r['xc_fit'][0] - 6.2) < 0.05 and abs(r['yc_fit'][0] - 5.7) < 0.05      # the model's x is the row: the kept quirk
    # the largest box, in the bottom right corner of an odd-sized frame
    cap = _lib.GAUSS2D_MAX_BOX
    H, W = cap + 5, cap + 9
    img = synthetic(H, W, H - cap / 2 - 0.3, W - cap / 2 + 0.2, 11.0)
    r = ops.gauss2d_fit(torch.from_numpy(img).cuda(), [W - cap / 2 + 0.2], [H - cap / 2 - 0.3], [4000.0], [50.0], 12.0, box_width=cap)
    assert (r['xmax'][0], r['ymax'][0]) == (W, H) and r['fit_ok'][0] and abs(r['fwhm_x'][0] - 11.0) < 0.2
    with pytest.raises(_lib.ApGpuError) as exc:
        ops.gauss2d_fit(torch.from_numpy(img).cuda(), [40.0], [40.0], [1.0], [0.0], 13.0, box_width=cap + 2)
    assert exc.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError):
        ops.gauss2d_fit(torch.from_numpy(img).cuda(), [3.0], [40.0], [1.0], [0.0], 3.0)
    # no pixel above zero: the weights' mean is over an empty set, nothing is fitted
    dark = -np.abs(synthetic(40, 40, 20, 20, 3.0)) * 0 - 1.0
    r = ops.gauss2d_fit(torch.from_numpy(dark.astype(np.float32)).cuda(), [20.0, 18.5], [20.0, 21.0], [10.0, 10.0], [0.0, 0.0], 3.0)
    assert not r['fit_ok'].any() and np.all(r['ampl_err'] == 0) and np.all(r['circular'])


@pytest.mark.parametrize('negatives', [23, 16, 6])
def test_weights_mean_on_both_sides_of_one_numpy_leaf(negatives):
    """The kernel's only numpy sum is the float32 mean of the positive pixels, which becomes the standard deviation of the
    others.  In the smallest box the op takes (12 pixels: 144 values; odd widths are an error) 23, 16 or 6 border pixels are
    negative, so the mean runs over 121 values (one leaf, with a tail of 1), over 128 (the largest leaf) and over 138 (a
    split tree: 64 + 74).  The fit does not publish the mean; the reduced chi^2 does depend on it: the terms of the negative
    pixels are divided by it, and they are a fifth of the sum or more.  The chi^2 of the device's own answer is recomputed on
    the host with the model's weights (numpy's mean).
    Bound: both sides add the same 144 float64 terms; they differ in the order of the adds (<= 144 eps relative), in exp
    (1 ulp each, argument <= 50 with a few roundings: <= 5e-14 relative in A E <= 4000, i.e. <= 2e-10 in the model) and each
    term moves by 2 |d - m| / sd^2 times that, |d - m| / sd^2 < 1: <= 144 * 4e-10 absolute on a chi^2 of several hundred,
    under 1e-9 relative.  One float32 ulp in the standard deviation of the negative pixels (two ulps of the mean) moves the
    chi^2 by over ten times as much, which the test checks on the host.  The limit of this test: one ulp of the mean is half
    an ulp of that standard deviation and may round away, so only an error of two ulps or more in the sum is sure to show;
    the exact check of the sum itself is tests/test_host_cpu.py::test_np_exact_header_equals_numpy."""
    from astrophotography_amd import ops
    Wb = 12
    img = synthetic(40, 40, 20.3, 19.6, 3.0)
    y0 = x0 = 20 - Wb // 2                                      # the box of a star at (19.6, 20.3): [rint(c) - Wb / 2, ...)
    border = [(0, c) for c in range(Wb)] + [(Wb - 1, c) for c in range(Wb)]
    for dy, dx in border[:negatives]:
        img[y0 + dy, x0 + dx] = -20.0
    got = ops.gauss2d_fit(torch.from_numpy(img).cuda(), [19.6], [20.3], [4000.0], [50.0], 3.0, box_width=Wb)
    assert got['fit_ok'][0] and (int(got['xmin'][0]), int(got['ymin'][0])) == (x0, y0)
    cut = img[y0:y0 + Wb, x0:x0 + Wb]
    var = np.where(cut > 0, cut, np.float32(1))
    count = int((var != 1).sum())
    assert count == Wb * Wb - negatives
    p, _ = mm.params(got, 0, got['xmin'][0], got['ymin'][0])
    model, _ = mm.model_and_jacobian(p, Wb)

    def rchisq(sd):
        return float(np.sum(((cut.astype(np.float64) - model) / sd.astype(np.float64)) ** 2)) / (Wb * Wb - 7)
    sd = mm.weights_of(cut)[1]
    off = np.where(var != 1, sd, np.nextafter(sd, np.float32(np.inf)))             # the negative pixels', one ulp up
    want, moved = rchisq(sd), rchisq(off)
    tol = 1e-9
    print('%d values: rchisq %.17g, host %.17g, relative difference %.2e; one ulp in the others moves it by %.2e' % (
        count, got['rchisq'][0], want, abs(got['rchisq'][0] - want) / want, abs(moved - want) / want))
    assert abs(moved - want) / want > 10 * tol
    assert abs(got['rchisq'][0] - want) / want <= tol


def test_measure_fwhm_and_script_end_to_end(tmp_path):
    yaml = pytest.importorskip('yaml')
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio
    from astrophotography_amd.scripts import ap_find_stars
    c = mm.case(0)
    obj = ap.ApFindStars.from_device(torch.from_numpy(c['img']).cuda(), {'EXPOSURE': 30.0}, search_fwhm=3.0)
    obj._phot_table, obj._full_srclist = c['src'], c['full']                   # the golden tables in place of the search's
    obj._search_fwhm, obj._bg_median = c['init_fwhm'], c['init_bglevel']
    both = obj.measure_fwhm(None)
    rmed, rmad, rn = c['medians']['both']
    assert both[2] == int(rn) and abs(both[0] - rmed) < 1e-4 and obj._nsrcs_fitted == 25
    assert np.array_equal(obj._psf_table['id'], c['res']['id']) and obj.measure_fwhm(None, 'x') == obj._fwhm_x
    assert 'psbl_sat' in c['src']                                              # the caller's table keeps its columns

    frame, srclist, report = tmp_path / 'frame.fits', tmp_path / 'stars.fits', tmp_path / 'quality.yaml'
    hdr = fitsio.Header()
    for key, v in (('EXPOSURE', 30.0), ('FOCALLEN', 1000.0), ('XPIXSZ', 5.0), ('YPIXSZ', 5.0)):
        hdr[key] = v
    fitsio.write(str(frame), c['img'], hdr)
    assert ap_find_stars.main([str(frame), str(srclist), '-q', '-l', 'ERROR', '--quality_report', str(report)]) == 0
    rep = yaml.safe_load(report.read_text())
    assert rep['psf_info']['num_fit'] > 5 and abs(rep['psf_info']['fwhm_xandy']['fwhm_val_pix'] - rmed) < 0.1
    assert rep['psf_info']['fwhm_xandy']['fwhm_val_arcs'] > 0
    psf, _, _ = fitsio.read_table(str(srclist), 'AP_L1PSF')
    assert len(psf['fwhm_x']) == rep['psf_info']['num_fit'] and set(('xc_fit', 'fit_ok', 'region', 'rchisq')) <= set(psf)
    _, _, prim = fitsio.read_table(str(srclist), 'AP_L1MAG')
    assert abs(prim['AP_FWHM'] - rep['psf_info']['fwhm_xandy']['fwhm_val_pix']) < 1e-5 and prim['AP_NFIT'] == rep['psf_info']['num_fit']
