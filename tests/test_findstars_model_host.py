"""F6 star finder on the host: the self-checks of the CPU model (tests/findstars_model.py), golden group G16 through its annulus
clip, the FITS table round trip, the script's argument parser and the argument checks of the new C entry points.  No GPU."""
import json
import math

import numpy as np
import pytest

from tests import findstars_model as fm
from tests.util import assert_biteq, load_golden, ulp_diff

FWHMS = (3.0, 4.3, 7.9)


def _field(H, W, seed, nstars=12, sky=200.0, noise=4.0):
    """Flat sky + Gaussian stars + seeded noise, quantised to multiples of 1/8."""
    rng = np.random.default_rng(seed)
    img = rng.normal(sky, noise, (H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(nstars):
        cy, cx, a, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(100, 5000), rng.uniform(1.0, 2.2)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return (np.rint(img * 8.0) / 8.0).astype(np.float32)


@pytest.mark.parametrize('fwhm,side', [(3.0, 5), (4.3, 5), (7.9, 11)])
def test_kernel_zero_sum_and_relerr(fwhm, side):
    k = fm.daofind_kernel(fwhm)
    K, fp = k['K'], k['fp']
    assert K.shape == (side, side) and k['R'] == side // 2
    assert k['sigma'] == fwhm / (2.0 * math.sqrt(2.0 * math.log(2.0)))
    assert fp[k['R'], k['R']] and k['npixels'] == fp.sum() and np.array_equal(fp, fp.T) and np.array_equal(fp, fp[::-1])
    assert np.all(K[~fp] == 0.0)
    # zero sum over the footprint: |sum| is a few roundings of the largest weight
    assert abs(K.sum()) <= 8 * k['npixels'] * np.finfo(np.float64).eps * np.abs(K).max()
    # K = (G - mean G) / denom on the footprint: sum(K * G) = 1 (a star of unit height convolves to 1) and relerr^2 = sum(K^2)
    gm = k['g'] * fp
    assert abs((K * gm).sum() - 1.0) < 1e-13
    assert abs(k['relerr'] ** 2 - (K * K).sum()) < 1e-13 * k['relerr'] ** 2
    assert np.array_equal(K, K.T) and np.array_equal(K, K[::-1, ::-1])


def test_ops_kernel_is_the_models_kernel():
    """The package builds its weights with the model's formula: every table bit-equal (no GPU needed to build them)."""
    from astrophotography_amd import ops
    for fwhm in FWHMS + (2.0, 11.3):
        a, b = fm.daofind_kernel(fwhm), ops.daofind_kernel(fwhm)
        for key in ('K', 'tables', 'quad'):
            assert_biteq(np.asarray(a[key], np.float64), np.asarray(b[key], np.float64), key)
        assert np.array_equal(a['fp'], b['fp'])
        assert (a['R'], a['npixels'], a['relerr'], a['sigma'], a['p']) == (b['R'], b['npixels'], b['relerr'], b['sigma'], b['p'])
        assert a['consts'] == b['consts']
    assert ops.DAOFIND_RECORD == fm.REC
    assert ops.aperture_radii(3.0) == fm.aperture_radii(3.0) == (6.0, 6.0, 9.0)
    assert ops.aperture_radii(7.9) == fm.aperture_radii(7.9) == (16.0, 16.0, 24.0)


# Largest difference between the model's convolution (row-major tap order, every tap) and scipy.ndimage.convolve(mode='constant',
# cval=0) on the same float32 input, in float32 ulps, over the three kernels and two fields below: 0 (recorded in DESIGN 4.12).
SCIPY_CONVOLVE_MAX_ULP = 0


@pytest.mark.parametrize('fwhm', FWHMS)
def test_convolve_agrees_with_scipy(fwhm):
    """Model vs scipy.ndimage.convolve on the same float32 input.  Measured largest difference: 0 float32 ulps (scipy accumulates
    the same float64 products; where its order differs the float32 rounding absorbs it on these fields).  Asserted: no more than
    the recorded value."""
    from scipy import ndimage
    k = fm.daofind_kernel(fwhm)
    worst = 0
    for shape, seed in (((97, 131), 1), ((64, 200), 2)):
        d = fm.subtract_bg(_field(*shape, seed), 200.0)
        mine = fm.convolve(d, k['K'])
        ref = ndimage.convolve(d, k['K'], mode='constant', cval=0.0)
        assert ref.dtype == np.float32
        worst = max(worst, int(ulp_diff(mine, ref).max()))
    print('fwhm %.1f: model vs scipy convolution, max %d float32 ulp' % (fwhm, worst))
    assert worst <= SCIPY_CONVOLVE_MAX_ULP


def test_find_peaks_square_form_is_scipys_maximum_filter():
    from scipy import ndimage
    img = _field(64, 200, 3)
    for box in (12, 31, 5):
        thr = 400.0
        mx = ndimage.maximum_filter(img, size=box, mode='constant', cval=0.0)
        ref = np.flatnonzero((img == mx) & (img > thr))
        got = fm.find_peaks(img, np.ones((box, box), bool), thr)
        assert np.array_equal(got, ref) and len(ref) > 3
    k = fm.daofind_kernel(3.0)
    mx = ndimage.maximum_filter(img, footprint=k['fp'], mode='constant', cval=0.0)
    assert np.array_equal(fm.find_peaks(img, k['fp'], 300.0), np.flatnonzero((img == mx) & (img > 300.0)))


def test_circle_overlap_against_subsampling_and_total_area():
    """The exact overlap areas against a sub-sampled count, to 1e-3 per pixel, and their sum against pi r^2 to 1e-12.

    A 64 x 64 count cannot serve as the yardstick of a 1e-3 bound: its own error reaches 1.1e-3 (r = 6 about (20, 19)), 1.5e-3
    (r = 9 about (21.37, 18.81)) and 2.4e-3 (r = 16 about (22.113, 20.004)) on the pixels where the circle runs nearly parallel
    to the sample rows, and shrinks as the count is refined (2.6e-4 at 256 x 256, 1.2e-4 at 512 x 512) - the areas are the exact
    ones.  So the bound stays 1e-3 and the count is refined where it matters: every pixel the circle's edge crosses is compared
    with a 256 x 256 count, every other pixel (area exactly 0 or 1) with the 64 x 64 count, which must then agree exactly."""
    H, W = 40, 44
    for cx, cy, r in ((20.0, 19.0, 6.0), (20.5, 19.5, 6.0), (21.37, 18.81, 9.0), (22.113, 20.004, 16.0), (3.2, 37.9, 6.0),
                      (20.25, 19.75, 0.3), (20.0, 19.0, 0.5)):
        ov = fm.circle_overlap(cx, cy, r, H, W)
        assert ov.min() >= 0.0 and ov.max() <= 1.0

        def count(n, i0, i1, j0, j1):
            s = (np.arange(n) + 0.5) / n - 0.5
            yy = (np.arange(i0, i1)[:, None] + s[None, :]).reshape(-1)
            xx = (np.arange(j0, j1)[:, None] + s[None, :]).reshape(-1)
            inside = ((xx[None, :] - cx) ** 2 + (yy[:, None] - cy) ** 2) <= r * r
            return inside.reshape(i1 - i0, n, j1 - j0, n).mean(axis=(1, 3))
        sub64 = count(64, 0, H, 0, W)
        edge = (ov > 0.0) & (ov < 1.0)
        assert edge.any() and np.array_equal(sub64[~edge], ov[~edge])
        worst = 0.0
        for i, j in zip(*np.nonzero(edge)):
            worst = max(worst, abs(ov[i, j] - count(256, i, i + 1, j, j + 1)[0, 0]))
        print('circle (%g, %g) r %g: %d edge pixels, max |area - 256^2 count| %.2e (64^2 count: %.2e)'
              % (cx, cy, r, edge.sum(), worst, np.abs(ov - sub64).max()))
        assert worst <= 1e-3, (cx, cy, r, worst)
        if r <= min(cx, cy, W - 1 - cx, H - 1 - cy):
            assert abs(ov.sum() - math.pi * r * r) <= 1e-12, (cx, cy, r, ov.sum() - math.pi * r * r)


def test_g16_annulus_clip_equals_astropy():
    """Every G16 vector through the model's annulus clip: the median (bkg_median), mean and std equal astropy's, compared as
    float32, exactly."""
    g = load_golden('g16_annulus.npz')
    meta = json.loads(str(g['_meta']))
    assert len(meta) == 30
    names = {m['name'] for m in meta}
    assert {'two_values', 'all_equal_150', 'nan_150', 'wing_1004', 'all_nan_12'} <= names
    for m in meta:
        v = g['c%d_values' % m['case']]
        assert v.dtype == np.float32 and 1 <= v.size <= 1100
        ref = g['c%d_stats' % m['case']].astype(np.float32)
        got = np.array(fm.annulus_clip(v), np.float32)
        assert_biteq(got, ref, m['name'])


def test_table_round_trip(tmp_path):
    from astrophotography_amd import fitsio
    g = load_golden('g16_annulus.npz')
    cols = {'id': np.arange(1, 8, dtype=np.int32), 'xcenter': np.linspace(0.5, 90.25, 7), 'peak_adu': np.arange(7, dtype=np.float32) * 3.5,
            'psbl_sat': np.arange(7) % 3 == 0, 'npix': np.full(7, 2 ** 40 + 3, np.int64)}
    cols['xcenter'][3] = np.nan
    assert [fitsio._tform_of(v) for v in cols.values()] == ['J', 'D', 'E', 'L', 'K']
    # the formats astropy read back from a file of this writer (recorded by the golden generator)
    assert json.loads(str(g['table_formats'])) == ['J', 'D', 'D', 'D', 'E', 'L', 'K']
    kw = {'IMG_FILE': ('frame.fits', 'Name of image file searched for stars'), 'AP_NDET': (7, 'Number of sources detected in the image.'),
          'AP_BGSTD': (4.25, '[ADU] Std dev of source-masked background level')}
    path = tmp_path / 't.fits'
    fitsio.write_table(str(path), [('AP_XYPOS', {'X': cols['xcenter'] + 1.0}, {'X': 'pix'}, [('COMMENT', 'one-based')]),
                                   ('AP_L1MAG', cols, {'xcenter': 'pix'}, None)], header=kw)
    raw = path.read_bytes()
    assert len(raw) % 2880 == 0 and raw[:6] == b'SIMPLE'
    got, eh, prim = fitsio.read_table(str(path), 'ap_l1mag')
    assert list(got) == list(cols)
    for n, v in cols.items():
        assert got[n].dtype == v.dtype and np.array_equal(got[n], v, equal_nan=v.dtype.kind == 'f'), n
    assert eh['NAXIS2'] == 7 and eh['NAXIS1'] == 4 + 8 + 4 + 1 + 8 and eh['TFIELDS'] == 5 and eh['TUNIT2'] == 'pix'
    assert [eh['TTYPE%d' % i] for i in range(1, 6)] == list(cols) and [eh['TFORM%d' % i] for i in range(1, 6)] == ['J', 'D', 'E', 'L', 'K']
    assert prim['AP_NDET'] == 7 and prim['AP_BGSTD'] == 4.25 and prim['IMG_FILE'] == 'frame.fits' and prim['NAXIS'] == 0
    xy, _, _ = fitsio.read_table(str(path), 'AP_XYPOS')
    assert np.array_equal(xy['X'], cols['xcenter'] + 1.0, equal_nan=True)
    with pytest.raises(KeyError):
        fitsio.read_table(str(path), 'NOPE')
    empty = tmp_path / 'e.fits'
    fitsio.write_table(str(empty), [('AP_L1MAG', {k: v[:0] for k, v in cols.items()}, None, None)])
    got, eh, _ = fitsio.read_table(str(empty), 'AP_L1MAG')
    assert eh['NAXIS2'] == 0 and all(len(v) == 0 for v in got.values())
    with pytest.raises(TypeError):
        fitsio.write_table(str(empty), [('X', {'c': np.zeros(3, np.complex64)}, None, None)])


def test_script_defaults():
    from astrophotography_amd.scripts import ap_find_stars as s
    a = s.command_line_opts(['img.fits', 'stars.fits'])
    assert (a.fits_image, a.source_list) == ('img.fits', 'stars.fits')
    assert (a.search_fwhm, a.search_nsigma, a.bitdepth, a.sat_frac) == (3.0, 7.0, 16, 0.80)
    assert (a.max_sources, a.fits_extension, a.retain_saturated, a.ds9, a.quiet, a.loglevel) == (None, 0, False, None, False, 'INFO')
    assert (a.plotfile, a.quality_report, a.fwhm_plot) == (None, None, None)
    a = s.command_line_opts(['i.fits', 'o.fits', '--search_fwhm', '4.5', '--search_nsigma', '5', '--bitdepth', '14', '--sat_frac', '0.7',
                             '-m', '50', '-e', '0', '--retain_saturated', '-d', 'r.reg', '-q', '-l', 'DEBUG', '--plotfile', 'p.png'])
    assert (a.search_fwhm, a.search_nsigma, a.bitdepth, a.sat_frac, a.max_sources) == (4.5, 5.0, 14, 0.7, 50)
    assert a.retain_saturated and a.ds9 == 'r.reg' and a.quiet and a.loglevel == 'DEBUG' and a.plotfile == 'p.png'


def test_class_is_exported_lazily_and_refuses_the_out_of_scope_methods():
    import astrophotography_amd as ap
    assert 'ApFindStars' in ap.__all__
    cls = ap.ApFindStars
    assert (cls.GOOD, cls.INPUT_ERROR) == (0, 1)
    obj = cls.__new__(cls)
    for name, args in (('measure_fwhm', ('p.png',)), ('plot_image', ('p.png',)), ('write_quality_report', ('q.yaml',))):
        with pytest.raises(NotImplementedError):
            getattr(obj, name)(*args)


def test_capi_rejects_bad_arguments_before_device_work():
    import ctypes as C
    from astrophotography_amd import _lib
    lib = _lib.load()
    d = C.c_void_p(16)                         # never dereferenced: validation comes first
    E, U = _lib.E_INVAL, _lib.E_UNSUPPORTED
    assert lib.apgpu_daofind_convolve_f32(None, 8, 8, d, 2, 0.0, d, None) == E
    assert lib.apgpu_daofind_convolve_f32(d, 0, 8, d, 2, 0.0, d, None) == E
    assert lib.apgpu_daofind_convolve_f32(d, 8, 8, d, 0, 0.0, d, None) == E
    assert lib.apgpu_daofind_convolve_f32(d, 8, 8, d, 13, 0.0, d, None) == U
    assert b'fwhm too large' in lib.apgpu_last_error()
    assert lib.apgpu_local_peaks_f32(d, 8, 8, None, 3, 3, 1.0, None, 0, d, 4, d, None) == E
    assert lib.apgpu_local_peaks_f32(d, 8, 8, d, 3, 3, 1.0, None, 0, None, 4, d, None) == E
    assert lib.apgpu_local_peaks_f32(d, 8, 8, d, 3, 3, 1.0, None, 0, d, -1, d, None) == E
    assert lib.apgpu_local_peaks_f32(d, 8, 8, d, 65, 3, 1.0, None, 0, d, 4, d, None) == E
    assert lib.apgpu_local_peaks_f32(d, 8, 8, d, 3, 3, 1.0, None, -1, d, 4, d, None) == E
    assert lib.apgpu_local_peaks_f32(d, 1 << 16, 1 << 15, d, 3, 3, 1.0, None, 0, d, 4, d, None) == U
    assert lib.apgpu_daofind_measure(d, d, 8, 8, d, 0, 2, 0.0, d, d, d, d, d, None) == 0          # nothing to do
    assert lib.apgpu_daofind_measure(d, d, 8, 8, None, 3, 2, 0.0, d, d, d, d, d, None) == E
    assert lib.apgpu_daofind_measure(d, d, 8, 8, d, 3, 13, 0.0, d, d, d, d, d, None) == U
    assert lib.apgpu_aperture_phot_f32(d, 8, 8, d, d, 0, 6.0, 6.0, 9.0, 3.0, 5, d, d, d, d, None) == 0
    assert lib.apgpu_aperture_phot_f32(d, 8, 8, None, d, 2, 6.0, 6.0, 9.0, 3.0, 5, d, d, d, d, None) == E
    assert lib.apgpu_aperture_phot_f32(d, 8, 8, d, d, 2, 6.0, 9.0, 9.0, 3.0, 5, d, d, d, d, None) == E
    assert lib.apgpu_aperture_phot_f32(d, 8, 8, d, d, 2, 0.0, 6.0, 9.0, 3.0, 5, d, d, d, d, None) == E
    # the annulus must fit on chip: r_in 30, r_out 45 does, r_in 32, r_out 48 does not
    assert lib.apgpu_aperture_phot_f32(d, 8, 8, d, d, 2, 32.0, 32.0, 48.0, 3.0, 5, d, d, d, d, None) == U
    assert b'fwhm too large' in lib.apgpu_last_error()
    assert lib.apgpu_version() == 130
