"""F11 on the GPU (csrc/continuum.hip) against the NumPy model tests/continuum_model.py: the blur and the combine
bit for bit, the moments to the worst-case bound of two summation orders, and ApContinuumSubtract / ap_continuum_subtract end to
end on the synthetic scene of tests/test_continuum_model_host.py."""
import os

import numpy as np
import pytest

from tests import continuum_model as cm

pytestmark = pytest.mark.gpu

F = np.float32
TH, TW = 32, 64                                                       # APGPU_BLUR_TILE_H, APGPU_BLUR_TILE_W
HEIGHTS = (1, TH - 1, TH, TH + 1, 2 * TH + 1)
WIDTHS = (1, TW - 1, TW, TW + 1, 2 * TW + 7, 2 * TW + 4)              # ragged multi-tile; a multi-tile multiple of 4 (wide loads)
RADII = (0, 1, 2, 7, 32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(got, want, what=''):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, 'NaN positions differ at', np.argwhere(gn != wn)[:5].tolist())
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~wn
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


def _taps(R):
    return cm.gauss_taps(0.0 if R == 0 else R / 4.0, R)


def _image(rng, H, W, holes):
    img = rng.normal(100.0, 30.0, (H, W)).astype(F)
    if holes == 'isolated':
        bad = rng.random((H, W)) < 0.07
        img[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(bad.sum()))
    elif holes == 'lines':
        img[H // 2, :] = np.nan
        img[:, W // 3] = np.inf
    elif holes == 'block':
        img[H // 4:H // 4 + 40, W // 4:W // 4 + 70] = np.nan             # larger than the R = 7 kernel: M < min_weight inside
    elif holes == 'seams':
        for y in range(TH - 1, H, TH):
            img[y:y + 2, ::3] = np.nan
        for x in range(TW - 1, W, TW):
            img[::2, x:x + 2] = -np.inf
        img[0, 0] = img[0, -1] = img[-1, 0] = img[-1, -1] = np.nan
        img[:2, :2] = np.nan
    elif holes == 'all':
        img[:] = np.nan
    return img


def _check_blur(img, R, mw=0.5, what=''):
    from astrophotography_amd import ops
    taps = _taps(R)
    got = ops.gauss_blur(_dev(img), taps, mw).cpu().numpy()
    _same_bits(got, cm.gauss_blur(img, taps, mw), '%s %s R %d min_weight %g' % (what, img.shape, R, mw))


@pytest.mark.parametrize('R', RADII)
def test_blur_shapes(R):
    """Every height x width that straddles a tile edge, clean and with isolated holes."""
    rng = np.random.default_rng(100 + R)
    for H in HEIGHTS:
        for W in WIDTHS:
            _check_blur(_image(rng, H, W, 'isolated' if (H + W) % 2 else 'none'), R, what='shapes')
    _check_blur(_image(rng, 5, 7, 'isolated'), R, what='R larger than the image')


@pytest.mark.parametrize('holes', ['lines', 'block', 'seams', 'all'])
def test_blur_holes(holes):
    rng = np.random.default_rng(7)
    img = _image(rng, 2 * TH + 9, 2 * TW + 13, holes)
    for R in (0, 2, 7, 32):
        for mw in (0.0, 0.5, 1.0):
            _check_blur(img, R, mw, holes)

def test_blur_gaussian_sigma_and_errors():
    import torch
    from astrophotography_amd import ops
    rng = np.random.default_rng(5)
    img = _image(rng, 70, 130, 'isolated')
    for sigma in (0.93, 2.5):
        got = ops.gauss_blur(_dev(img), sigma).cpu().numpy()
        _same_bits(got, cm.gauss_blur(img, cm.gauss_taps(sigma)), 'sigma %g' % sigma)
        assert np.array_equal(ops.gauss_taps(sigma), cm.gauss_taps(sigma))
    with pytest.raises(ValueError, match='radius'):
        ops.gauss_blur(_dev(img), 8.5)
    with pytest.raises(ValueError):
        ops.gauss_blur(torch.zeros((4, 4)), 1.0)                         # a CPU tensor
    from astrophotography_amd import _lib
    import ctypes as C
    d = _dev(img)
    taps = np.ones(67) / 67.0
    rc = _lib.load().apgpu_gauss_blur_norm_f32(C.c_void_p(d.data_ptr()), 70, 130, taps.ctypes.data_as(C.POINTER(C.c_double)), 33, 0.5,
                                               C.c_void_p(torch.empty_like(d).data_ptr()), None)
    assert rc == _lib.E_UNSUPPORTED


# ---- moments -----------------------------------------------------------------------------------------------------------------
def _moment_case(rng, shape, nonfinite=True):
    c = rng.normal(50.0, 20.0, shape).astype(F)
    n = (F(0.1) * c + F(2.0) + rng.normal(0.0, 1.0, shape).astype(F)).astype(F)
    if nonfinite and n.size > 4:
        k = max(1, n.size // 20)
        n.ravel()[rng.choice(n.size, k, replace=False)] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), k)
        c.ravel()[rng.choice(n.size, k, replace=False)] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), k)
    mask = (rng.random(shape) < 0.1).astype(np.uint8)
    return n, c, mask


def _check_moments(n, c, mask, s, b, lo, hi, what):
    from astrophotography_amd import ops
    dn, dc, dm = _dev(n), _dev(c), None if mask is None else _dev(mask)
    got = ops.pair_moments(dn, dc, s, b, lo, hi, dm).cpu().numpy()
    again = ops.pair_moments(dn, dc, s, b, lo, hi, dm).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), (what, 'two runs differ')
    want = cm.pair_moments(n, c, s, b, lo, hi, mask)
    absum = cm.moment_terms_abs(n, c, s, b, lo, hi, mask)
    assert got[0] == want[0], (what, got[0], want[0])
    cnt = want[0]
    for k in range(1, 6):
        bound = 2.0 * cnt * 2.0 ** -53 * absum[k]                       # worst case of two summation orders of cnt terms
        assert abs(got[k] - want[k]) <= bound, (what, k, got[k], want[k], bound)
    return got


@pytest.mark.parametrize('shape', [(1, 1), (3, 4), (67, 259), (257, 1030)])
def test_moments(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    n, c, mask = _moment_case(rng, shape)
    for m in (None, mask):
        _check_moments(n, c, m, 0.0, 0.0, -np.inf, np.inf, 'unclipped')
        _check_moments(n, c, m, 0.1, 2.0, -1.5, 1.0, 'finite bounds')
        got = _check_moments(n, c, m, 0.1, 2.0, 1e30, 2e30, 'bounds that exclude everything')
        assert np.array_equal(got, np.zeros(6))
    # an unaligned view: the same bits as the aligned copy (the order depends on the pixel count alone)
    if n.size > 8:
        import torch
        from astrophotography_amd import ops
        flat_n, flat_c = _dev(np.concatenate([[F(0)], n.ravel()])), _dev(np.concatenate([[F(0)], c.ravel()]))
        a = ops.pair_moments(flat_n[1:].view(1, -1), flat_c[1:].view(1, -1), 0.1, 2.0, -1.5, 1.0).cpu().numpy()
        b = ops.pair_moments(_dev(n).view(1, -1), _dev(c).view(1, -1), 0.1, 2.0, -1.5, 1.0).cpu().numpy()
        assert flat_n[1:].data_ptr() % 16 != 0 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        del torch


def test_moments_inclusive_bounds():
    """Residuals placed exactly on lo and hi are kept; one ulp outside they are not."""
    c = np.array([[0.0, 0.0, 0.0, 0.0, 2.0, 4.0]], F)
    s, b = 0.5, 1.0                                                      # s c + b = 1, 1, 1, 1, 2, 3, exact
    n = np.array([[0.25, np.nextafter(F(0.25), F(0)), 1.25, np.nextafter(F(1.25), F(2)), 2.0, 2.25]], F)
    exact = n.astype(np.float64) - (s * c.astype(np.float64) + b)
    assert exact[0, 0] == -0.75 and exact[0, 2] == 0.25 and exact[0, 1] < -0.75 and exact[0, 3] > 0.25 and exact[0, 5] == -0.75
    got = _check_moments(n, c, None, s, b, -0.75, 0.25, 'on the bounds')
    assert got[0] == 4.0 and got[1] == 6.0 and got[2] == 0.25 + 1.25 + 2.0 + 2.25


# ---- combine -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [1, 5, 1024, 4099])
def test_combine(size):
    from astrophotography_amd import ops
    rng = np.random.default_rng(size)
    x = rng.normal(0, 100, size).astype(F)
    y = rng.normal(0, 100, size).astype(F)
    if size >= 5:
        x[0], x[1], y[2], y[3] = np.nan, np.inf, -np.inf, np.nan
    x[-1] = F(-0.0)
    for ca, cb, c0 in ((1.0, -0.083, -0.4), (0.3, 1.7, 0.0), (-1.0, 0.0, -0.0), (1.0, -1.0, 0.0)):
        got = ops.linear_combine(_dev(x), _dev(y), ca, cb, c0).cpu().numpy()
        _same_bits(got, cm.linear_combine(x, y, ca, cb, c0), 'combine %s' % ((ca, cb, c0),))
        got = ops.linear_combine(_dev(x), None, ca, cb, c0).cpu().numpy()
        _same_bits(got, cm.linear_combine(x, None, ca, cb, c0), 'combine y NULL %s' % ((ca, cb, c0),))
    # an unaligned view takes the single-value path
    xx, yy = _dev(np.concatenate([[F(0)], x])), _dev(np.concatenate([[F(0)], y]))
    _same_bits(ops.linear_combine(xx[1:], yy[1:], 1.0, -0.083, -0.4).cpu().numpy(), cm.linear_combine(x, y, 1.0, -0.083, -0.4), 'unaligned')
    z = cm.linear_combine(np.array([-0.0], F), None, 1.0, 0.0, -0.0)
    assert np.signbit(z[0]) and np.signbit(ops.linear_combine(_dev(np.array([-0.0], F)), None, 1.0, 0.0, -0.0).cpu().numpy()[0])


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    sc = cm.scene()
    n, c, info = cm.psf_match(sc['n'], sc['c'], sc['fwhm_n'], sc['fwhm_c'])
    sc.update(nm=n, cm=c, info=info, fit=cm.continuum_scale_pixels(n, c))
    return sc


def test_subtract_equals_model(scene):
    import astrophotography_amd as ap
    cs = ap.ApContinuumSubtract('ERROR', method='pixels', keep_matched=True)
    r = cs.subtract(_dev(scene['n']), _dev(scene['c']), fwhm=(scene['fwhm_n'], scene['fwhm_c']))
    rep, fit = r['report'], scene['fit']
    assert rep['blurred'] == scene['info']['blurred'] == 'continuum' and rep['taps'] == len(scene['info']['taps'])
    assert rep['sigma_k'] == scene['info']['sigma_k']
    _same_bits(r['continuum_matched'].cpu().numpy(), scene['cm'], 'matched continuum')
    _same_bits(r['narrow_matched'].cpu().numpy(), scene['nm'], 'matched narrow')
    assert rep['iterations'] == fit['iterations'] and rep['n_pixels'] == fit['n']
    print('s %.12g model %.12g; b %.12g model %.12g' % (rep['scale'], fit['s'], rep['offset'], fit['b']))
    assert abs(rep['scale'] - fit['s']) <= 1e-9 * abs(fit['s']) and abs(rep['offset'] - fit['b']) <= 1e-9 * abs(fit['b'])
    _same_bits(r['image'].cpu().numpy(), cm.subtract(scene['nm'], scene['cm'], rep['scale'], rep['offset']), 'line image')
    assert abs(rep['scale'] - scene['s']) <= 5 * rep['se_scale'] and abs(rep['offset'] - scene['b']) <= 5 * rep['se_offset']


def test_subtract_stars_method(scene):
    import astrophotography_amd as ap
    from astrophotography_amd import ops
    cs = ap.ApContinuumSubtract('ERROR', method='stars', keep_matched=True)
    r = cs.subtract(_dev(scene['n']), _dev(scene['c']), fwhm=(scene['fwhm_n'], scene['fwhm_c']), stars=scene['xy'])
    rep = r['report']
    xy = scene['xy']
    fn = ops.aperture_photometry(r['narrow_matched'], xy[:, 0], xy[:, 1], fwhm=3.4)['aperture_sum'].cpu().numpy()
    fc = ops.aperture_photometry(r['continuum_matched'], xy[:, 0], xy[:, 1], fwhm=3.4)['aperture_sum'].cpu().numpy()
    want = cm.scale_from_fluxes(fn, fc)
    assert rep['method'] == 'stars' and rep['scale'] == want['s'] and rep['n_stars'] == want['n_used']
    assert abs(rep['scale'] - scene['s']) <= 5 * want['se_s']
    fixed = cm.continuum_scale_pixels(scene['nm'], scene['cm'], fixed_scale=rep['scale'])
    assert abs(rep['offset'] - fixed['b']) <= 1e-9 * abs(fixed['b'])
    assert 0 <= rep['star_residual_frac'] < 0.05
    with pytest.raises(RuntimeError, match='usable stars'):
        cs.subtract(_dev(scene['n']), _dev(scene['c']), fwhm=(3.4, 2.6), stars=xy[:3])
    with pytest.raises(RuntimeError, match='one pixel grid'):
        cs.subtract(_dev(scene['n']), _dev(scene['c'][:, :-1]), fwhm=(3.4, 2.6))
    with pytest.raises(RuntimeError, match='FWHM'):
        cs.subtract(_dev(scene['n']), _dev(scene['c']), fwhm=(2.0, 25.0))


def test_iteration_stops_by_itself():
    """A field small enough that the count stands still before maxiters: the kernel's loop ends in the model's round."""
    from astrophotography_amd import ops
    rng = np.random.default_rng(21)
    c = rng.normal(30.0, 5.0, (40, 50)).astype(F)
    n = (F(0.083) * c + F(0.4) + rng.normal(0.0, 0.5, c.shape).astype(F)).astype(F)
    want = cm.continuum_scale_pixels(n, c, maxiters=50)
    got = ops.continuum_scale_pixels(_dev(n), _dev(c), maxiters=50)
    assert 1 <= want['iterations'] < 50 and got['iterations'] == want['iterations'] and got['n'] == want['n']
    assert abs(got['s'] - want['s']) <= 1e-9 * abs(want['s']) and abs(got['b'] - want['b']) <= 1e-9 * abs(want['b'])
    assert (got['lo'], got['hi']) != (-np.inf, np.inf) and abs(got['lo'] - want['lo']) <= 1e-9 * abs(want['lo'])


def test_given_scale_is_held_while_the_offset_is_fitted(scene):
    """scale alone: whatever the method, b is the pixel fit with that s held."""
    import astrophotography_amd as ap
    want = cm.continuum_scale_pixels(scene['nm'], scene['cm'], fixed_scale=0.08)
    for method in ('stars', 'pixels', None):
        r = ap.ApContinuumSubtract('ERROR', method=method).subtract(_dev(scene['n']), _dev(scene['c']), fwhm=(3.4, 2.6), stars=scene['xy'],
                                                                   scale=0.08)
        rep = r['report']
        assert rep['scale'] == 0.08 and rep['method'] == 'pixels' and rep['n_pixels'] == want['n']
        assert abs(rep['offset'] - want['b']) <= 1e-9 * abs(want['b'])
        assert 'narrow_matched' not in r
    r = ap.ApContinuumSubtract('ERROR').subtract(_dev(scene['n']), _dev(scene['c']), fwhm=(3.4, 2.6), keep_matched=True)
    assert 'narrow_matched' in r and 'continuum_matched' in r


def test_headline_command_measures_fwhm_and_fits_pixels(scene, tmp_path):
    """ap_continuum_subtract ha.fits r.fits line.fits, nothing else given: the FWHMs are measured from the images, the method is the
    pixel fit (no star list was given; the stars found on the way only serve the residual figure), and the cards say so.  The
    scene's stars are sampled Gaussians, the very model that is fitted, so the measured FWHM differs from the truth by noise alone:
    0.1 pixel (3 to 4 %) is far outside that and far inside the 0.8 pixel between the two images."""
    from astrophotography_amd import fitsio
    from astrophotography_amd.scripts import ap_continuum_subtract as script
    nf, cf, out = str(tmp_path / 'ha.fits'), str(tmp_path / 'r.fits'), str(tmp_path / 'line.fits')
    fitsio.write(nf, scene['n'])
    fitsio.write(cf, scene['c'])
    assert script.main([nf, cf, out, '-l', 'ERROR']) == 0
    data, h = fitsio.read(out)
    print('measured FWHM: narrow %.4f (3.4), continuum %.4f (2.6); s %.6f b %.5f' % (h['CSUBFWN'], h['CSUBFWC'], h['CSUBSCAL'], h['CSUBOFF']))
    assert h['CSUBMETH'] == 'PIXELS'
    assert abs(h['CSUBFWN'] - 3.4) <= 0.1 and abs(h['CSUBFWC'] - 2.6) <= 0.1
    plan = cm.psf_match_plan(h['CSUBFWN'], h['CSUBFWC'])
    assert plan[0] == 'continuum' and h['CSUBKSIG'] == plan[1]
    # the model, given the measured FWHMs, gives the same fit and the same image
    nm, cmm, _ = cm.psf_match(scene['n'], scene['c'], h['CSUBFWN'], h['CSUBFWC'])
    fit = cm.continuum_scale_pixels(nm, cmm)
    assert h['CSUBNPIX'] == fit['n'] and h['CSUBITER'] == fit['iterations']
    assert abs(h['CSUBSCAL'] - fit['s']) <= 1e-9 * abs(fit['s']) and abs(h['CSUBOFF'] - fit['b']) <= 1e-9 * abs(fit['b'])
    _same_bits(np.asarray(data, F), cm.subtract(nm, cmm, h['CSUBSCAL'], h['CSUBOFF']), 'headline image')
    # Truth: the formal errors do not know that the FWHMs were measured.  Stars carry the fit's leverage, and for Gaussian stars
    # the slope of N' on C' is s 2 sc^2 / (sn^2 + sc^2) (sn, sc the matched widths), s (1 + e) to first order when the matched
    # widths differ by the fraction e; e is at most the sum of the two relative FWHM errors.  Bound: that first-order term doubled,
    # plus the 5 formal errors; the offset follows as the mean continuum level times the change of s.
    e = abs(h['CSUBFWN'] / 3.4 - 1.0) + abs(h['CSUBFWC'] / 2.6 - 1.0)
    ds = 2.0 * e * scene['s']
    print('relative FWHM error %.2e: s off by %.2e (bound %.2e + %.2e), b off by %.2e (bound %.2e + %.2e)' % (
        e, h['CSUBSCAL'] - scene['s'], ds, 5 * fit['se_s'], h['CSUBOFF'] - scene['b'], ds * fit['cbar'], 5 * fit['se_b']))
    assert abs(h['CSUBSCAL'] - scene['s']) <= ds + 5 * fit['se_s']
    assert abs(h['CSUBOFF'] - scene['b']) <= ds * fit['cbar'] + 5 * fit['se_b']
    # the class: the same choice, and the stars met while measuring give the residual figure
    import astrophotography_amd as ap
    rep = ap.ApContinuumSubtract('ERROR').subtract(_dev(scene['n']), _dev(scene['c']))['report']
    assert rep['method'] == 'pixels' and rep['n_stars'] == 0 and rep['fwhm_narrow'] == h['CSUBFWN'] and rep['scale'] == h['CSUBSCAL']
    assert 0 <= rep['star_residual_frac'] < 0.05
    # method 'stars' without a list: the stars are searched on the matched continuum image
    rs = ap.ApContinuumSubtract('ERROR', method='stars').subtract(_dev(scene['n']), _dev(scene['c']), fwhm=(3.4, 2.6))['report']
    assert rs['method'] == 'stars' and rs['n_stars'] >= 50 and abs(rs['scale'] - scene['s']) <= 5 * rs['se_scale']


def test_files_and_script(scene, tmp_path):
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio
    from astrophotography_amd.scripts import ap_continuum_subtract as script
    hdr = fitsio.Header()
    hdr['FILTER'] = 'Ha'
    nf, cf = str(tmp_path / 'ha.fits'), str(tmp_path / 'r.fits')
    fitsio.write(nf, scene['n'], header=hdr)
    fitsio.write(cf, scene['c'])
    out = str(tmp_path / 'line.fits')
    rep = ap.ApContinuumSubtract('ERROR').subtract_files(nf, cf, out, fwhm=(3.4, 2.6))
    data, h = fitsio.read(out)
    for key in ('CSUBSCAL', 'CSUBOFF', 'CSUBMETH', 'CSUBFILE', 'CSUBFWN', 'CSUBFWC', 'CSUBKSIG', 'CSUBNPIX', 'CSUBITER'):
        assert key in h, key
    assert h['FILTER'] == 'Ha' and h['CSUBMETH'] == 'PIXELS' and h['CSUBFILE'] == 'r.fits' and h['CSUBSCAL'] == rep['scale']
    assert h['CSUBNPIX'] == scene['fit']['n'] and h['CSUBITER'] == scene['fit']['iterations'] and h['CSUBFWN'] == 3.4
    assert any('ApContinuumSubtract' in line for line in h.history())
    _same_bits(np.asarray(data, F), cm.subtract(scene['nm'], scene['cm'], rep['scale'], rep['offset']), 'file image')
    # the script: files in, files out, status 0; without PSF matching and with a given scale and offset it is N - s C - b exactly
    out2 = str(tmp_path / 'line2.fits')
    assert script.main([nf, cf, out2, '--no_psf_match', '--scale', '0.083', '--offset', '0.4', '-l', 'ERROR']) == 0
    data2, h2 = fitsio.read(out2)
    want = (scene['n'] - F(0.083) * scene['c']) - F(0.4)
    _same_bits(np.asarray(data2, F), want.astype(F), 'script, given scale')
    assert h2['CSUBMETH'] == 'USER' and h2['CSUBSCAL'] == 0.083 and h2['CSUBKSIG'] == 0.0
    out3, pre = str(tmp_path / 'line3.fits'), str(tmp_path / 'matched')
    assert script.main([nf, cf, out3, '--fwhm', '3.4,2.6', '--matched_out', pre, '-l', 'ERROR']) == 0
    _same_bits(np.asarray(fitsio.read(out3)[0], F), np.asarray(data, F), 'script, fitted')
    _same_bits(np.asarray(fitsio.read(pre + '_continuum.fits')[0], F), scene['cm'], 'matched_out')
    with pytest.raises(RuntimeError, match='one pixel grid'):
        fitsio.write(cf, scene['c'][:-1])
        script.main([nf, cf, out3, '-l', 'ERROR'])
    assert os.path.exists(out3)
