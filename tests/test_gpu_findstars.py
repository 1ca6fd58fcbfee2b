"""F6 star finder on the GPU: every kernel of csrc/findstars.hip against the CPU model (tests/findstars_model.py), the annulus
clip against astropy's own numbers (G16), and ApFindStars / ap_find_stars end to end.

Fields are a flat sky plus Gaussian stars plus seeded noise, quantised to multiples of 1/8; shapes are no multiple of the
convolution's 16 x 64 tile."""
import json
import math

import numpy as np
import pytest

from tests import findstars_model as fm
from tests.util import assert_biteq, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
SKY = 200.0
EPS = 2.0 ** -52


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def add_star(img, cy, cx, amp, s):
    H, W = img.shape
    yy, xx = np.mgrid[0:H, 0:W]
    img += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))


def quant(img):
    return (np.rint(np.asarray(img, np.float64) * 8.0) / 8.0).astype(np.float32)


def field(H, W, seed, nstars=12, noise=4.0, stars=()):
    rng = np.random.default_rng(seed)
    img = rng.normal(SKY, noise, (H, W))
    for _ in range(nstars):
        add_star(img, rng.uniform(0, H), rng.uniform(0, W), rng.uniform(100, 5000), rng.uniform(1.0, 2.2))
    for s in stars:
        add_star(img, *s)
    return quant(img)


# ---- convolution ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fwhm', [3.0, 4.3, 7.9])
@pytest.mark.parametrize('shape', [(97, 131), (64, 200), (1, 40), (3, 4)])
def test_convolve_bit_equal(fwhm, shape):
    """Every pixel bit-equal to the model: the first and last R rows and columns (zero padding), the seams of the 16 x 64 tiles
    (rows 16, 32, ..; columns 64, 128), images narrower than a tile, a single row, an image smaller than the kernel."""
    from astrophotography_amd import ops
    img = field(*shape, seed=11, nstars=6)
    k = fm.daofind_kernel(fwhm)
    ref = fm.convolve(fm.subtract_bg(img, SKY), k['K'])
    got = ops.daofind_convolve(dev(img), fwhm, bg_median=SKY).cpu().numpy()
    assert_biteq(got, ref, 'convolve fwhm %g %s' % (fwhm, shape))
    assert np.isfinite(ref).all() and (np.abs(ref).max() > 1.0 or min(shape) < 5)


def test_convolve_nonfinite_pixels_spread_as_in_the_model():
    from astrophotography_amd import ops
    img = field(40, 70, seed=12, nstars=3)
    img[5, 5], img[20, 64], img[39, 0] = np.nan, np.inf, -np.inf
    k = fm.daofind_kernel(3.0)
    ref = fm.convolve(fm.subtract_bg(img, 0.0), k['K'])
    got = ops.daofind_convolve(dev(img), k, bg_median=0.0).cpu().numpy()
    assert np.isnan(ref).sum() >= 25 + 9 and np.isfinite(ref).sum() > 2000
    assert_biteq(got, ref, 'non-finite')


# ---- peaks ------------------------------------------------------------------------------------------------------------------
def test_peaks_exact_on_constructed_cases():
    """Stars on tile seams and corners, closer to the border than R (dropped) and exactly R from it (kept), a two-pixel plateau
    (both kept), a masked star, peaks just inside and just outside a saturation box, a value exactly equal to the threshold."""
    from astrophotography_amd import ops
    H, W, fwhm = 97, 131, 3.0
    k = fm.daofind_kernel(fwhm)
    R = k['R']
    assert R == 2
    stars = [(16.0, 64.0, 900.0, 1.3), (47.0, 63.0, 700.0, 1.3), (32.0, 128.0, 800.0, 1.3), (48.0, 30.0, 900.0, 1.3),
             (1.0, 20.0, 900.0, 1.3), (2.0, 40.0, 900.0, 1.3), (50.0, 1.0, 900.0, 1.3), (60.0, 2.0, 900.0, 1.3),
             (95.0, 100.0, 900.0, 1.3), (94.0, 80.0, 900.0, 1.3), (70.0, 129.0, 900.0, 1.3), (80.0, 128.0, 900.0, 1.3),
             (30.0, 90.0, 900.0, 1.3), (70.0, 40.0, 60000.0, 1.5), (70.0, 52.0, 900.0, 1.3),
             (81.0, 51.0, 900.0, 1.3), (70.0, 28.0, 900.0, 1.3)]
    img = field(H, W, seed=21, nstars=0, noise=1.0, stars=stars)
    d = fm.subtract_bg(img, SKY)
    plane = fm.convolve(d, k['K'])
    thr = float(np.float32(40.0))
    # a two-pixel plateau of equal maxima
    plane[40, 100] = plane[40, 101] = np.float32(500.0)
    # an isolated local maximum exactly equal to the threshold: rejected (strict), its twin one ulp above: kept
    plane[88, 20:25] = 0.0
    plane[86:91, 22] = 0.0
    plane[88, 22] = np.float32(thr)
    plane[88, 60:65] = 0.0
    plane[86:91, 62] = 0.0
    plane[88, 62] = np.nextafter(np.float32(thr), np.float32(np.inf))
    # the saturated star at (70, 40): box columns 40 - 11 .. 40 + 11, rows 70 - 11 .. 70 + 11 (half-open 29:52, 59:82)
    sat = fm.find_peaks(img, np.ones((12, 12), bool), 52428.0)
    assert sat.tolist() == [70 * W + 40]
    rects = fm.saturation_boxes(sat, W, H, fwhm)
    assert rects.tolist() == [[59, 82, 29, 52]]
    mask = np.zeros((H, W), np.uint8)
    mask[59:82, 29:52] = 1
    mask[28:33, 88:93] = 1                                   # the masked star at (30, 90)
    ref = fm.find_peaks(plane, k['fp'], thr, mask=mask, border=R)
    idx, n = ops.local_peaks(dev(plane), k['fp'], thr, mask=dev(mask), border=R)
    assert n == len(ref)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), ref)
    got = set(ref.tolist())

    def at(i, j):
        return i * W + j
    assert {at(16, 64), at(47, 63), at(32, 128)} <= got                                  # seams and corners of the tiles
    assert at(1, 20) not in got and at(2, 40) in got and at(50, 1) not in got and at(60, 2) in got
    assert at(95, 100) not in got and at(94, 80) in got and at(70, 129) not in got and at(80, 128) in got
    assert at(40, 100) in got and at(40, 101) in got                                       # the plateau
    assert at(30, 90) not in got and at(70, 40) not in got                                 # masked, saturated
    assert at(70, 52) in got and at(81, 51) not in got and at(70, 28) in got               # just outside / inside the box
    assert at(88, 22) not in got and at(88, 62) in got                                     # == threshold, threshold + 1 ulp
    # without the mask the masked ones come back
    ref2 = fm.find_peaks(plane, k['fp'], thr, border=R)
    idx2, n2 = ops.local_peaks(dev(plane), k['fp'], thr, border=R)
    assert np.array_equal(idx2.cpu().numpy().astype(np.int64), ref2) and at(30, 90) in set(ref2.tolist()) and n2 > n


@pytest.mark.parametrize('box', [12, 31, 5])
def test_square_footprint_is_scipys_maximum_filter(box):
    from scipy import ndimage
    from astrophotography_amd import ops
    img = field(64, 200, seed=3)
    thr = 400.0
    mx = ndimage.maximum_filter(img, size=box, mode='constant', cval=0.0)
    ref = np.flatnonzero((img == mx) & (img > thr))
    idx, n = ops.local_peaks(dev(img), box, thr)
    assert n == len(ref) > 3 and np.array_equal(idx.cpu().numpy().astype(np.int64), ref)
    assert np.array_equal(fm.find_peaks(img, np.ones((box, box)), thr), ref)


@pytest.mark.parametrize('shape', [(1, 40), (3, 4), (4, 131)])
def test_images_smaller_than_the_kernel_give_no_sources(shape):
    from astrophotography_amd import ops
    img = field(*shape, seed=5, nstars=0)
    img[shape[0] // 2, shape[1] // 2] += 5000.0
    r = ops.find_stars(dev(img), 3.0, 20.0, bg_median=SKY)
    assert r['n_candidates'] == 0 and r['xcentroid'].numel() == 0 and r['idx'].numel() == 0
    assert len(fm.find_stars(img, 3.0, 20.0, bg_median=SKY)['idx']) == 0


def spikes_image():
    img = np.full((64, 200), SKY, np.float32)
    pos = [(3 + 6 * a, 4 + 8 * b) for a in range(10) for b in range(24)][:200]
    assert len(set(pos)) == 200
    for t, (i, j) in enumerate(pos):
        img[i, j] += 1000.0 + 8.0 * t
        img[i, j - 1] += 400.0 + t                           # not a bare spike: some of them pass the sharpness limit
        img[i - 1, j] += 380.0
        img[i, j + 1] += 390.0
        img[i + 1, j] += 410.0
    return img, pos


def test_capacity_is_respected_and_the_true_count_returned():
    """200 isolated peaks, a list of 64: the count is 200, exactly 64 entries are written, the guard region behind the list is
    untouched; ops.find_stars then repeats the search with the right size and matches the model."""
    from astrophotography_amd import ops
    img, pos = spikes_image()
    W = img.shape[1]
    idx_all, n_all = ops.local_peaks(dev(img), 5, SKY + 500.0)
    assert n_all == 200 and set(idx_all.cpu().numpy().tolist()) == {i * W + j for i, j in pos}
    buf = torch.full((64 + 192,), -7, dtype=torch.int32, device='cuda')
    idx, n = ops.local_peaks(dev(img), 5, SKY + 500.0, capacity=64, list_out=buf)
    host = buf.cpu().numpy()
    assert n == 200
    assert np.all(host[64:] == -7), 'the list was written past its capacity'
    assert len(set(host[:64].tolist())) == 64 and set(host[:64].tolist()) <= {i * W + j for i, j in pos}
    assert idx.numel() == 64
    # capacity 0: nothing is written at all
    buf.fill_(-7)
    _, n0 = ops.local_peaks(dev(img), 5, SKY + 500.0, capacity=0, list_out=buf)
    assert n0 == 200 and np.all(buf.cpu().numpy() == -7)
    ref = fm.find_stars(img, 3.0, 50.0, bg_median=SKY)
    assert len(ref['peaks']) > 64
    r = ops.find_stars(dev(img), 3.0, 50.0, bg_median=SKY, capacity=64)
    assert r['n_candidates'] == len(ref['peaks'])
    assert np.array_equal(r['idx'].cpu().numpy().astype(np.int64), ref['idx'])


# ---- measurement ------------------------------------------------------------------------------------------------------------
def measure_bounds(m, k, thr):
    """Per candidate and record column, the bound on |kernel - model|.

    The kernel's only freedom is the order in which a wavefront adds the n_taps products of a sum, so a sum differs from the
    model's by at most e = n_taps * 2^-52 * S, S = the sum of the absolute values of its terms (both orders are within
    (n_taps - 1) * 2^-53 * S of the exact sum).  The scalar arithmetic after the sums is the same sequence of IEEE operations
    on both sides, so the bounds propagate to first order through the partial derivatives below; `slack` = 16 * 2^-52 * |value|
    covers the roundings of those operations (at most 8 per quantity, half an ulp each, on either side) and the second-order
    terms.  mag = -2.5 log10(flux) carries the device log10's 2 ulp instead (flux itself is exact: one IEEE division)."""
    n = (2 * k['R'] + 1) ** 2
    e = n * EPS * m['abs']                                   # [ncand, NQ + 2]
    s = m['sums']
    rec = m['rec']
    col = {nm: i for i, nm in enumerate(fm.REC)}
    p, sigsq = k['p'], k['sigma'] ** 2
    b = np.zeros_like(rec)
    with np.errstate(all='ignore'):
        b[:, col['sharpness']] = e[:, fm.Q_FP] / ((k['npixels'] - 1) * np.abs(rec[:, col['conv_peak']]))
        s2, s4 = s[:, fm.NQ], s[:, fm.NQ + 1]
        b[:, col['roundness1']] = 2.0 * (e[:, fm.NQ] / np.abs(s4) + np.abs(s2) * e[:, fm.NQ + 1] / (s4 * s4))
        eh = {}
        for tag, qg, qd in (('x', fm.Q_SUMGD_X, fm.Q_SDDGD_X), ('y', fm.Q_SUMGD_Y, fm.Q_SDDGD_Y)):
            c = k['consts'][tag]
            den = c['sumgsq'] - c['sumg'] ** 2 / p
            h = rec[:, col['h' + tag]]
            eh[tag] = (e[:, qg] + abs(c['sumg'] / p) * e[:, fm.Q_SUMD]) / abs(den)
            num = c['sgdgd'] - (s[:, qd] - c['sdgd'] * s[:, fm.Q_SUMD])
            enum = e[:, qd] + abs(c['sdgd']) * e[:, fm.Q_SUMD]
            D = h * c['sdgds'] / sigsq
            b[:, col['h' + tag]] = eh[tag]
            b[:, col['d' + tag]] = enum / np.abs(D) + np.abs(num) * eh[tag] * (c['sdgds'] / sigsq) / (D * D)
        b[:, col['xcentroid']] = b[:, col['dx']]
        b[:, col['ycentroid']] = b[:, col['dy']]
        hx, hy = rec[:, col['hx']], rec[:, col['hy']]
        b[:, col['roundness2']] = 2.0 * ((eh['x'] + eh['y']) / np.abs(hx + hy) + np.abs(hx - hy) * (eh['x'] + eh['y']) / (hx + hy) ** 2)
        slack = 16 * EPS * np.abs(rec)
        slack[:, col['xcentroid']] = 16 * EPS * (np.abs(rec[:, col['xcentroid']]) + np.abs(rec[:, col['dx']]))
        slack[:, col['ycentroid']] = 16 * EPS * (np.abs(rec[:, col['ycentroid']]) + np.abs(rec[:, col['dy']]))
        for exact in ('x_peak', 'y_peak', 'npix', 'peak', 'conv_peak', 'flux'):
            slack[:, col[exact]] = 0.0
        slack[:, col['mag']] = 4 * EPS * np.abs(rec[:, col['mag']])
    return b + slack


@pytest.mark.parametrize('fwhm,shape', [(3.0, (97, 131)), (4.3, (64, 200)), (7.9, (97, 131))])
def test_measure_matches_the_model(fwhm, shape):
    from astrophotography_amd import ops
    H, W = shape
    rng = np.random.default_rng(31)
    stars = [(rng.uniform(8, H - 8), rng.uniform(8, W - 8), rng.uniform(300, 6000), fwhm / 2.3548 * rng.uniform(0.8, 1.3)) for _ in range(22)]
    img = field(H, W, seed=32, nstars=0, noise=3.0, stars=stars).astype(np.float64)
    for t in range(10):                                      # cosmic-ray-like spikes (too sharp) and elongated trails (not round)
        i, j = int(rng.integers(14, H - 14)), int(rng.integers(14, W - 14))
        if t % 2:
            img[i, j] += 3000.0
        else:
            add_star(img, i, j, 900.0, 0.9)
            add_star(img, i, j + 2.0 * fwhm / 3.0, 850.0, 0.9)
    img = quant(img)
    img[50, 60] = np.nan                                     # a NaN poisons the candidates round it: rejected, not crashed
    k = fm.daofind_kernel(fwhm)
    threshold = 6.0 * 3.0
    thr_eff = threshold * k['relerr']
    d = fm.subtract_bg(img, SKY)
    conv = fm.convolve(d, k['K'])
    peaks = fm.find_peaks(conv, k['fp'], thr_eff, border=k['R'])
    m = fm.daofind_measure(d, conv, peaks, k, thr_eff)
    assert len(peaks) >= 25 and 10 <= m['keep'].sum() < len(peaks)
    bound = measure_bounds(m, k, thr_eff)
    col = {nm: i for i, nm in enumerate(fm.REC)}
    # no candidate of the model lies within its bound of a limit: the keep flags are then decided
    fin = np.isfinite(m['rec']).all(axis=1)
    for nm, limits in (('sharpness', (fm.SHARPLO, fm.SHARPHI)), ('roundness1', (fm.ROUNDLO, fm.ROUNDHI)),
                       ('roundness2', (fm.ROUNDLO, fm.ROUNDHI)), ('hx', (0.0,)), ('hy', (0.0,)), ('dx', (-k['R'], k['R'])),
                       ('dy', (-k['R'], k['R']))):
        for lim in limits:
            v, bd = m['rec'][fin, col[nm]], bound[fin, col[nm]]
            assert np.all(np.abs(v - lim) > bd), (nm, lim)
    rec, keep = ops.daofind_measure(dev(img), dev(conv), dev(peaks.astype(np.int32)), k, thr_eff, bg_median=SKY)
    rec, keep = rec.cpu().numpy(), keep.cpu().numpy().astype(bool)
    assert np.array_equal(keep, m['keep'])
    assert np.array_equal(rec[:, col['npix']], m['rec'][:, col['npix']]) and rec[0, col['npix']] == (2 * k['R'] + 1) ** 2
    assert np.array_equal(np.isnan(rec), np.isnan(m['rec']))
    worst = {}
    for nm, c in col.items():
        a, b_, bd = rec[fin, c], m['rec'][fin, c], bound[fin, c]
        diff = np.abs(a - b_)
        worst[nm] = float((diff / np.maximum(bd, 1e-300)).max()) if diff.max() > 0 else 0.0
        assert np.all(diff <= bd), (nm, diff.max(), bd[diff.argmax()])
    print('fwhm %g: %d candidates, %d kept; largest |diff| / bound per column: %s' % (fwhm, len(peaks), keep.sum(), worst))
    # and the composite gives the kept rows, in flat-index order
    r = ops.find_stars(dev(img), fwhm, threshold, bg_median=SKY)
    assert np.array_equal(r['idx'].cpu().numpy().astype(np.int64), peaks[m['keep']]) and r['n_candidates'] == len(peaks)
    assert_biteq(r['conv'].cpu().numpy(), conv, 'conv')


# ---- photometry -------------------------------------------------------------------------------------------------------------
def phot_bound(img, xc, yc, r, ref):
    """|kernel - model| bound of aperture_sum_raw: the order of the npix products (npix * 2^-52 * S, S = sum |overlap * data|)
    plus the overlap areas themselves - they go through sqrt, asin and sin, and the device's asin / sin may differ from libm's by
    2 ulp each: the arc term r^2 / 2 * (t - sin t), t <= pi, moves by at most 16 * 2^-52 * r^2 per edge pixel (two arc integrals of
    two arcs at most, 4 ulp of pi each), weighted with that pixel's |data|."""
    H, W = img.shape
    out = np.zeros(len(xc))
    for k in range(len(xc)):
        ov = fm.circle_overlap(float(xc[k]), float(yc[k]), r, H, W)
        edge = (ov > 0) & (ov < 1)
        out[k] = ref['npix'][k] * EPS * ref['abs'][k] + 16 * EPS * r * r * np.abs(img[edge].astype(np.float64)).sum()
    return out


@pytest.mark.parametrize('fwhm', [3.0, 7.9])
def test_aperture_photometry_matches_the_model(fwhm):
    """Centres at integer, half-integer and arbitrary fractions; apertures and annuli hanging over every edge and corner; an
    annulus holding NaN; an annulus with a neighbouring star in it (the clip removes it: the median stays at the sky)."""
    from astrophotography_amd import ops
    H, W = 97, 131
    r, r_in, r_out = fm.aperture_radii(fwhm)
    img = field(H, W, seed=41, nstars=0, noise=3.0,
                stars=[(48.0, 60.0, 4000.0, 1.4), (48.0 + 1.2 * r, 60.0 + 0.3 * r, 9000.0, 1.4), (20.0, 100.0, 2500.0, 1.4)])
    img[48, 60 - int(r) - 2] = np.nan
    img[47, 60 - int(r) - 2] = np.inf
    xc = [60.0, 100.0, 30.5, 30.0, 77.5, 41.37, 88.113, 0.0, 3.3, 130.0, 128.6, 65.2, 64.0, 0.4, 129.9, 1.7, 129.2, -3.0, 135.0, 64.25]
    yc = [48.0, 20.0, 70.0, 70.5, 30.5, 66.81, 71.004, 50.0, 44.4, 52.0, 60.1, 0.0, 96.0, 0.3, 0.2, 95.8, 96.0, 40.0, 99.5, 2.5]
    ref = fm.aperture_photometry(img, xc, yc, fwhm)
    got = {k_: v.cpu().numpy() for k_, v in ops.aperture_photometry(dev(img), xc, yc, fwhm).items()}
    assert np.array_equal(got['n_annulus'], ref['n_annulus']) and ref['n_annulus'].min() > 0
    assert_biteq(got['bkg_median'], ref['bkg_median'], 'bkg_median')
    # source 0 sits in the middle: its annulus holds the NaN, the inf and the neighbour's core, and its median is the sky
    vals = fm.annulus_values(img, xc[0], yc[0], r_in, r_out)
    assert np.isnan(vals).any() and np.isinf(vals).any() and np.nanmax(np.where(np.isfinite(vals), vals, 0)) > SKY + 1000
    assert abs(float(ref['bkg_median'][0]) - SKY) < 2.0
    bound = phot_bound(img, xc, yc, r, ref)
    diff = np.abs(got['aperture_sum_raw'] - ref['aperture_sum_raw'])
    fin = np.isfinite(ref['aperture_sum_raw'])
    assert np.array_equal(np.isfinite(got['aperture_sum_raw']), fin) and fin.sum() >= len(xc) - 2
    print('fwhm %g: aperture sums, largest |diff| / bound %.3f; areas: largest |diff| %.2e' % (
        fwhm, (diff[fin] / bound[fin]).max(), np.abs(got['area'] - ref['area']).max()))
    assert np.all(diff[fin] <= bound[fin])
    nedge = 8 * (r + 1)
    assert np.all(np.abs(got['area'] - ref['area']) <= ref['npix'] * EPS * ref['area'] + 16 * EPS * r * r * nedge)
    inside = [k_ for k_ in range(len(xc)) if r <= min(xc[k_], yc[k_], W - 1 - xc[k_], H - 1 - yc[k_])]
    assert len(inside) >= 6 and np.all(np.abs(got['area'][inside] - math.pi * r * r) < 1e-10)
    assert np.all(got['area'][[7, 9, 13, 17]] < math.pi * r * r - 1.0)                 # hanging over an edge / a corner
    exp = got['aperture_sum_raw'] - got['bkg_median'].astype(np.float64) * (math.pi * r * r)
    assert np.array_equal(got['aperture_sum'][fin], exp[fin])


@pytest.mark.parametrize('radii,lo,hi', [((2.0, 1.0, 1.7), 3, 8), ((2.0, 5.0, 8.1), 120, 129), ((2.0, 5.0, 8.3), 129, 138),
                                         ((2.0, 5.0, 10.3), 250, 258)])
def test_annulus_counts_on_both_sides_of_numpys_boundaries(radii, lo, hi):
    """Thin annuli on a 64 x 64 field with stars in it (the clip removes them): the clip's float32 sums run over a handful of
    values (numpy's short form below 8), over counts on both sides of 128 (one leaf against the split tree) and over about
    250; the annuli of the sources at the edges are cut off by the image.  bkg_median depends on the sums only through the
    clip's bounds, so a last-bit error would seldom show here: the exact check of the sum is the host test of np_exact.h."""
    from astrophotography_amd import ops
    img = field(64, 64, seed=64, nstars=6, noise=3.0)
    xc = [32.0, 31.5, 30.25, 20.7, 40.37, 33.113, 0.0, 63.0, 2.3, 25.5]
    yc = [32.0, 30.5, 33.4, 41.1, 22.81, 28.004, 30.0, 63.0, 60.1, 36.0]
    vals = [fm.annulus_values(img, x, y, radii[1], radii[2]) for x, y in zip(xc, yc)]
    got = ops.aperture_photometry(dev(img), xc, yc, radii=radii)
    counts = got['n_annulus'].cpu().numpy()
    assert np.array_equal(counts, [v.size for v in vals]) and counts.min() > 0
    assert counts.min() <= lo and counts.max() >= hi and np.any((counts > lo) & (counts < hi)), counts
    if lo < 128 <= hi:
        assert np.any(counts == 128) and np.any(counts < 128) and np.any(counts > 128), counts
    assert_biteq(got['bkg_median'].cpu().numpy(), np.array([fm.annulus_clip(v)[1] for v in vals], np.float32), 'bkg_median')


def test_annulus_clip_equals_astropy_g16():
    """Every G16 vector laid, in row-major order, into the annulus of one source (radii 17 .. 26, 1252 pixels), the rest of the
    annulus NaN (dropped before the clip): the kernel's bkg_median equals astropy's median, compared as float32, exactly."""
    from astrophotography_amd import ops
    g = load_golden('g16_annulus.npz')
    meta = json.loads(str(g['_meta']))
    H = W = 61
    cx = cy = 30.0
    radii = (17.0, 17.0, 26.0)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = (xx - cx) ** 2 + (yy - cy) ** 2
    member = np.flatnonzero((d2 >= radii[1] ** 2) & (d2 <= radii[2] ** 2))
    assert len(member) >= 1100
    imgs = np.full((len(meta), H * W), SKY, np.float32)
    for t, m in enumerate(meta):
        v = g['c%d_values' % m['case']]
        imgs[t, member] = np.nan
        imgs[t, member[:len(v)]] = v
    # one tall image, one source per vector: the sources are 61 rows apart, so no annulus reaches a neighbour's rows
    tall = imgs.reshape(len(meta) * H, W)
    r = ops.aperture_photometry(dev(tall), [cx] * len(meta), [cy + H * t for t in range(len(meta))], radii=radii)
    got = r['bkg_median'].cpu().numpy()
    assert np.all(r['n_annulus'].cpu().numpy() == len(member))
    for t, m in enumerate(meta):
        ref = np.float32(g['c%d_stats' % m['case']][1])
        assert_biteq(got[t:t + 1], np.array([ref], np.float32), m['name'])


def test_unsupported_fwhm_is_an_error_not_a_fallback():
    from astrophotography_amd import ops
    from astrophotography_amd._lib import ApGpuError, E_UNSUPPORTED
    img = dev(field(40, 70, seed=1, nstars=1))
    with pytest.raises(ValueError):
        ops.find_stars(img, 22.0, 10.0)
    with pytest.raises(ApGpuError) as e:
        ops.aperture_photometry(img, [20.0], [20.0], fwhm=16.0)
    assert e.value.code == E_UNSUPPORTED


# ---- class and script -------------------------------------------------------------------------------------------------------
def frame_256(dtype):
    H = W = 256
    rng = np.random.default_rng(51)
    img = rng.normal(300.0, 5.0, (H, W))
    img[100:140, 20:60] = 300.0                              # two noise-free patches holding the same star: a tie of the sort key
    img[100:140, 180:220] = 300.0
    for _ in range(36):
        add_star(img, rng.uniform(10, H - 10), rng.uniform(62, 178), rng.uniform(200, 20000), rng.uniform(1.1, 1.6))
    add_star(img, 200.3, 30.6, 64000.0, 1.6)                 # two stars above sat_frac * 65535
    add_star(img, 30.2, 215.1, 58000.0, 1.5)
    stamp = np.zeros((H, W))
    add_star(stamp, 120.0, 40.0, 5000.0, 1.3)
    stamp = np.rint(stamp[100:140, 20:60])
    img[100:140, 20:60] += stamp
    img[100:140, 180:220] += stamp
    img = np.clip(np.rint(img), 0, 65535)
    return img.astype(dtype)


def model_flow(img, fwhm, nsigma, bitdepth, sat_frac, nosatmask, max_sources, exposure):
    """The reference's constructor on the model, with the background statistics from ops.sigclip_global used as it prescribes."""
    from astrophotography_amd import ops
    H, W = img.shape
    t = ops.to_device_u16(img) if img.dtype == np.uint16 else dev(img)
    d32 = img.astype(np.float32)
    d32_t = dev(d32)
    s10 = ops.sigclip_global(d32_t, sigma=3.0, maxiters=10)
    thr = (s10[0].float() + s10[2].float() * 2.0).double()
    above, _ = ops.threshold_mask(d32_t, thresholds=torch.stack([torch.full_like(thr, -float('inf')), thr]).contiguous())
    smask, _ = ops.source_mask(above, min_pixels=5, dilate_size=11)
    x = d32_t.clone() if img.dtype == np.float32 else dev(img.astype(np.float64))
    x[smask != 0] = float('nan')
    st = ops.sigclip_global(x, sigma=3.0).cpu().numpy()
    bg_mean, bg_median, bg_std = float(st[0]), float(st[1]), float(st[2])
    sat_thresh = math.floor(sat_frac * (2 ** bitdepth - 1))
    box = int(4 * fwhm)
    sat = fm.find_peaks(d32, np.ones((box, box), bool), float(sat_thresh))
    rects = fm.saturation_boxes(sat, W, H, fwhm)
    mask = np.zeros((H, W), np.uint8)
    if not nosatmask:
        for r0, r1, c0, c1 in rects:
            mask[r0:r1, c0:c1] = 1
    fs = fm.find_stars(d32, fwhm, nsigma * bg_std, bg_median=bg_median, mask=mask)
    col = {nm: i for i, nm in enumerate(fm.REC)}
    xcen, ycen, peak = fs['rec'][:, col['xcentroid']], fs['rec'][:, col['ycentroid']], fs['rec'][:, col['peak']]
    ph = fm.aperture_photometry(d32, xcen, ycen, fwhm)
    adu = ph['aperture_sum'] / exposure
    order = np.lexsort((ycen, xcen, adu))[::-1]
    if max_sources is not None:
        order = order[:max_sources]
    table = dict(id=np.arange(1, len(xcen) + 1)[order], xcenter=xcen[order], ycenter=ycen[order], aperture_sum=ph['aperture_sum'][order],
                 peak_adu=peak[order], psbl_sat=(peak > sat_thresh)[order], bgmed_per_pix=ph['bkg_median'].astype(np.float64)[order],
                 adu_per_sec=adu[order])
    return dict(bg=(bg_mean, bg_median, bg_std), sat=sat, rects=rects, mask=mask, table=table, ndet=len(xcen))


def check_table(t, ref, fwhm):
    """ids, flags, peaks and annulus medians are exact.  The centroids carry the measurement bound (below 1e-12 here: sums of
    |terms| < 1e7 over 25 taps, divided by amplitudes > 10); an aperture sum moves with its centre by at most (perimeter 2 pi r) *
    (peak < 65535) per pixel of shift, i.e. by < 1e-5 for a shift of 1e-12, plus its own summation bound (< 1e-8)."""
    assert np.array_equal(t['id'], ref['id'])
    assert np.array_equal(t['psbl_sat'], ref['psbl_sat'])
    assert np.array_equal(t['peak_adu'], ref['peak_adu'])
    assert np.array_equal(t['bgmed_per_pix'], ref['bgmed_per_pix'])
    assert np.all(np.abs(t['xcenter'] - ref['xcenter']) < 1e-12) and np.all(np.abs(t['ycenter'] - ref['ycenter']) < 1e-12)
    assert np.all(np.abs(t['aperture_sum'] - ref['aperture_sum']) < 1e-5)
    assert np.all(np.abs(t['adu_per_sec'] - ref['adu_per_sec']) < 1e-5)
    with np.errstate(all='ignore'):
        assert np.allclose(t['magnitude'], -2.5 * np.log10(t['adu_per_sec']), rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize('dtype', [np.uint16, np.float32])
def test_class_and_script(tmp_path, dtype):
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio, ops
    from astrophotography_amd.scripts import ap_find_stars as script
    img = frame_256(dtype)
    hdr = fitsio.Header()
    hdr['EXPTIME'] = 4.0
    hdr['FILTER'] = 'L'
    path = tmp_path / 'frame.fits'
    fitsio.write(str(path), img, hdr)
    fwhm, nsigma = 3.0, 7.0
    ref = model_flow(img, fwhm, nsigma, 16, 0.80, False, 25, 4.0)
    assert len(ref['sat']) == 2 and ref['ndet'] >= 30

    fs = ap.ApFindStars(str(path), 0, fwhm, nsigma, 16, 25, False, 0.80, 'WARNING', None, True)
    # background statistics: ops.sigclip_global as the reference prescribes (model_flow made the same calls)
    assert (fs._bg_mean, fs._bg_median, fs._bg_stddev) == ref['bg']
    assert fs._nsrcs_saturated == 2 and np.array_equal(fs._saturated_idx, ref['sat'])
    assert np.array_equal(fs._sat_rects, ref['rects']) and np.array_equal(fs._mask.cpu().numpy(), ref['mask'])
    assert fs._nsrcs_detected == ref['ndet'] and fs._nsrcs_photom == 25 and len(fs._sources['id']) == ref['ndet']
    assert list(fs._phot_table) == ['id', 'xcenter', 'ycenter', 'aperture_sum', 'peak_adu', 'psbl_sat', 'bgmed_per_pix', 'adu_per_sec',
                                    'magnitude']
    assert list(fs._sources) == ['id', 'xcentroid', 'ycentroid', 'sharpness', 'roundness1', 'roundness2', 'npix', 'sky', 'peak', 'flux',
                                 'mag', 'psbl_sat']
    check_table(fs._phot_table, ref['table'], fwhm)
    assert not fs._phot_table['psbl_sat'].any()              # the saturated stars were masked out
    t = fs._phot_table
    # notrim keeps all; trim cuts
    full = fs.aperture_photometry(notrim=True)
    assert len(full['id']) == ref['ndet'] == fs._nsrcs_photom
    # the tie: the two identical stars have equal adu_per_sec and follow each other, larger xcenter first (:428, reverse=True)
    tie = [i for i in range(len(full['id']) - 1) if full['adu_per_sec'][i] == full['adu_per_sec'][i + 1]]
    assert len(tie) == 1 and full['xcenter'][tie[0]] > full['xcenter'][tie[0] + 1] and abs(full['xcenter'][tie[0]] - 200.0) < 0.5
    assert abs(full['xcenter'][tie[0] + 1] - 40.0) < 0.5 and abs(full['ycenter'][tie[0]] - 120.0) < 0.5
    fs.trim(5)
    assert len(fs._phot_table['id']) == 5 and np.array_equal(fs._phot_table['id'], ref['table']['id'][:5])
    fs.aperture_photometry()

    # --retain_saturated: the saturated stars stay in the list, flagged
    ref_keep = model_flow(img, fwhm, nsigma, 16, 0.80, True, None, 4.0)
    keep = ap.ApFindStars(str(path), 0, fwhm, nsigma, 16, None, True, 0.80, 'WARNING', None, True)
    assert keep._nsrcs_saturated == 2 and int(keep._mask.sum()) == 0
    check_table(keep._phot_table, ref_keep['table'], fwhm)
    assert keep._phot_table['psbl_sat'].sum() == 2 and keep._sources['psbl_sat'].sum() == 2

    # from_device gives the file path's table
    t_dev = ops.to_device_u16(img) if dtype == np.uint16 else dev(img)
    fd = ap.ApFindStars.from_device(t_dev, hdr, search_fwhm=fwhm, search_nsigma=nsigma, max_sources=25, loglevel='WARNING')
    for key, v in fs._phot_table.items():
        assert np.array_equal(fd._phot_table[key], v, equal_nan=v.dtype.kind == 'f'), key
    assert (fd._bg_mean, fd._bg_median, fd._bg_stddev) == ref['bg']

    # files
    reg, out = tmp_path / 'stars.reg', tmp_path / 'stars.fits'
    fs.write_ds9_region_file(str(reg))
    circles = [ln for ln in reg.read_text().splitlines() if ln.startswith('circle(')]
    assert len(circles) == 25 and all(ln.split(')')[0].endswith(',%.4f' % math.ceil(2 * fwhm)) for ln in circles)
    assert circles[0].startswith('circle(%.4f,%.4f,' % (t['xcenter'][0] + 1, t['ycenter'][0] + 1))
    assert script.main([str(path), str(out), '-m', '25', '-q', '-l', 'WARNING', '-d', str(tmp_path / 's2.reg'), '--plotfile', 'x.png']) == 0
    cols, eh, prim = fitsio.read_table(str(out), 'AP_L1MAG')
    for key, v in fs._phot_table.items():
        assert np.array_equal(cols[key], v, equal_nan=v.dtype.kind == 'f'), key
    xy, _, _ = fitsio.read_table(str(out), 'AP_XYPOS')
    assert np.array_equal(xy['X'], t['xcenter'] + 1.0) and np.array_equal(xy['Y'], t['ycenter'] + 1.0)
    assert prim['AP_NDET'] == ref['ndet'] and prim['AP_NPHOT'] == 25 and prim['AP_NFIT'] == 0 and prim['AP_NSIGM'] == nsigma
    assert prim['AP_BGMED'] == ref['bg'][1] and prim['AP_BGSTD'] == ref['bg'][2] and prim['IMG_COLS'] == 256 and prim['FILTER'] == 'L'
    assert 'AP_FWHM' not in prim and len((tmp_path / 's2.reg').read_text().splitlines()) == 27
