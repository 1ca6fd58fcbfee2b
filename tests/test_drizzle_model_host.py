"""F14 on the host: the NumPy model tests/drizzle_model.py against what it must do - identity, constants, flux and
coverage, the resolution a dithered set buys, CFA planes, outlier rejection, argument errors.  No GPU, no torch: the kernels are
held to this model bit for bit in tests/test_gpu_drizzle.py."""
import numpy as np
import pytest

from tests import drizzle_model as dm

F = np.float32
EPS = 2.0 ** -24                                                      # half a float32 ulp, relative


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_identity():
    rng = np.random.default_rng(1)
    img = rng.normal(300.0, 40.0, (23, 31)).astype(F)
    r = dm.drizzle(img[None], [dm.shift_affine(0, 0)], scale=1, pixfrac=1)
    assert r['image'].shape == img.shape and np.array_equal(r['image'].view(np.uint32), img.view(np.uint32))
    assert np.all(r['weight'] == 1)
    img[4, 5] = np.nan                                                # a hole stays a hole and takes nothing else with it
    r = dm.drizzle(img[None], [dm.shift_affine(0, 0)], scale=1, pixfrac=1)
    assert np.isnan(r['image'][4, 5]) and r['weight'][4, 5] == 0 and np.isnan(r['image']).sum() == 1


@pytest.mark.parametrize('s', [1, 1.5, 2, 3])
@pytest.mark.parametrize('p', [0.3, 0.5, 1])
def test_constant(s, p):
    """A constant stays that constant, to 1 float32 ulp, wherever anything lands (the sums are float64: the quotient of the two sums
    is the constant to ~1e-15 and rounds to it or its neighbour)."""
    rng = np.random.default_rng(int(10 * s + 100 * p))
    N, H, W = 5, 21, 26
    c = F(1234.567)
    frames = np.full((N, H, W), c, F)
    aff = [dm.shift_affine(rng.uniform(-3, 3), rng.uniform(-3, 3), 3.0 if i % 2 else 0.0) for i in range(N)]
    aff[1] = dm.shift_affine(0.5, -1.5)
    mask = rng.random((H, W)) < 0.1
    fmask = rng.random((N, H, W)) < 0.2
    frames[rng.random(frames.shape) < 0.05] = np.nan
    r = dm.drizzle(frames, aff, s, p, weights=rng.uniform(0.2, 5.0, N), mask=mask, frame_masks=fmask)
    got = r['weight'] > 0
    assert got.any() and np.array_equal(np.isnan(r['image']), ~got)
    assert _ulps(r['image'][got], np.full(int(got.sum()), c, F)).max() <= 1


def _wholly_inside(shape, A, p, out_shape):
    """bool [H, W]: the drop of input pixel (i, j) lies inside the area the output grid covers (A: the composed transform, no
    rotation)."""
    H, W = shape
    h, w = out_shape
    xa, xb = sorted((A[0] * -0.5 + A[2], A[0] * (w - 0.5) + A[2]))
    ya, yb = sorted((A[4] * -0.5 + A[5], A[4] * (h - 0.5) + A[5]))
    i, j = np.arange(W), np.arange(H)
    okx = (i - p / 2 >= xa) & (i + p / 2 <= xb)
    oky = (j - p / 2 >= ya) & (j + p / 2 <= yb)
    return oky[:, None] & okx[None, :]


@pytest.mark.parametrize('s,p', [(1, 1), (1.5, 0.5), (2, 0.5), (2, 0.3), (3, 1), (3, 0.3)])
def test_flux_and_coverage(s, p):
    """Without rotation the footprints of the output pixels tile the plane, so the covers of a drop that lies wholly inside the grid
    add up to 1: sum(weight) = sum_i w_i n_i and, flux conserved, sum(image weight) = sum_i w_i g_i sum(v) over those pixels (the
    others are masked here).
    Bound: window coordinates are below 4, so a float32 edge is off by at most 2^-23 and an overlap by 2^-22; at most 4 output pixels
    per axis share a drop, so its covers add up to 1 within 2 x 4 x 2^-22 / p, plus 16 roundings of 2^-24 in the products, the
    quotient and the float32 planes.  The sums of the planes themselves are taken in float64 here."""
    rng = np.random.default_rng(int(7 * s + 13 * p))
    N, H, W = 4, 19, 23
    frames = rng.uniform(50.0, 150.0, (N, H, W)).astype(F)
    shifts = [(0.0, 0.0), (0.25, -0.5), (-1.37, 2.21), (3.5, 0.125)]
    aff = [dm.shift_affine(dx, dy, 0.0, 1.0 if k else 1.03) for k, (dx, dy) in enumerate(shifts)]
    w = np.array([1.0, 2.5, 0.4, 1.7], F)
    fs = np.array([1.0, 0.5, 0.25, 2.0], F)
    out_shape = dm.default_out_shape((H, W), s)
    prm = dm.frame_params(aff, s, N, fs, w, conserve_flux=True)
    inside = np.stack([_wholly_inside((H, W), prm[k], float(F(p)), out_shape) for k in range(N)])
    assert inside.any() and not inside.all()                           # some drops are cut by the grid's edge: they are left out
    r = dm.drizzle(frames, aff, s, p, fscale=fs, weights=w, frame_masks=~inside, conserve_flux=True)
    tol = 2 * 4 * 2.0 ** -22 / float(p) + 16 * EPS
    want_w = float((w.astype(np.float64) * inside.sum((1, 2))).sum())
    got_w = float(r['weight'].astype(np.float64).sum())
    g = prm[:, 9]
    want_f = float((w.astype(np.float64) * g * (frames.astype(np.float64) * inside).sum((1, 2))).sum())
    ok = r['weight'] > 0
    got_f = float((r['image'][ok].astype(np.float64) * r['weight'][ok].astype(np.float64)).sum())
    print('s %g p %g: coverage %.9g / %.9g (rel %.2e), flux %.9g / %.9g (rel %.2e), bound %.2e'
          % (s, p, got_w, want_w, got_w / want_w - 1, got_f, want_f, got_f / want_f - 1, tol))
    assert abs(got_w / want_w - 1) <= tol and abs(got_f / want_f - 1) <= tol


RESOLUTION_TOL = 0.012
LATTICE_TOL = 1e-5


def test_resolution():
    """The point of the feature: 16 noise-free frames of Gaussian stars (sigma_0 = 0.5 input pixels, integrated over the pixels with
    erf) on the exact 4 x 4 lattice of quarter-pixel dithers.  At s = 2, p = 0.5 the star's second-moment variance per axis
    approaches the true PSF's plus those of the input pixel, the drop and the output pixel: 0.25 + (1 + 0.25 + 0.25) / 12 = 0.375
    pixels^2.  Measured with the model on the CPU over a +-4 pixel stamp, the four stars, both axes: 0.3645833 (all eight within
    4e-9 of each other); the same stars at s = 1, p = 1 measure 0.4895833 against 0.25 + 3 / 12 = 0.5.  Both fall short by 1 / 96 =
    0.0104167, and for a known reason: on a lattice of spacing d = 1/4 the drop and the output pixel act as sums over points d
    apart, not as integrals, and n points d apart have the variance (L^2 - d^2) / 12 of a box of L = n d less d^2 / 12 = 1 / 192
    each.  So the value for this lattice is 0.375 - 2 / 192, which the model meets to 4e-9 (the stamp's truncation and float32;
    asserted to 1e-5), and the tolerance against the continuous value is that shortfall plus 0.0016: 0.012 pixels^2, a fifth of the
    0.0625 by which a drop or an output pixel of twice the size would raise the variance."""
    sc = dm.scene()
    fine = dm.drizzle(sc['frames'], sc['affines'], 2, 0.5)
    coarse = dm.drizzle(sc['frames'], sc['affines'], 1, 1)
    want = sc['sigma0'] ** 2 + (1 + 0.5 ** 2 + 1 / 2 ** 2) / 12
    want_coarse = sc['sigma0'] ** 2 + 3 / 12
    short = 2 * 0.25 ** 2 / 12
    for x, y, _ in sc['stars']:
        vf = dm.star_variance(fine['image'], 2, x, y)
        vc = dm.star_variance(coarse['image'], 1, x, y)
        print('star (%.2f, %.2f): variance %.9f %.9f at s 2 p 0.5 (analytic %.6f, on the lattice %.9f), %.9f %.9f at s 1 p 1'
              % (x, y, vf[0], vf[1], want, want - short, vc[0], vc[1]))
        for a, b in zip(vf, vc):
            assert abs(a - want) <= RESOLUTION_TOL and a < b
            assert abs(a - (want - short)) <= LATTICE_TOL and abs(b - (want_coarse - short)) <= LATTICE_TOL


def _colour_planes(shape):
    """Three smooth planes over reference coordinates (x, y): callables, and the largest gradient per axis among them."""
    planes = [lambda x, y: 1000.0 + 2.0 * x + 1.0 * y + 0.01 * x * y,
              lambda x, y: 1500.0 - 1.5 * x + 2.0 * y + 0.02 * x * x,
              lambda x, y: 800.0 + 1.0 * x - 2.0 * y - 0.02 * y * y]
    n = max(shape) + 8
    gx = max(2.0 + 0.01 * n, 1.5 + 0.04 * n, 1.0)
    gy = max(1.0 + 0.01 * n, 2.0, 2.0 + 0.04 * n)
    return planes, gx, gy


def cfa_scene(shape=(24, 28), pattern='RGGB'):
    """16 quarter-pixel dithers whose whole-pixel parts run through the four CFA phases; the three planes as every frame sees them
    ([3, N, H, W]) and the mosaics ([N, H, W])."""
    H, W = shape
    pat = dm.COLOURS[pattern]
    planes, gx, gy = _colour_planes(shape)
    shifts = [(dx + (k & 1), dy + ((k >> 1) & 1)) for k, (dx, dy) in enumerate(dm.lattice(4))]
    assert {(int(sx) & 1, int(sy) & 1) for sx, sy in shifts} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    jj, ii = np.mgrid[0:H, 0:W].astype(np.float64)
    full = np.stack([np.stack([pl(ii - sx, jj - sy) for sx, sy in shifts]) for pl in planes]).astype(F)
    colour = np.array(pat)[((np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1))]
    chan = np.where(colour == 3, 1, colour)
    mosaic = np.take_along_axis(full, np.broadcast_to(chan[None, None], (1,) + full.shape[1:]), 0)[0]
    return dict(full=full, mosaic=mosaic, affines=[dm.shift_affine(sx, sy) for sx, sy in shifts], pattern=pat, gx=gx, gy=gy, chan=chan)


@pytest.mark.parametrize('pattern', ['RGGB', 'GBRG'])
def test_cfa_planes(pattern):
    """Each plane drizzled from the mosaic against the same model run on the whole (un-mosaicked) plane.  Both are weighted means of
    samples of a smooth plane P taken within hx + p/2 = 0.5 pixels per axis of the output pixel's centre, so each lies within
    0.5 (Gx + Gy) of P there and they differ by at most Gx + Gy (the planes' largest gradients per axis), plus float32 rounding of
    values near 2000 (4 x 2^-24 x 2000)."""
    sc = cfa_scene(pattern=pattern)
    tol = (sc['gx'] + sc['gy']) * 2 * (0.25 + 0.25) + 4 * EPS * 2000
    for c in range(3):
        got = dm.drizzle(sc['mosaic'], sc['affines'], 2, 0.5, cfa=(sc['pattern'], c))
        want = dm.drizzle(sc['full'][c], sc['affines'], 2, 0.5)
        both = (got['weight'] > 0) & (want['weight'] > 0)
        inner = np.zeros_like(both)
        inner[8:-8, 8:-8] = True
        assert both[inner].mean() > 0.5                               # (16 dithers do not bring every colour to every output pixel)
        d = np.abs(got['image'][both].astype(np.float64) - want['image'][both])
        print('%s channel %d: max |difference| %.4f (bound %.4f), %d pixels' % (pattern, c, d.max(), tol, both.sum()))
        assert d.max() <= tol
        # the weight of a plane is the share of its colour: a quarter (a half for green) of the whole plane's
        share = got['weight'][inner].astype(np.float64).sum() / want['weight'][inner].astype(np.float64).sum()
        print('weight share %.4f' % share)
        assert abs(share - (0.5 if c == 1 else 0.25)) < 0.02


@pytest.mark.parametrize('pattern', ['RGGB', 'BGGR', 'GRBG', 'GBRG'])
def test_cfa_single_frame_reach(pattern):
    """One frame, identity, s = 2, p = 0.5: output pixel u sits at u / 2 - 0.25, its footprint and the drops are a quarter pixel
    either way, so it overlaps input pixel floor(u / 2) alone (all of it exact in binary): the weight is zero exactly where
    that pixel has another colour."""
    sc = cfa_scene(pattern=pattern)
    H, W = sc['mosaic'].shape[1:]
    src_j, src_i = np.arange(2 * H) // 2, np.arange(2 * W) // 2
    for c in range(3):
        r = dm.drizzle(sc['mosaic'][:1], sc['affines'][:1], 2, 0.5, cfa=(sc['pattern'], c))
        reach = (src_j[:, None] < H) & (src_i[None, :] < W)
        reach &= sc['chan'][np.minimum(src_j, H - 1)[:, None], np.minimum(src_i, W - 1)[None, :]] == c
        assert np.array_equal(r['weight'] > 0, reach) and np.array_equal(np.isnan(r['image']), ~reach)


REJECT_FALSE_CAP = 5e-4


def reject_scene():
    """The star scene on a sky of 100 with Gaussian noise of 5, and 40 hits of 10 to 40 sigma at known sky pixels of single frames."""
    clean = dm.scene(noise=5.0, sky=100.0, seed=11)
    rng = np.random.default_rng(12)
    frames = clean['frames'].copy()
    N, H, W = frames.shape
    hits = []
    while len(hits) < 40:
        f, r, c = int(rng.integers(N)), int(rng.integers(4, H - 4)), int(rng.integers(4, W - 4))
        sx, sy = clean['shifts'][f]
        if min(np.hypot(c - (x + sx), r - (y + sy)) for x, y, _ in clean['stars']) < 5 or (f, r, c) in hits:
            continue
        hits.append((f, r, c))
        frames[f, r, c] += rng.uniform(10, 40) * clean['noise']
    return dict(clean, clean_frames=clean['frames'], frames=frames, hits=hits)


def median_reference(frames, affines):
    """The blot reference: the median, over the frames that reach a pixel, of the frames drizzled one by one onto the s = 2 grid
    with p = 0.5 (a single frame reaches a quarter of it).  The same median on the s = 1 grid with p = 1 is too smooth for stars of
    sigma_0 = 0.5: measured, it has 27 peak pixels of the hit-free frames flagged at grow = 1.2."""
    each = np.stack([dm.drizzle(frames[k], affines[k:k + 1], 2, 0.5)['image'] for k in range(len(frames))])
    with np.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return np.nanmedian(each, 0).astype(F)


def test_rejection():
    """Hits of at least 10 sigma are all flagged; no flag falls within 2 pixels of a star's centre in the hit-free frames (the
    grow d term: the reference's spread under an undersampled core is hundreds of ADU); the drizzle is closer to the hit-free one with
    the flags than without.  Measured with the model on the CPU (seeds 11 / 12, k 3.5, grow 1.2): 40 of 40 hits flagged, 0 flags
    on the 16 x 4 star cores, false-flag share on the clean pixels 0 of 39 896 (the threshold is 3.5 sigma_i + 1.2 d with d about one
    sigma of the reference's noise: 4 sigma and more, 6e-5 two-sided for a Gaussian, about two pixels expected); rms against the
    hit-free drizzle 1.60 without and 0.049 with the flags.  Cap: 5e-4, twenty pixels, well above the expected two."""
    sc = reject_scene()
    N, H, W = sc['frames'].shape
    sig = np.full(N, sc['noise'])
    ref = median_reference(sc['frames'], sc['affines'])
    flags = dm.drizzle_reject(sc['frames'], sc['affines'], ref, 2.0, None, sig)
    hit = np.zeros(flags.shape, bool)
    for f, r, c in sc['hits']:
        hit[f, r, c] = True
    assert flags[hit].all()
    clean_flags = dm.drizzle_reject(sc['clean_frames'], sc['affines'], median_reference(sc['clean_frames'], sc['affines']), 2.0, None, sig)
    cores = 0
    for f, (sx, sy) in enumerate(sc['shifts']):
        for x, y, _ in sc['stars']:
            r0, c0 = int(round(y + sy)), int(round(x + sx))
            cores += int(clean_flags[f, r0 - 2:r0 + 3, c0 - 2:c0 + 3].sum())
    assert cores == 0
    false_share = float(flags[~hit].mean())
    truth = dm.drizzle(sc['clean_frames'], sc['affines'], 2, 0.5)['image']
    plain = dm.drizzle(sc['frames'], sc['affines'], 2, 0.5)['image']
    clipped = dm.drizzle(sc['frames'], sc['affines'], 2, 0.5, frame_masks=flags)['image']
    ok = np.isfinite(truth) & np.isfinite(plain) & np.isfinite(clipped)
    rms0 = float(np.sqrt(np.mean((plain[ok].astype(np.float64) - truth[ok]) ** 2)))
    rms1 = float(np.sqrt(np.mean((clipped[ok].astype(np.float64) - truth[ok]) ** 2)))
    print('hits flagged %d / %d, flags on hit-free star cores %d, false-flag share %.3e (%d of %d), rms %.4f without, %.4f with'
          % (int(flags[hit].sum()), len(sc['hits']), cores, false_share, int(flags[~hit].sum()), int((~hit).sum()), rms0, rms1))
    assert false_share <= REJECT_FALSE_CAP
    assert rms1 < rms0


def test_argument_errors():
    fr = np.ones((2, 8, 9), F)
    ident = [dm.shift_affine(0, 0)]
    with pytest.raises(ValueError, match='footprint'):
        dm.drizzle(fr, [dm.shift_affine(0, 0, 0, 2.2)], 1, 0.5)      # lx = 2.2 input pixels per output pixel
    dm.drizzle(fr, [dm.shift_affine(0, 0, 0, 2.0)], 1, 0.5)          # lx = 2 is allowed
    with pytest.raises(ValueError, match='footprint'):
        dm.drizzle(fr, ident, 0.4, 0.5)
    for p in (0.0, -0.5, 1.01, float('nan')):
        with pytest.raises(ValueError, match='pixfrac'):
            dm.drizzle(fr, ident, 2, p)
    for w in ([1.0, 0.0], [1.0, -2.0], [1.0, float('inf')], [1.0, float('nan')], [1.0]):
        with pytest.raises(ValueError, match='weights'):
            dm.drizzle(fr, ident, 2, 0.5, weights=w)
    with pytest.raises(ValueError, match='mask'):
        dm.drizzle(fr, ident, 2, 0.5, mask=np.zeros((9, 8), bool))
    with pytest.raises(ValueError, match='frame_masks'):
        dm.drizzle(fr, ident, 2, 0.5, frame_masks=np.zeros((8, 9), bool))
    with pytest.raises(ValueError, match='affines'):
        dm.drizzle(fr, [dm.shift_affine(0, 0)] * 3, 2, 0.5)
    with pytest.raises(ValueError, match='singular'):
        dm.drizzle_reject(fr, [[1, 0, 0, 2, 0, 0]], np.ones((8, 9), F))
