"""L.A.Cosmic (csrc/lacosmic.hip) where tests/test_gpu_lacosmic.py does not go: cosmic rays on the border rows and columns
and in the corners, every parameter away from its default, input masks (the 'no good neighbour -> background level' branch
among them), non-finite pixels, images smaller than a filter window and larger than a convolution tile.  Reference:
oracle/lacosmic_ref.detect_cosmics (its helpers are held to scipy.ndimage by tests/test_oracle_lacosmic_scipy.py) -
mask and cleaned image bit for bit, and the number of iterations run."""
import numpy as np
import pytest

from tests.util import assert_biteq

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from astrophotography_amd import ops as _ops
    return _ops


def _field(rng, H, W, ncr=30, nstars=None, saturated=True):
    """Sky + stars + (optionally) a saturated star + cosmic rays: on every border row / column 0, 1, 2, H-3 .. H-1,
    W-3 .. W-1, in the four corners, and `ncr` anywhere (borders included)."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = rng.normal(400.0, 8.0, (H, W))
    for _ in range(nstars if nstars is not None else max(2, H * W // 700)):
        cy, cx, amp = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(200, 8000)
        r = 10
        y0, y1, x0, x1 = max(0, int(cy) - r), min(H, int(cy) + r), max(0, int(cx) - r), min(W, int(cx) + r)
        img[y0:y1, x0:x1] += amp * np.exp(-((xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2) / (2 * 1.5 ** 2))
    if saturated and min(H, W) >= 30:
        cy, cx = int(H * 0.6), int(W * 0.3)
        y0, y1, x0, x1 = max(0, cy - 20), min(H, cy + 20), max(0, cx - 20), min(W, cx + 20)
        img[y0:y1, x0:x1] += 400000.0 * np.exp(-((xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2) / (2 * 2.0 ** 2))
    img = np.minimum(img, 65535.0)
    truth = np.zeros((H, W), bool)

    def hit(r, c, amp=None):
        if 0 <= r < H and 0 <= c < W:
            img[r, c] += rng.uniform(800, 6000) if amp is None else amp
            truth[r, c] = True
    for k in (0, 1, 2):
        for edge_r in (k, H - 1 - k):
            hit(edge_r, int(rng.integers(0, W)))
            hit(edge_r, int(rng.integers(0, W)))
        for edge_c in (k, W - 1 - k):
            hit(int(rng.integers(0, H)), edge_c)
            hit(int(rng.integers(0, H)), edge_c)
    for (r, c) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        hit(r, c, 3000.0)
    for _ in range(ncr):
        r, c = int(rng.integers(0, H)), int(rng.integers(0, W))
        for k in range(int(rng.integers(1, 4))):
            hit(r + k, c + (k if rng.random() < 0.5 else 0))
    return img.astype(np.float32), truth


def _compare(ops, img, what, inmask=None, **kw):
    from oracle import lacosmic_ref as L
    satlevel = kw.pop('satlevel', 65535.0)
    ref_clean, ref_mask, info = L.detect_cosmics(img, gain=1.0, satlevel=satlevel, inmask=inmask, return_info=True, **kw)
    d = torch.from_numpy(img).cuda()
    m = None if inmask is None else torch.from_numpy(np.ascontiguousarray(inmask, np.uint8)).cuda()
    clean, crmask, niter = ops.lacosmic(d, inmask=m, satlevel=satlevel, **kw)
    what = '%s %s %s' % (what, img.shape, kw)
    assert np.array_equal(crmask.cpu().numpy().astype(bool), ref_mask), what + ': cosmic-ray mask'
    assert_biteq(clean.cpu().numpy(), ref_clean, what + ': cleaned image')
    assert niter == info['niter'], what + ': iterations run %d, oracle %d' % (niter, info['niter'])
    # nothing within 2 pixels of the border is ever modified
    H, W = img.shape
    border = np.ones((H, W), bool)
    border[2:H - 2, 2:W - 2] = False
    assert_biteq(clean.cpu().numpy()[border], img[border], what + ': border pixels')
    return ref_clean, ref_mask, info


SHAPES = ((4, 40), (40, 4), (8, 8), (16, 70), (65, 17), (120, 150))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('fsmode', ('convolve', 'median'))
def test_border_cosmic_rays_every_shape(ops, shape, fsmode):
    rng = np.random.default_rng(7000 + 131 * shape[0] + shape[1])
    img, truth = _field(rng, *shape, ncr=max(2, shape[0] * shape[1] // 500))
    _, ref_mask, info = _compare(ops, img, 'borders', fsmode=fsmode)
    if shape == (120, 150):
        H, W = shape
        border = np.ones(shape, bool)
        border[3:H - 3, 3:W - 3] = False
        assert (ref_mask & truth & border).sum() >= 10          # border cosmic rays ARE detected (and, above, left uncleaned)
        assert info['niter'] >= 2


PARAMS = [dict(sigclip=3.0), dict(sigclip=6.0), dict(sigfrac=0.1), dict(sigfrac=1.0), dict(objlim=1.0), dict(objlim=20.0),
          dict(readnoise=0.0), dict(readnoise=50.0), dict(niter=1), dict(niter=8), dict(psffwhm=2.0), dict(psffwhm=5.0),
          dict(fsmode='median', objlim=1.0), dict(fsmode='median', sigclip=3.0, niter=8),
          dict(sigclip=3.0, sigfrac=0.1, objlim=1.0, readnoise=0.0, niter=8, psffwhm=2.0),
          dict(sigclip=6.0, sigfrac=1.0, objlim=20.0, readnoise=50.0, niter=1, psffwhm=5.0, fsmode='median'),
          dict(sigclip=3.0, sigfrac=1.0, objlim=20.0, readnoise=0.0, niter=8, psffwhm=5.0)]


@pytest.mark.parametrize('kw', PARAMS, ids=lambda kw: ','.join('%s=%s' % i for i in kw.items()))
def test_non_default_parameters(ops, kw):
    rng = np.random.default_rng(7100)
    img, _ = _field(rng, 90, 131, ncr=40)
    _, ref_mask, info = _compare(ops, img, 'parameters', **kw)
    assert info['niter'] <= kw.get('niter', 6)
    if kw.get('niter') == 1:
        assert info['niter'] == 1


def test_parameters_change_the_result(ops):
    """The parameter sets above are different computations: the oracle's masks differ between them."""
    from oracle import lacosmic_ref as L
    rng = np.random.default_rng(7100)
    img, _ = _field(rng, 90, 131, ncr=40)
    base = L.detect_cosmics(img)[1]
    for kw in (dict(sigclip=3.0), dict(sigclip=6.0), dict(sigfrac=1.0), dict(objlim=20.0), dict(readnoise=50.0), dict(niter=1)):
        assert not np.array_equal(L.detect_cosmics(img, **kw)[1], base), kw


def test_input_masks(ops):
    rng = np.random.default_rng(7200)
    H, W = 100, 140
    img, truth = _field(rng, H, W, ncr=40)
    random2 = rng.random((H, W)) < 0.02
    _compare(ops, img, 'random 2 % mask', inmask=random2)
    block = np.zeros((H, W), bool)
    block[30:55, 60:100] = True
    block[0:4, 0:9] = True                                           # a masked corner
    _compare(ops, img, 'block mask', inmask=block)
    # a 7 x 7 block with a 3 x 3 hole centred on a cosmic ray: the one-pixel grow leaves the ray alone in a 9 x 9 masked
    # block - no good neighbour in its 5 x 5 window, it takes the background level
    img2 = img.copy()
    cy, cx = 20, 110
    img2[cy - 6:cy + 7, cx - 6:cx + 7] = rng.normal(400.0, 8.0, (13, 13)).astype(np.float32)
    img2[cy, cx] += 5000.0
    hole = np.zeros((H, W), bool)
    hole[cy - 3:cy + 4, cx - 3:cx + 4] = True
    hole[cy - 1:cy + 2, cx - 1:cx + 2] = False
    for extra in (None, random2):
        inmask = hole if extra is None else (hole | (extra & ~hole & (np.hypot(*np.mgrid[-cy:H - cy, -cx:W - cx]) > 8)))
        ref_clean, ref_mask, info = _compare(ops, img2, 'hole mask', inmask=inmask)
        assert not info['mask'][cy, cx] and info['mask'][cy - 2:cy + 3, cx - 2:cx + 3].sum() == 24
        assert (cy, cx) in info['background_pixels'] and ref_mask[cy, cx]             # the branch was taken ...
        assert ref_clean[cy, cx] == info['background'] and 380.0 < info['background'] < 420.0     # ... with the median level


def test_everything_masked_and_nothing_to_find(ops):
    rng = np.random.default_rng(7300)
    img = rng.normal(400.0, 8.0, (40, 50)).astype(np.float32)
    _, m, info = _compare(ops, img, 'all masked', inmask=np.ones(img.shape, bool))
    assert not m.any() and info['niter'] == 1 and info['background'] == 0
    _, m, info = _compare(ops, img, 'quiet sky', sigclip=8.0)
    assert not m.any() and info['niter'] == 1
    _compare(ops, img, 'niter 0', niter=0)


def test_nonfinite_pixels_through_the_class(ops):
    """ApFixCosmicRays.process zeroes and masks NaN / inf pixels and hands them back unchanged."""
    import astrophotography_amd as ap
    from oracle import lacosmic_ref as L
    rng = np.random.default_rng(7400)
    H, W = 80, 96
    img, _ = _field(rng, H, W, ncr=25)
    img[10, 12] = np.nan
    img[0, 0] = np.inf
    img[H - 1, 40] = -np.inf
    img[40:43, 50:52] = np.nan
    img[41, 53] += 4000.0                                              # a cosmic ray next to the NaN block
    gain = 1.3
    fx = ap.ApFixCosmicRays('CRITICAL')
    clean, kw = fx.process(img, gain)
    ref_clean, ref_mask = L.detect_cosmics(img, gain=gain, satlevel=gain * 65535)
    ref_adu = ref_clean / np.float32(gain)
    bad = ~np.isfinite(img)
    assert_biteq(clean[bad], img[bad], 'non-finite pixels come back as they went in')
    assert_biteq(clean[~bad], ref_adu[~bad], 'ApFixCosmicRays.process with non-finite pixels')
    assert np.array_equal(fx.get_crmask().astype(bool), ref_mask) and not ref_mask[bad].any()
    assert kw['CR_NPIX'][0] == int(ref_mask.sum()) > 10


def test_frame_larger_than_many_tiles(ops):
    """1024 x 1536: 16 x 24 convolution tiles (64 x 16) with ragged... none - plus 1000 x 1531, ragged in both directions."""
    rng = np.random.default_rng(7500)
    for (H, W, kw) in ((1024, 1536, dict(niter=2)), (1000, 1531, dict(niter=2, fsmode='median'))):
        img, truth = _field(rng, H, W, ncr=400, nstars=300)
        _, ref_mask, info = _compare(ops, img, 'large', **kw)
        assert (ref_mask & truth).sum() >= 0.7 * truth[3:-3, 3:-3].sum() and info['niter'] == 2
