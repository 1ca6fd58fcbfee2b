"""The source mask of ApMeasureBackground (csrc/background.hip: lock-free union-find labelling with a minimum-area filter,
then a square dilation) against scipy.ndimage directly: label(structure=ones((3, 3))) + bincount + binary_dilation.  Exact
mask, exact component count - on patterns whose components hold together only through the diagonal links, wind through the
whole image, sit on workgroup boundaries of the flat pixel index, or fill / empty the image."""
import numpy as np
import pytest
from scipy import ndimage

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from astrophotography_amd import ops as _ops
    return _ops


def _reference(fg, min_pixels, dilate_size):
    lab, nlab = ndimage.label(fg, structure=np.ones((3, 3), int))
    sizes = np.bincount(lab.ravel(), minlength=nlab + 1)
    keep = sizes >= min_pixels
    keep[0] = False
    seg = keep[lab]
    H, W = fg.shape
    if dilate_size > 2 * max(H, W):                     # wider than the image: every row and column of a source, then all
        mask = np.full(fg.shape, bool(seg.any()))
    else:
        mask = ndimage.binary_dilation(seg, structure=np.ones((dilate_size, dilate_size), bool), border_value=0)
    return mask, int(keep.sum())


def _compare(ops, fg, min_pixels, dilate_size, what):
    fg = np.ascontiguousarray(fg, np.uint8)
    ref_mask, ref_n = _reference(fg.astype(bool), min_pixels, dilate_size)
    mask, nsrc = ops.source_mask(torch.from_numpy(fg).cuda(), min_pixels, dilate_size)
    what = '%s %s min_pixels=%d dilate=%d' % (what, fg.shape, min_pixels, dilate_size)
    assert int(nsrc.item()) == ref_n, what
    got = mask.cpu().numpy()
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}, what
    assert np.array_equal(got.astype(bool), ref_mask), what
    return ref_n


def _checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy + xx) % 2 == 0


def _diagonals(H, W, slope):
    """Lines one pixel wide, 6 apart, joined only through their NE (slope -1) or NW (slope +1) neighbours."""
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx + slope * yy) % 6 == 0


def _double_spiral(H, W):
    """Two interleaved rectangular spirals, 1 and 2, one pixel wide and one pixel apart: a spiral walk on the half-resolution
    grid (turn right when the cell two ahead is taken) is arm 1, the corridor it leaves is arm 2."""
    h, w = (H + 1) // 2, (W + 1) // 2
    A = np.zeros((h, w), bool)

    def taken(r, c):
        return not (0 <= r < h and 0 <= c < w) or A[r, c]
    r, c, dr, dc = 0, 0, 0, 1
    while True:
        A[r, c] = True
        if taken(r + dr, c + dc) or (0 <= r + 2 * dr < h and 0 <= c + 2 * dc < w and A[r + 2 * dr, c + 2 * dc]):
            dr, dc = dc, -dr
            if taken(r + dr, c + dc) or (0 <= r + 2 * dr < h and 0 <= c + 2 * dc < w and A[r + 2 * dr, c + 2 * dc]):
                break
        r, c = r + dr, c + dc
    out = np.zeros((2 * h - 1, 2 * w - 1), np.uint8)
    for arm, cells in ((1, A), (2, ~A)):
        out[::2, ::2][cells] = arm
        out[1::2, ::2][cells[:-1] & cells[1:]] = arm
        out[::2, 1::2][cells[:, :-1] & cells[:, 1:]] = arm
    return out


def _comb(H, W):
    a = np.zeros((H, W), bool)
    a[0, :] = True
    a[:, ::2] = True                                      # teeth one pixel apart, joined at the top row only
    a[H // 2, 1::4] = False
    return a


def _patterns():
    yield 'checkerboard', _checkerboard(64, 96)
    yield 'checkerboard', _checkerboard(512, 512)
    yield 'checkerboard-odd', _checkerboard(61, 37)
    yield 'diagonal-ne', _diagonals(200, 317, +1)
    yield 'diagonal-nw', _diagonals(200, 317, -1)
    yield 'diagonal-both', _diagonals(128, 128, +1) | _diagonals(128, 128, -1)
    sp = _double_spiral(257, 300)
    yield 'spiral-arm-1', sp == 1
    yield 'spiral-arm-2', sp == 2
    yield 'spiral-512', _double_spiral(512, 512) == 1
    yield 'comb', _comb(300, 301)
    rng = np.random.default_rng(1540)
    for fill in (0.05, 0.3, 0.6):
        yield 'random-%.2f' % fill, rng.random((512, 512)) < fill
        yield 'random-%.2f' % fill, rng.random((97, 263)) < fill
    yield 'ones', np.ones((130, 70), bool)
    yield 'zeros', np.zeros((130, 70), bool)
    for shape in ((1, 700), (700, 1), (2, 2), (1, 1)):
        yield 'line-ones', np.ones(shape, bool)
        yield 'line-random', rng.random(shape) < 0.6
        yield 'line-zeros', np.zeros(shape, bool)


@pytest.mark.parametrize('min_pixels', (1, 5))
def test_patterns_match_scipy(ops, min_pixels):
    n = 0
    for name, fg in _patterns():
        H, W = fg.shape
        for dilate_size in (1, 3, 13, 2 * max(H, W) + 1):
            if dilate_size > 1 and H * W > 100000 and name.startswith('random') and dilate_size != 13:
                continue                                   # (the reference's dilation is the slow part: one width on the big fields)
            _compare(ops, fg, min_pixels, dilate_size, name)
            n += 1
    assert n > 60


def test_diagonal_links_are_single_components(ops):
    """What scipy says about the patterns above, so that they test what they are meant to: the checkerboard and each
    diagonal line hold together only through diagonal neighbours."""
    assert ndimage.label(_checkerboard(64, 96), structure=np.ones((3, 3), int))[1] == 1
    assert ndimage.label(_checkerboard(64, 96))[1] == 64 * 96 // 2                      # 4-connectivity: every pixel alone
    for slope in (+1, -1):
        fg = _diagonals(200, 317, slope)
        n8 = ndimage.label(fg, structure=np.ones((3, 3), int))[1]
        assert n8 < 100 and ndimage.label(fg)[1] == fg.sum()
        assert _compare(ops, fg, 5, 1, 'diagonal') >= n8 - 8                             # all but the corner stubs survive
    sp = _double_spiral(257, 300)
    for arm in (1, 2):
        assert ndimage.label(sp == arm, structure=np.ones((3, 3), int))[1] == 1 and (sp == arm).sum() > 15000
    assert ndimage.label(sp > 0, structure=np.ones((3, 3), int))[1] == 2


@pytest.mark.parametrize('W', (256, 512, 300, 1024))
def test_blobs_across_workgroup_boundaries(ops, W):
    """Components of exactly min_pixels - 1 and min_pixels pixels laid across multiples of 256 in the flat pixel index
    (one workgroup's first sweep ends there), as horizontal runs, vertical runs and diagonal steps."""
    min_pixels = 5
    fg = _blobs(W, min_pixels)
    lab, nlab = ndimage.label(fg, structure=np.ones((3, 3), int))
    sizes = np.bincount(lab.ravel())[1:]
    assert set(sizes) == {2, min_pixels - 1, min_pixels} and (sizes == min_pixels).sum() >= 4 and (sizes == min_pixels - 1).sum() >= 4
    for mp in (1, min_pixels - 1, min_pixels):
        for dilate_size in (1, 3):
            assert _compare(ops, fg, mp, dilate_size, 'blobs') == (sizes >= mp).sum()


def _blobs(W, min_pixels, H=44):
    fg = np.zeros((H, W), np.uint8)
    slot = 0
    for size in (min_pixels - 1, min_pixels):
        for lead in range(0, size + 1):                    # `lead` pixels before the boundary, the rest after it
            r = 1 + 2 * slot                               # every blob on a row of its own, an empty row between two
            slot += 1
            c = (-r * W) % 256                             # (r, c) is a multiple of 256 in the flat index
            if c < lead:
                c += 256
            if c + size - lead <= W:
                fg[r, c - lead:c - lead + size] = 1
    # vertical and diagonal blobs
    for i, size in enumerate((min_pixels - 1, min_pixels, min_pixels - 1, min_pixels)):
        r0, c0 = 2 * slot + 2, 10 + 12 * i
        for j in range(size):
            fg[r0 + j, c0 + (j if i >= 2 else 0)] = 1
    # neighbours in the flat index that are no neighbours in the image: the end of one row and the start of the next
    r = r0 + min_pixels + 2
    fg[r, W - 2:] = 1
    fg[r + 1, :2] = 1
    return fg


def test_frame_sized_star_field(ops):
    """A 4096 x 4096 thresholded star field (what ApMeasureBackground hands the kernels), default npixels=5 and size 13."""
    rng = np.random.default_rng(1550)
    H = W = 4096
    img = rng.normal(300.0, 6.0, (H, W)).astype(np.float32)
    for _ in range(4000):
        cy, cx, amp, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(100, 20000), rng.uniform(1.2, 2.5)
        r = int(6 * s) + 2
        y0, y1, x0, x1 = max(0, int(cy) - r), min(H, int(cy) + r), max(0, int(cx) - r), min(W, int(cx) + r)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        img[y0:y1, x0:x1] += (amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))).astype(np.float32)
    img[rng.integers(0, H, 4000), rng.integers(0, W, 4000)] += 500.0                     # hot pixels: below 5 connected pixels
    fg = img > np.float32(312.0)                                                          # 2 sigma: ~2 % of the sky pixels too
    n = _compare(ops, fg, 5, 13, 'star field')
    assert n > 3000
