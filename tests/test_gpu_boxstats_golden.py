"""box_stats_kernel (csrc/background.hip) on every launch form: against golden group G15 - astropy's own SigmaClip +
np.nanmedian / np.nanstd per box, as photutils' Background2D calls them (tests/golden/make_golden_boxstats.py) - and, beyond
the fixture's sizes, against oracle/background_ref.box_clipped_stats, which tests/test_oracle_golden.py holds to G15 as well.

Launch forms by box pixel count (background.hip, apgpu_box_clipped_stats_f32):
    <256, resident>        <= 8192 pixels       G15 boxes 64x70, 40x45, 16x20; here 1x1, 1x700, 700x1, 64x64
    <1024, resident>       8193 .. 32768        G15 boxes 110x120, 100x100, 150x170; here 128x128, 100x150
    <1024, non-resident>   > 32768              G15 boxes 182x184 (3 x 3 meshes, ragged); here 256x256 on 4096^2, 200x200
"""
import numpy as np
import pytest

from tests.util import G15_ORACLE_STD_DEV, g15_cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

STD_RTOL = max(1e-12, 4 * G15_ORACLE_STD_DEV)        # 4 x: another summation order over at most 2^24 float64 terms


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from astrophotography_amd import ops as _ops
    return _ops


def _run(ops, img, mask, bh, bw, sigma, maxiters):
    d = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    return ops.box_clipped_stats(d, m, bh, bw, sigma=sigma, maxiters=maxiters).cpu().numpy()


def _check(st, median, std_ref, count, nmasked0, rtol, what):
    assert st.dtype == np.float64 and st.shape == median.shape + (4,), what
    bad = np.argwhere(st[..., 2].astype(np.int64) != count)
    assert bad.size == 0, '%s: survivor counts differ in %d boxes, first %s: %s vs %s' % (
        what, len(bad), bad[0], st[..., 2][tuple(bad[0])], count[tuple(bad[0])])
    assert np.array_equal(st[..., 3].astype(np.int64), nmasked0), what + ': pre-clip masked counts'
    assert np.array_equal(st[..., 0], median, equal_nan=True), what + ': medians'
    assert np.array_equal(np.isnan(st[..., 1]), np.isnan(std_ref)), what + ': NaN std'
    f = ~np.isnan(std_ref)
    err = np.abs(st[..., 1][f] - std_ref[f])
    assert np.all(err <= rtol * std_ref[f]), '%s: std off by %.3e (relative), bound %.1e' % (
        what, float(np.max(err / np.maximum(std_ref[f], 1e-300))), rtol)


def test_g15_kernel_matches_astropy(ops):
    """Every case of G15, none filtered: survivor count, pre-clip masked count and median EXACT in astropy's dtype (float64),
    std within max(1e-12, 4 x 1.3e-13) = 1e-12 of the high-precision (math.fsum) value recorded in the fixture."""
    n, forms = 0, set()
    for c in g15_cases():
        assert c['dtype'] == 'float64'
        what = '%s %s box %s (%s) sigma %s maxiters %s' % (c['file'], c['name'], c['box'], c['form'], c['sigma'], c['maxiters'])
        st = _run(ops, c['img'], c['mask_arr'], c['box'][0], c['box'][1], c['sigma'], c['maxiters'])
        _check(st, c['median'], c['std_hp'], c['count'], c['nmasked0'], STD_RTOL, what)
        forms.add(c['form'])
        n += 1
    assert n == 72 and forms == {'256-resident', '1024-resident', '1024-non-resident'}


def _stamp_stars(rng, img, n):
    H, W = img.shape
    for _ in range(n):
        cy, cx, amp, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(100, 20000), rng.uniform(1.2, 2.5)
        r = int(6 * s) + 2
        y0, y1, x0, x1 = max(0, int(cy) - r), min(H, int(cy) + r), max(0, int(cx) - r), min(W, int(cx) + r)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        img[y0:y1, x0:x1] += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))


def _sky(rng, H, W, level=300.0, nstars=None):
    img = rng.normal(level, 6.0, (H, W))
    img += 0.002 * np.arange(W)[None, :] + 0.001 * np.arange(H)[:, None]
    _stamp_stars(rng, img, nstars if nstars is not None else max(3, H * W // 4000))
    return img.astype(np.float32)


def _vs_oracle(ops, img, mask, bh, bw, sigma=3.0, maxiters=5, what=''):
    from oracle import background_ref as br
    med, std, nfin, nm0 = br.box_clipped_stats(img, mask, bh, bw, sigma, maxiters)
    st = _run(ops, img, mask, bh, bw, sigma, maxiters)
    _check(st, med, std, nfin, nm0, 1e-12, '%s %dx%d boxes %dx%d sigma %s maxiters %s' % (what, img.shape[0], img.shape[1], bh, bw, sigma, maxiters))
    return st


@pytest.mark.parametrize('masked', (False, True))
def test_full_frame_default_mesh(ops, masked):
    """A 4096 x 4096 frame with ApMeasureBackground's default 16 x 16 mesh: 256 non-resident boxes of 65536 pixels, sky near
    zero (a background-subtracted frame: the speculated second radix level misses) with NaN / inf pixels."""
    rng = np.random.default_rng(1510 + masked)
    img = _sky(rng, 4096, 4096, level=0.2, nstars=3000)
    img[17, 4000] = np.nan
    img[2000:2010, 300:340] = np.inf
    mask = None
    if masked:
        mask = (rng.random(img.shape) < 0.03).astype(np.uint8)
        mask[256:512, 512:768] = 1                                          # one box fully masked
        mask[1024:1280, 0:256] = 1
        mask[1100, 100] = 0                                                 # one box with a single unmasked pixel
    st = _vs_oracle(ops, img, mask, 256, 256, what='full frame')
    assert st.shape == (16, 16, 4)
    if masked:
        assert st[1, 2, 2] == 0 and np.isnan(st[1, 2, 0]) and st[4, 0, 2] == 1 and st[4, 0, 1] == 0


def test_mid_form_and_ragged_meshes_float_and_rint(ops):
    """1024 x 1536: 128 x 128 boxes (16384 pixels: the 1024-thread resident form) and 100 x 150 boxes (ragged last row and
    column); the same image as float sky and as its np.rint copy (integer ties)."""
    rng = np.random.default_rng(1520)
    img = _sky(rng, 1024, 1536)
    mask = (rng.random(img.shape) < 0.02).astype(np.uint8)
    for im in (img, np.rint(img)):
        for (bh, bw) in ((128, 128), (100, 150)):
            for (sigma, maxiters, m) in ((3.0, 5, mask), (2.0, 10, None)):
                _vs_oracle(ops, im, m, bh, bw, sigma, maxiters, what='rint' if im is not img else 'float')


def test_degenerate_shapes(ops):
    """Box larger than the image (resident and non-resident), 1 x 1 boxes, images one pixel high or wide."""
    rng = np.random.default_rng(1530)
    small = _sky(rng, 50, 60, level=-3.0)
    small[4, 4] = np.nan
    msmall = (rng.random(small.shape) < 0.1).astype(np.uint8)
    for im in (small, np.rint(small)):
        _vs_oracle(ops, im, msmall, 64, 64, what='box larger than the image')
        _vs_oracle(ops, im, None, 1, 1, what='1x1 boxes')
        _vs_oracle(ops, im, msmall, 1, 1, sigma=0.5, maxiters=0, what='1x1 boxes')
    mid = _sky(rng, 150, 170, level=0.1)
    mid[100:104, 20:30] = -np.inf
    mmid = (rng.random(mid.shape) < 0.05).astype(np.uint8)
    for im in (mid, np.rint(mid)):
        _vs_oracle(ops, im, mmid, 200, 200, what='non-resident box larger than the image')
        _vs_oracle(ops, im, None, 200, 170, sigma=2.0, maxiters=10, what='non-resident box higher than the image')
    row = _sky(rng, 1, 5000, level=0.5, nstars=20)
    col = np.ascontiguousarray(row.T)
    for im, (bh, bw) in ((row, (1, 700)), (col, (700, 1)), (row, (1, 5000)), (col, (3, 1)), (np.rint(row), (1, 700))):
        _vs_oracle(ops, im, None, bh, bw, sigma=2.0, maxiters=5, what='one pixel high / wide')
    with pytest.raises(Exception):
        ops.box_clipped_stats(torch.from_numpy(small).cuda(), None, 5000, 5000)         # above 2^24 pixels per box: refused
