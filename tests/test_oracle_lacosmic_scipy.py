"""The hand-written helpers of oracle/lacosmic_ref.py against scipy.ndimage (CPU only).  The L.A.Cosmic kernels are held to
the oracle bit for bit; these tests hold the oracle's building blocks to a third-party implementation of the same
operation, with bounds derived from the float32 arithmetic the oracle declares."""
import numpy as np
import pytest
from scipy import ndimage

from oracle import lacosmic_ref as L

U = 2.0 ** -24                  # unit roundoff of float32


def _images(rng):
    for shape in ((40, 57), (9, 9), (6, 30), (30, 4), (1, 20), (20, 1), (3, 3), (64, 65)):
        yield rng.normal(100, 20, shape).astype(np.float32)
        yield np.rint(rng.normal(100, 3, shape)).astype(np.float32)           # ties
        a = rng.normal(0, 50, shape).astype(np.float32)                       # both signs, isolated spikes
        a[rng.random(shape) < 0.05] += 5000
        yield a


@pytest.mark.parametrize('size', (5, 7, 9))
def test_sepmedfilt_is_two_1d_median_filters_with_copied_borders(size):
    rng = np.random.default_rng(600 + size)
    h = size // 2
    for a in _images(rng):
        H, W = a.shape
        out = L.sepmedfilt(a, size)
        rows = a.copy()
        if W >= size:
            rows[:, h:W - h] = ndimage.median_filter(a, size=(1, size), mode='nearest')[:, h:W - h]
        ref = rows.copy()
        if H >= size:
            ref[h:H - h, :] = ndimage.median_filter(rows, size=(size, 1), mode='nearest')[h:H - h, :]
        assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), ref.view(np.uint32)), (a.shape, size)
        # what is copied: the first / last h columns through the row pass, the first / last h rows through the column pass -
        # so the border rows are the row-filtered image and the four h x h corners are the input itself
        hr, hc = min(h, H), min(h, W)
        assert np.array_equal(rows[:, :hc], a[:, :hc]) and np.array_equal(rows[:, W - hc:], a[:, W - hc:])
        assert np.array_equal(out[:hr], rows[:hr]) and np.array_equal(out[H - hr:], rows[H - hr:])
        for cr in (slice(0, hr), slice(H - hr, H)):
            for cc in (slice(0, hc), slice(W - hc, W)):
                assert np.array_equal(out[cr, cc], a[cr, cc])


def test_dilate_is_binary_dilation_with_zero_border():
    rng = np.random.default_rng(610)
    five = np.ones((5, 5), bool)
    five[0, 0] = five[0, 4] = five[4, 0] = five[4, 4] = False
    for shape in ((40, 57), (9, 9), (1, 20), (20, 1), (2, 2), (5, 3), (64, 64)):
        for fill in (0.0, 0.02, 0.3, 1.0):
            m = rng.random(shape) < fill
            m[0, 0] = m[-1, -1] = fill > 0                                        # corners and borders set
            assert np.array_equal(L.dilate(m, 3), ndimage.binary_dilation(m, structure=np.ones((3, 3), bool), border_value=0))
            assert np.array_equal(L.dilate(m, 5), ndimage.binary_dilation(m, structure=five, border_value=0))


def test_convolve7_against_float64_correlate():
    """float32 accumulation of 49 products: |error| <= 49 * 2^-24 * sum |k a| per pixel (each product and each of the 48
    additions rounds once, relative 2^-24, on partial sums bounded by sum |k a|; the float64 reference's own error, 49 * 2^-53,
    is nine orders below).  The kernel is float32 in both, widened exactly."""
    rng = np.random.default_rng(620)
    for fwhm in (2.0, 3.5, 5.0):
        k = L.gausskernel(fwhm, 7)
        assert k.dtype == np.float32 and k.shape == (7, 7) and abs(float(k.astype(np.float64).sum()) - 1.0) < 49 * U
        for a in _images(rng):
            out = L.convolve7(a, k)
            ref = ndimage.correlate(a.astype(np.float64), k.astype(np.float64), mode='constant', cval=0.0)
            bound = 49 * U * ndimage.correlate(np.abs(a).astype(np.float64), np.abs(k).astype(np.float64), mode='constant', cval=0.0)
            assert out.dtype == np.float32
            assert np.all(np.abs(out.astype(np.float64) - ref) <= bound), (fwhm, a.shape)
    a = np.zeros((12, 13), np.float32)
    a[0, 0] = a[11, 12] = a[5, 6] = 1.0                                   # an asymmetric kernel: correlation, not convolution
    k = rng.random((7, 7)).astype(np.float32)
    assert np.array_equal(L.convolve7(a, k), ndimage.correlate(a.astype(np.float64), k.astype(np.float64), mode='constant').astype(np.float32))


def test_laplace_rebin_against_float64_on_the_subsampled_image():
    """Reference: the image subsampled 2 x explicitly, the 0 -1 0 / -1 4 -1 / 0 -1 0 kernel with nothing outside the image,
    negatives clipped, 2 x 2 block mean - float64.  The oracle's float32 form per sub-pixel: 4 a (exact), four subtractions
    whose intermediates are bounded by S = 6 |a| + |p| + |q| (p, q the two outer neighbours) -> error <= 4 u S; clipping at 0
    does not grow it; three additions of the four sub-pixels (each sum bounded by the sum of the four S) -> 3 u sum(S); the
    multiplication by 0.25 is exact.  Total <= 0.25 * 7 u * sum(S), sum(S) = 24 |a| + 2 (|up| + |down| + |left| + |right|):
    7 float32 ulps of 4 |a| on a smooth image.  1 % is added for the second-order terms."""
    rng = np.random.default_rng(630)
    lap = np.array([[0, -1, 0], [-1, 4, -1], [0, -1, 0]], np.float64)
    for a in _images(rng):
        H, W = a.shape
        out = L.laplace_rebin(a)
        sub = np.repeat(np.repeat(a.astype(np.float64), 2, axis=0), 2, axis=1)
        conv = np.maximum(ndimage.correlate(sub, lap, mode='constant', cval=0.0), 0.0)
        ref = conv.reshape(H, 2, W, 2).sum(axis=(1, 3)) * 0.25
        absa = np.abs(a).astype(np.float64)
        nb = np.zeros_like(absa)
        nb[1:] += absa[:-1]; nb[:-1] += absa[1:]; nb[:, 1:] += absa[:, :-1]; nb[:, :-1] += absa[:, 1:]
        bound = 1.01 * 0.25 * 7 * U * (24 * absa + 2 * nb)
        assert out.dtype == np.float32 and out.shape == a.shape
        err = np.abs(out.astype(np.float64) - ref)
        assert np.all(err <= bound), (a.shape, float((err / np.maximum(bound, 1e-300)).max()))
        border = np.ones(a.shape, bool)
        border[1:-1, 1:-1] = False
        assert np.all(err[border] <= bound[border])
