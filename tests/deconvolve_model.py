"""F12 in NumPy: the damped Richardson-Lucy stage of csrc/deconvolve.hip restated operation by operation (include/apgpu.h
F12).  The reference has no such stage: this file is the definition the kernels are held to, bit for bit, and
tests/test_deconvolve_model_host.py holds it to synthetic truth.  No torch, no GPU.

Inputs.  d [H][W] float32; a non-finite value means "no data"; valid(y, x) = inside the image and finite.  p [K][K] float32,
  K = 2 R + 1, 0 <= R <= 12; every weight finite and >= 0, the sum > 0; the weights are used as given.  Sky level b >= 0; gain > 0
  (e-/ADU); read noise rn >= 0 (ADU); damping threshold T >= 0; niter >= 0; min_weight (0.1).
Rounding and order.  Every operation is float32 and every multiply and add rounds on its own.  Accumulators start at +0.  The 2-D tap
  order is row-major: j (PSF row) ascending outside, i ascending inside.  min(x, 1) means x where x < 1, else 1, and max(x, 0)
  means x where x > 0, else 0 (a NaN gives the constant).
1 Norm plane (once): n(y, x) = sum_{j,i} p[j][i] W(y + j - R, x + i - R), W = 1 where valid and 0 elsewhere, outside the image
  included.  inv(y, x) = 1 / n where n >= min_weight, else 0.
2 Start: u(y, x) = start everywhere (a positive float32), or the caller's plane.
3 Forward + ratio, per iteration: c = (sum_{j,i} p[j][i] u(clampy(y + R - j), clampx(x + R - i))) + b: a true convolution (the PSF
  flipped), u edge-replicated outside the image.  At an invalid pixel r = 0.  At a valid pixel with !(c > 0), r = 1.  Otherwise,
  with T == 0: r = d / c.  Otherwise, with T > 0: e = d - c; var = max(c, 0) / gain + rn rn; U = min((e e) / ((T T) var), 1);
  U2 = U U; U4 = U2 U2; U8 = U4 U4; U9 = U8 U; w = U9 (10 - 9 U); r = 1 + (w e) / c.  In both cases r = max(r, 0).
4 Back-projection + update: q = sum_{j,i} p[j][i] r(y + j - R, x + i - R), a correlation; taps outside the image are +0.
  u' = (u q) inv where inv != 0, else u' = u.
5 Output: out = u + b at the valid pixels, NaN at the others.
"""
import math

import numpy as np

F = np.float32
MAX_RADIUS = 12
FWHM_TO_SIGMA = 0.42466090014400953                                  # 1 / (2 sqrt(2 ln 2))
NAN32 = np.array([0x7fc00000], np.uint32).view(F)[0]


# ---- the PSF stamps ----------------------------------------------------------------------------------------------------------
def _stamp(profile, fwhm, radius, default_radius):
    fwhm = float(fwhm)
    if not (fwhm > 0.0 and math.isfinite(fwhm)):
        raise ValueError('the FWHM must be finite and > 0, got %r' % fwhm)
    R = int(default_radius if radius is None else radius)
    if R < 0 or R > MAX_RADIUS:
        raise ValueError('a PSF of FWHM %g pixels needs a radius of %d, the kernels hold %d: bin the image' % (fwhm, R, MAX_RADIUS))
    k = np.arange(2 * R + 1, dtype=np.float64) - R
    sub = (np.arange(5, dtype=np.float64) + 0.5) / 5.0 - 0.5             # 5 x 5 midpoints inside the pixel
    g = np.zeros((2 * R + 1, 2 * R + 1), np.float64)
    for dy in sub:
        for dx in sub:
            g += profile((k[:, None] + dy) ** 2 + (k[None, :] + dx) ** 2)
    return (g / g.sum()).astype(F)


def psf_gaussian(fwhm, radius=None):
    """[K][K] float32: a round Gaussian, pixel-integrated by 5 x 5 midpoint sub-sampling in float64, normalised to sum 1, then cast.
    Default radius ceil(1.7 FWHM)."""
    s = float(fwhm) * FWHM_TO_SIGMA
    return _stamp(lambda r2: np.exp(-r2 / (2.0 * s * s)), fwhm, radius, math.ceil(1.7 * float(fwhm)))


def psf_moffat(fwhm, beta=2.5, radius=None):
    """The same for a Moffat profile (1 + r^2 / alpha^2)^-beta, alpha = FWHM / (2 sqrt(2^(1/beta) - 1)).  Default radius ceil(2.5 FWHM)."""
    beta = float(beta)
    if not (beta > 1.0 and math.isfinite(beta)):
        raise ValueError('the Moffat beta must be finite and > 1, got %r' % beta)
    alpha = float(fwhm) / (2.0 * math.sqrt(2.0 ** (1.0 / beta) - 1.0))
    return _stamp(lambda r2: (1.0 + r2 / (alpha * alpha)) ** -beta, fwhm, radius, math.ceil(2.5 * float(fwhm)))


def check_stamp(psf):
    """The stamp as a contiguous float32 [K][K] array and its radius; ValueError for a shape that is not odd and square, a radius
    above 12, a negative or non-finite weight or a sum <= 0."""
    p = np.ascontiguousarray(psf, dtype=F)
    if p.ndim != 2 or p.shape[0] != p.shape[1] or p.shape[0] % 2 != 1:
        raise ValueError('the PSF stamp must be square with an odd side, got shape %s' % (p.shape,))
    R = p.shape[0] // 2
    if R > MAX_RADIUS:
        raise ValueError('a PSF stamp of radius %d, the kernels hold %d: bin the image' % (R, MAX_RADIUS))
    if not np.all(np.isfinite(p)) or np.any(p < 0) or not p.astype(np.float64).sum() > 0:
        raise ValueError('the PSF weights must be finite and >= 0 with a sum > 0')
    return p, R


# ---- the three steps -----------------------------------------------------------------------------------------------------------
def _taps(plane, p, flip, mode):
    """sum_{j,i} p[j][i] plane(.), row-major, float32, from +0.  flip: the convolution, plane(y + R - j, x + R - i); else the
    correlation, plane(y + j - R, x + i - R).  mode: 'edge' (replicated) or 'constant' (+0 outside)."""
    H, W = plane.shape
    K = p.shape[0]
    R = K // 2
    pad = np.pad(plane.astype(F), R, mode=mode)
    acc = np.zeros((H, W), F)
    for j in range(K):
        for i in range(K):
            sl = pad[2 * R - j:2 * R - j + H, 2 * R - i:2 * R - i + W] if flip else pad[j:j + H, i:i + W]
            acc = acc + F(p[j, i]) * sl
    return acc


def forward(u, p):
    """The forward sum of step 3 without the sky: the model of the blur itself (u convolved with the PSF, edges replicated)."""
    p, _ = check_stamp(p)
    return _taps(np.asarray(u, F), p, True, 'edge')


def norm(d, p, min_weight=0.1):
    p, _ = check_stamp(p)
    n = _taps(np.isfinite(d).astype(F), p, False, 'constant')
    ok = n >= F(min_weight)
    with np.errstate(divide='ignore'):
        return np.where(ok, F(1) / np.where(ok, n, F(1)), F(0)).astype(F)


def ratio(u, d, p, sky, gain=1.0, readnoise=0.0, damp=0.0):
    d = np.asarray(d, F)
    b, gain, rn, T = F(sky), F(gain), F(readnoise), F(damp)
    valid = np.isfinite(d)
    dz = np.where(valid, d, F(0)).astype(F)
    with np.errstate(all='ignore'):
        c = forward(u, p) + b
        pos = c > 0
        if T == 0:
            r = dz / c
        else:
            e = dz - c
            var = np.where(pos, c, F(0)) / gain + rn * rn
            t = (e * e) / ((T * T) * var)
            U = np.where(t < 1, t, F(1)).astype(F)
            U2 = U * U
            U4 = U2 * U2
            U8 = U4 * U4
            U9 = U8 * U
            w = U9 * (F(10) - F(9) * U)
            r = F(1) + (w * e) / c
        r = np.where(r > 0, r, F(0)).astype(F)
    r = np.where(pos, r, F(1))
    return np.where(valid, r, F(0)).astype(F)


def back(r, p):
    p, _ = check_stamp(p)
    return _taps(np.asarray(r, F), p, False, 'constant')


def update(u, r, inv, p):
    u = np.asarray(u, F)
    with np.errstate(all='ignore'):
        return np.where(inv != 0, (u * back(r, p)) * inv, u).astype(F)


def start_level(d, sky):
    """The default start: the float64 mean of d - b over the valid pixels, at least 1e-6, as a float32."""
    d = np.asarray(d, F)
    v = np.isfinite(d)
    m = float((d[v].astype(np.float64) - float(F(sky))).mean()) if v.any() else 0.0
    return F(max(m, 1e-6))


def richardson_lucy(d, p, sky, niter=30, damp=0.0, gain=1.0, readnoise=0.0, start=None, min_weight=0.1):
    """(out, u): the output of step 5 and the estimate without the sky.  start: a float32 scalar, a plane, or None (start_level)."""
    d = np.asarray(d, F)
    inv = norm(d, p, min_weight)
    if start is None:
        start = start_level(d, sky)
    u = np.full(d.shape, F(start), F) if np.ndim(start) == 0 else np.array(start, F)
    for _ in range(int(niter)):
        u = update(u, ratio(u, d, p, sky, gain, readnoise, damp), inv, p)
    with np.errstate(all='ignore'):
        return np.where(np.isfinite(d), u + F(sky), NAN32).astype(F), u


# ---- the synthetic scene of the tests --------------------------------------------------------------------------------------
SCENE_SEED = 1
SCENE_FWHM, SCENE_SKY, SCENE_RADIUS = 3.5, 100.0, 6
SCENE_STARS = ((30.3, 40.6, 4e4), (60.7, 100.2, 8e4), (20.5, 120.4, 2e4), (70.2, 30.8, 3e4), (48.0, 75.5, 6e4))    # y, x, total flux


def scene(faint=1.0, stars=True, seed=SCENE_SEED):
    """96 x 160: five Gaussian stars of FWHM 3.5 with a total flux of 2e4 .. 8e4 (times `faint`) on a sky of 100, Poisson noise
    (numpy default_rng(seed)).  Returns dict(d, truth, stars, sky, fwhm, psf)."""
    rng = np.random.default_rng(seed)
    H, W = 96, 160
    s = SCENE_FWHM * FWHM_TO_SIGMA
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    truth = np.zeros((H, W))
    if stars:
        for y, x, fl in SCENE_STARS:
            truth += faint * fl * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * s * s)) / (2 * math.pi * s * s)
    d = rng.poisson(truth + SCENE_SKY).astype(F)
    return dict(d=d, truth=truth, stars=SCENE_STARS, sky=SCENE_SKY, fwhm=SCENE_FWHM, psf=psf_gaussian(SCENE_FWHM, SCENE_RADIUS))


def moment_fwhm(img, x, y, bg, half=7):
    """(FWHM, flux) of a star from the second moments of the (2 half + 1)^2 box about its own centroid, the background removed."""
    yi, xi = int(round(y)), int(round(x))
    s = img[yi - half:yi + half + 1, xi - half:xi + half + 1].astype(np.float64) - bg
    yy, xx = np.mgrid[-half:half + 1, -half:half + 1]
    f = s.sum()
    cx, cy = (s * xx).sum() / f, (s * yy).sum() / f
    v = ((s * ((xx - cx) ** 2 + (yy - cy) ** 2)).sum() / f) / 2.0
    return math.sqrt(max(v, 0.0)) / FWHM_TO_SIGMA, f
