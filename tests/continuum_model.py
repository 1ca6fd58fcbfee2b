"""NumPy restatement of F11, narrow-band continuum subtraction (include/apgpu.h "F11"): the taps, the normalised
blur, the PSF-matching rule, the six moments, the clipped straight-line fit and its truncation correction, the stars rule and the
combine.  No torch, no GPU.  PARITY UNPINNED: the reference lists the stage as not yet built, so these definitions are the
project's own and tests/test_continuum_model_host.py holds them to synthetic truth; the kernels are then held to this file.

Every float64 expression below rounds after each operation, in the order written (NumPy never contracts)."""
import math

import numpy as np

F = np.float32
MAX_RADIUS = 32
FWHM_TO_SIGMA = 1.0 / (2.0 * math.sqrt(2.0 * math.log(2.0)))


# ---- taps and blur ---------------------------------------------------------------------------------------------------------
def gauss_taps(sigma, radius=None):
    """float64 taps w[0 .. 2R] = exp(-(k - R)^2 / (2 sigma^2)) normalised to sum 1; R = ceil(4 sigma), at least 1.  sigma = 0 (or
    radius = 0): the identity {1}.  R > 32 raises ValueError."""
    sigma = float(sigma)
    if not sigma >= 0.0 or not math.isfinite(sigma):
        raise ValueError('sigma must be finite and >= 0, got %r' % sigma)
    if radius is None:
        radius = 0 if sigma == 0.0 else max(1, int(math.ceil(4.0 * sigma)))
    radius = int(radius)
    if radius < 0 or radius > MAX_RADIUS:
        raise ValueError('a blur of sigma = %g pixels needs a radius of %d, the kernel holds %d' % (sigma, radius, MAX_RADIUS))
    if radius == 0 or sigma == 0.0:
        w = np.zeros(2 * radius + 1)
        w[radius] = 1.0
        return w
    k = np.arange(2 * radius + 1, dtype=np.float64) - radius
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum()


def _pass(v, ok, w, axis):
    """sum_k w[k] v(. + k - R) over the taps with ok, k ascending, accumulators from +0; v float64 [H, W]."""
    R = (len(w) - 1) // 2
    n = v.shape[axis]
    acc = np.zeros(v.shape, np.float64)
    for k in range(2 * R + 1):
        d = k - R                                           # out[i] takes v[i + d]
        lo, hi = max(0, -d), min(n, n - d)
        if hi <= lo:
            continue
        dst = [slice(None)] * 2
        src = [slice(None)] * 2
        dst[axis], src[axis] = slice(lo, hi), slice(lo + d, hi + d)
        dst, src = tuple(dst), tuple(src)
        with np.errstate(all='ignore'):
            t = w[k] * v[src]
            acc[dst] = np.where(ok[src], acc[dst] + t, acc[dst])
    return acc


def gauss_blur(data, taps, min_weight=0.5):
    """The normalised separable blur of a float32 image with NaN / inf holes -> float32."""
    data = np.asarray(data, F)
    w = np.asarray(taps, np.float64)
    ok = np.isfinite(data)
    v = np.where(ok, data, F(0)).astype(np.float64)
    one = np.ones(data.shape, np.float64)
    a = _pass(v, ok, w, 1)
    m = _pass(one, ok, w, 1)
    inside = np.ones(data.shape, bool)
    A = _pass(a, inside, w, 0)
    M = _pass(m, inside, w, 0)
    keep = ok & (M >= float(min_weight))
    with np.errstate(all='ignore'):
        q = (A / M).astype(F)
    return np.where(keep, q, F(np.nan)).astype(F)


def psf_match_plan(fwhm_n, fwhm_c, threshold=0.05):
    """Which image is blurred: ('narrow' | 'continuum' | None, sigma_k, taps or None)."""
    fwhm_n, fwhm_c = float(fwhm_n), float(fwhm_c)
    if not (fwhm_n > 0 and fwhm_c > 0 and math.isfinite(fwhm_n) and math.isfinite(fwhm_c)):
        raise ValueError('the FWHMs must be positive and finite, got %r and %r' % (fwhm_n, fwhm_c))
    if abs(fwhm_n - fwhm_c) < float(threshold):
        return None, 0.0, None
    sn, sc = fwhm_n * FWHM_TO_SIGMA, fwhm_c * FWHM_TO_SIGMA
    broad, sharp = max(sn, sc), min(sn, sc)
    sigma_k = math.sqrt(broad * broad - sharp * sharp)
    try:
        taps = gauss_taps(sigma_k)
    except ValueError as exc:
        raise ValueError('PSF matching FWHM %g to %g: %s' % (fwhm_n, fwhm_c, exc)) from None
    return ('narrow' if sn < sc else 'continuum'), sigma_k, taps


def psf_match(n, c, fwhm_n, fwhm_c, threshold=0.05, min_weight=0.5):
    which, sigma_k, taps = psf_match_plan(fwhm_n, fwhm_c, threshold)
    n, c = np.asarray(n, F), np.asarray(c, F)
    if which == 'narrow':
        n = gauss_blur(n, taps, min_weight)
    elif which == 'continuum':
        c = gauss_blur(c, taps, min_weight)
    return n, c, dict(blurred=which, sigma_k=sigma_k, taps=taps)


# ---- moments and the straight-line fit ----------------------------------------------------------------------------------------
def pair_moments(n, c, s=0.0, b=0.0, lo=-np.inf, hi=np.inf, mask=None):
    """float64 [6] = count, sum c, sum n, sum cc, sum cn, sum nn over the pairs finite in both, unmasked, lo <= r <= hi."""
    n, c = np.asarray(n, F).ravel(), np.asarray(c, F).ravel()
    ok = np.isfinite(n) & np.isfinite(c)
    if mask is not None:
        ok &= np.asarray(mask).ravel() == 0
    y, x = n[ok].astype(np.float64), c[ok].astype(np.float64)
    with np.errstate(all='ignore'):
        r = y - (np.float64(s) * x + np.float64(b))
        keep = (r >= lo) & (r <= hi)
    y, x = y[keep], x[keep]
    return np.array([float(y.size), x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum()], np.float64)


def moment_terms_abs(n, c, s=0.0, b=0.0, lo=-np.inf, hi=np.inf, mask=None):
    """The sums of |terms| behind the worst-case bound of two summation orders: [6] like pair_moments."""
    n, c = np.asarray(n, F).ravel(), np.asarray(c, F).ravel()
    ok = np.isfinite(n) & np.isfinite(c)
    if mask is not None:
        ok &= np.asarray(mask).ravel() == 0
    y, x = n[ok].astype(np.float64), c[ok].astype(np.float64)
    with np.errstate(all='ignore'):
        r = y - (np.float64(s) * x + np.float64(b))
        keep = (r >= lo) & (r <= hi)
    y, x = y[keep], x[keep]
    return np.array([float(y.size), np.abs(x).sum(), np.abs(y).sum(), (x * x).sum(), np.abs(x * y).sum(), (y * y).sum()], np.float64)


def line_from_moments(mom, fixed_scale=None):
    """Centred solution of n = s c + b: dict(s, b, sigma (rms residual), n, se_s, se_b, cbar, scc)."""
    cnt, sc, sy, scc, scy, syy = (float(v) for v in mom)
    if cnt < 3:
        raise RuntimeError('continuum fit: %d valid pixel pairs survive, at least 3 are needed' % int(cnt))
    cbar, ybar = sc / cnt, sy / cnt
    Scc, Scy, Syy = scc - sc * cbar, scy - sc * ybar, syy - sy * ybar
    if fixed_scale is None:
        if not Scc > 0.0:
            raise RuntimeError('continuum fit: the continuum image has zero variance over the valid pixels')
        s = Scy / Scc
        rss = Syy - s * Scy
        dof = cnt - 2.0
    else:
        s = float(fixed_scale)
        rss = (Syy - 2.0 * s * Scy) + s * s * Scc
        dof = cnt - 1.0
    rss = max(rss, 0.0)
    b = ybar - s * cbar
    var = rss / dof
    se_s = math.sqrt(var / Scc) if (fixed_scale is None) else 0.0
    se_b = math.sqrt(var * (1.0 / cnt + cbar * cbar / Scc)) if fixed_scale is None else math.sqrt(var / cnt)
    return dict(s=s, b=b, sigma=math.sqrt(rss / cnt), n=int(cnt), se_s=se_s, se_b=se_b, cbar=cbar, scc=Scc)


def _phi(x):
    return math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi) if math.isfinite(x) else 0.0


def _Phi(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def truncation_shift(kappa_lo, kappa_hi):
    """Mean of a unit Gaussian truncated to [-kappa_lo, kappa_hi]: (phi(-kl) - phi(kh)) / (Phi(kh) - Phi(-kl)); -0.0508 for (3, 2)."""
    return (_phi(-kappa_lo) - _phi(kappa_hi)) / (_Phi(kappa_hi) - _Phi(-kappa_lo))


def truncated_moments(alpha, beta):
    """(mean, variance) of a unit Gaussian truncated to [alpha, beta]."""
    Z = _Phi(beta) - _Phi(alpha)
    pa, pb = _phi(alpha), _phi(beta)
    mean = (pa - pb) / Z
    ta = alpha * pa if math.isfinite(alpha) else 0.0
    tb = beta * pb if math.isfinite(beta) else 0.0
    return mean, 1.0 + (ta - tb) / Z - mean * mean


def gaussian_truncation(lo, hi, mean_kept, sigma_kept):
    """The Gaussian N(mu, sigma0^2) whose part inside [lo, hi] has the mean mean_kept and the standard deviation sigma_kept (all in
    one coordinate: residuals about the line the bounds were set on).  With a = (lo - mu) / sigma0, b = (hi - mu) / sigma0 and the
    truncated unit Gaussian's mean m(a, b) = (phi(a) - phi(b)) / (Phi(b) - Phi(a)) and variance V(a, b):
        mean_kept = mu + sigma0 m(a, b),    sigma_kept^2 = sigma0^2 V(a, b)
    solved by fixed-point rounds from (mean_kept, sigma_kept), 200 at most.  Returns (mu, sigma0).  For bounds at -3 sigma0 and
    +2 sigma0 about mu the shift mean_kept - mu is the closed form -0.0508 sigma0."""
    if not (math.isfinite(lo) or math.isfinite(hi)) or not sigma_kept > 0.0:
        return mean_kept, sigma_kept
    mu, s0 = mean_kept, sigma_kept
    for _ in range(200):
        m, var = truncated_moments((lo - mu) / s0, (hi - mu) / s0)
        ns0 = sigma_kept / math.sqrt(var)
        nmu = mean_kept - ns0 * m
        done = abs(ns0 - s0) <= 1e-13 * s0 and abs(nmu - mu) <= 1e-13 * s0
        mu, s0 = nmu, ns0
        if done:
            break
    return mu, s0


def continuum_scale_pixels(n, c, mask=None, sigma_lower=3.0, sigma_upper=2.0, maxiters=10, fixed_scale=None, moments=pair_moments):
    """The iteratively clipped fit.  Returns dict(s, b (corrected), b_uncorrected, sigma, sigma0, shift, n, iterations, se_s, se_b,
    lo, hi, n_unclipped, unclipped (the first fit))."""
    lo, hi = -np.inf, np.inf
    fit = line_from_moments(moments(n, c, 0.0, 0.0, lo, hi, mask), fixed_scale)
    first = dict(fit)
    prev_b = fit['b']
    count, iters = fit['n'], 0
    for _ in range(int(maxiters)):
        nlo, nhi = -float(sigma_lower) * fit['sigma'], float(sigma_upper) * fit['sigma']
        mom = moments(n, c, fit['s'], fit['b'], nlo, nhi, mask)
        if int(mom[0]) == count:
            break
        prev_b = fit['b']
        fit = line_from_moments(mom, fixed_scale)
        lo, hi, count = nlo, nhi, fit['n']
        iters += 1
    # residuals about the line the last bounds were set on: the kept ones have the mean b - prev_b and the rms sigma
    mu, sigma0 = gaussian_truncation(lo, hi, fit['b'] - prev_b, fit['sigma'])
    out = dict(fit)
    out.update(b=prev_b + mu, b_uncorrected=fit['b'], sigma0=sigma0, shift=fit['b'] - (prev_b + mu), iterations=iters, lo=lo, hi=hi,
               n_unclipped=first['n'], unclipped=first)
    return out


# ---- the stars rule -------------------------------------------------------------------------------------------------------------
def clipped_median(x, sigma=3.0, maxiters=5):
    """(median, std, n) of the float64 sample after clipping at median +- sigma std, at most maxiters rounds."""
    x = np.asarray(x, np.float64).ravel()
    x = x[np.isfinite(x)]
    for _ in range(int(maxiters)):
        if x.size == 0:
            break
        med, sd = np.median(x), np.std(x)
        y = x[(x >= med - sigma * sd) & (x <= med + sigma * sd)]
        if y.size == x.size:
            break
        x = y
    if x.size == 0:
        return float('nan'), float('nan'), 0
    return float(np.median(x)), float(np.std(x)), int(x.size)


def scale_from_fluxes(flux_n, flux_c, peak=None, satlevel=None, min_stars=5):
    """s = clipped median of F_N / F_C over the stars with both fluxes positive and finite and peak < satlevel.
    Returns dict(s, spread, n, n_used, se_s, keep)."""
    fn, fc = np.asarray(flux_n, np.float64), np.asarray(flux_c, np.float64)
    keep = np.isfinite(fn) & np.isfinite(fc) & (fn > 0) & (fc > 0)
    if peak is not None and satlevel is not None:
        keep &= np.asarray(peak, np.float64) < float(satlevel)
    if int(keep.sum()) < int(min_stars):
        raise RuntimeError('continuum scale from stars: %d usable stars, at least %d are needed' % (int(keep.sum()), int(min_stars)))
    s, spread, used = clipped_median(fn[keep] / fc[keep])
    return dict(s=s, spread=spread, n=int(keep.sum()), n_used=used, se_s=spread / math.sqrt(max(used, 1)), keep=keep)


def star_residual_frac(flux_l, flux_n):
    """median |aperture flux in L| / aperture flux in N' over the stars with a positive finite N' flux."""
    fl, fn = np.asarray(flux_l, np.float64), np.asarray(flux_n, np.float64)
    ok = np.isfinite(fl) & np.isfinite(fn) & (fn > 0)
    return float(np.median(np.abs(fl[ok]) / fn[ok])) if ok.any() else float('nan')


# ---- the subtraction -----------------------------------------------------------------------------------------------------------
def linear_combine(x, y, ca, cb, c0):
    """(float32(ca x) + float32(cb y)) + c0 in float32, NaN where x or y is not finite; y None: float32(ca x) + c0."""
    x = np.asarray(x, F)
    ok = np.isfinite(x)
    with np.errstate(all='ignore'):
        v = F(ca) * x
        if y is not None:
            y = np.asarray(y, F)
            ok = ok & np.isfinite(y)
            v = v + F(cb) * y
        v = v + F(c0)
    return np.where(ok, v, F(np.nan)).astype(F)


def subtract(n_matched, c_matched, s, b):
    """L = N' - s C' - b with the kernel's roundings: ca = 1, cb = float32(-s), c0 = float32(-b)."""
    return linear_combine(n_matched, c_matched, 1.0, -float(s), -float(b))


# ---- the synthetic scene of the tests ----------------------------------------------------------------------------------------------
def scene(shape=(256, 384), n_stars=150, fwhm_n=3.4, fwhm_c=2.6, s=0.083, b=0.4, sky_c=30.0, noise_n=0.5, noise_c=0.3, seed=11,
          emission_peak=25.0):
    """A continuum image C (sky, stars of fwhm_c, noise) and a narrow-band image N = s (sky + stars of fwhm_n) + b + emission +
    noise, the emission a smooth region over about 15 % of the pixels.  The defaults are the scene of the tests: the continuum image
    is the sharper and the deeper one (a broad-band co-add), so it is the one that is blurred and the residual noise stays white,
    which is what the formal errors of the fit assume.  Returns dict(n, c, xy [n_stars, 2] (x, y), flux_c,
    emission, s, b, fwhm_n, fwhm_c)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    margin = 16
    xs = rng.uniform(margin, W - margin, n_stars)
    ys = rng.uniform(margin, H - margin, n_stars)
    flux = 10.0 ** rng.uniform(3.0, 4.6, n_stars)                     # total counts in C

    def stars(fwhm):
        sg = fwhm * FWHM_TO_SIGMA
        img = np.zeros(shape)
        r = int(math.ceil(6 * sg))
        for x0, y0, f in zip(xs, ys, flux):
            i0, i1 = max(0, int(y0) - r), min(H, int(y0) + r + 1)
            j0, j1 = max(0, int(x0) - r), min(W, int(x0) + r + 1)
            d2 = (xx[i0:i1, j0:j1] - x0) ** 2 + (yy[i0:i1, j0:j1] - y0) ** 2
            img[i0:i1, j0:j1] += f / (2.0 * math.pi * sg * sg) * np.exp(-d2 / (2.0 * sg * sg))
        return img

    # emission: an ellipse with a soft edge (tanh over about three pixels), structured inside, about 15 % of the area
    ey, ex, ay, ax = 0.55 * H, 0.6 * W, 0.2 * H, 0.25 * W
    rad = np.sqrt(((yy - ey) / ay) ** 2 + ((xx - ex) / ax) ** 2)
    edge = 0.5 * (1.0 - np.tanh((rad - 0.97) * min(ay, ax) / 1.5))
    emission = emission_peak * edge * (0.6 + 0.4 * np.cos(xx / 23.0) * np.sin(yy / 17.0) ** 2)
    c_img = sky_c + stars(fwhm_c) + rng.normal(0.0, noise_c, shape)
    n_img = s * (sky_c + stars(fwhm_n)) + b + emission + rng.normal(0.0, noise_n, shape)
    return dict(n=n_img.astype(F), c=c_img.astype(F), xy=np.stack([xs, ys], 1), flux_c=flux, emission=emission, s=s, b=b,
                fwhm_n=fwhm_n, fwhm_c=fwhm_c)
