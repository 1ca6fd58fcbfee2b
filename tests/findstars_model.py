"""CPU model of the star finder (F6): NumPy float64, every rule the HIP kernels of csrc/findstars.hip follow.

PARITY UNPINNED (photutils absent): DAOStarFinder, find_peaks and aperture_photometry are restated from the published
DAOFIND algorithm (Stetson 1987, PASP 99, 191) in the form photutils gives it; only the annulus statistic is pinned to
astropy itself (golden group G16).  This file is the yardstick of tests/test_gpu_findstars.py.

Conventions: images are [H][W] row-major, pixel (i, j) = (row, column) = (y, x) and covers [j-0.5, j+0.5] x [i-0.5, i+0.5].

Rules
-----
daofind_kernel   sigma = fwhm / (2 sqrt(2 ln 2)); R = max(2, int(1.5 sigma)); g = exp(-(x^2 + y^2) / (2 sigma^2)) on the
                 (2R+1)^2 grid; footprint fp = (g >= exp(-1.5^2 / 2)) | (x^2 + y^2 <= 4); npixels = sum(fp);
                 K = ((g fp - sum(g fp) / npixels) / denom) fp with denom = sum((g fp)^2) - sum(g fp)^2 / npixels;
                 relerr = 1 / sqrt(denom); the detection threshold on the convolved image is threshold * relerr.
convolve         True convolution out[i, j] = sum_{a, b} K[a, b] * d[i + R - a, j + R - b] (kernel flipped; K is symmetric
                 here, so the flip changes no value, only the order of the terms), d = 0 outside the image.  Every one of
                 the (2R+1)^2 taps takes part - also those whose weight is 0 and those outside the image - in row-major
                 (a, b) order: acc = acc + float64(d) * K[a, b] with a separately rounded multiply and add, acc starts
                 at +0.0; the result is acc rounded once to float32.  d = data - float32(bg_median) is one float32
                 subtraction made before the convolution (in-image pixels only).
find_peaks       Pixel p is a peak when no pixel under the footprint centred on p (centre index = size // 2 per axis,
                 scipy's convention; no flip) holds a value > v[p], where a footprint tap outside the image holds 0, AND
                 float64(v[p]) > threshold (strict), AND mask[p] == 0, AND border <= i < H - border, border <= j < W - border
                 (border = R for DAOFIND: the (2R+1)^2 cut-out lies wholly inside the image; 0 for the saturation search).
                 Equal neighbouring maxima are all peaks.  A NaN is never a peak and never suppresses one.  Peaks are
                 ordered by flat index i * W + j.  The mask only excludes peaks: the convolution sees the unmodified image.
daofind_measure  For a peak at (i, j) with cut-outs D (of d) and C (of the convolved image), both (2R+1)^2:
                   npix       = (2R+1)^2 (the size of the kernel array)
                   peak       = D[R, R]; conv_peak = C[R, R]
                   sharpness  = (peak - (sum(D fp) - peak) / (npixels - 1)) / conv_peak
                   roundness1 = 2 sum2 / sum4; with C' = C but C'[R, R] = 0: sum4 = sum |C'|, sum2 = sum Q C' where
                                Q = -1 for (row <= R, col > R), +1 for (row < R, col <= R), -1 for (row >= R, col < R),
                                +1 for (row > R, col >= R), 0 at the centre; sum2 == 0 gives 0, otherwise sum4 <= 0 gives NaN
                   marginal fits (DAOFIND's triangular weights w[k] = R - |k - R| + 1, p = sum(w), G = the unmasked g):
                     x: sg[j] = sum_i G[i, j] w[i]; dg[j] = sg[j] (R - j); sumg = sum w sg; sumgsq = sum w sg^2;
                        sdgd = sum w dg; sdgds = sum w dg^2; sgdgd = sum w sg dg;
                        sumd = sum_ij D w[i] w[j]; sumgd = sum_ij D w[i] w[j] sg[j]; sddgd = sum_ij D w[i] w[j] dg[j]
                        hx = (sumgd - sumg sumd / p) / (sumgsq - sumg^2 / p)
                        dx = (sgdgd - (sddgd - sdgd sumd)) / (hx sdgds / sigma^2)
                     y: the same with rows and columns exchanged (sg[i] = sum_j G[i, j] w[j], dg[i] = sg[i] (R - i)) -> hy, dy
                   xcentroid = j + dx; ycentroid = i + dy; roundness2 = 2 (hx - hy) / (hx + hy)
                   flux = conv_peak / threshold_eff; mag = -2.5 log10(flux)
                 The per-tap weights (w[i] w[j], w[i] w[j] sg[j], ...) are formed once in float64 (measure_tables) and each
                 sum over the cut-out is sum(float64(value) * weight); the kernel may add the products in any order.
                 A candidate is REJECTED (keep = 0) when any of these holds:
                   1. hx or hy is not > 0 (a non-positive or NaN amplitude);
                   2. sharpness is not strictly inside (sharplo, sharphi), or roundness1 or roundness2 is not strictly
                      inside (roundlo, roundhi);
                   3. |dx| > R or |dy| > R (a centroid shift larger than the kernel radius);
                   4. xcentroid, ycentroid, sharpness, roundness1, roundness2, peak or flux is not finite.
circle_overlap   exact area of circle ∩ pixel square: area = I(y1) - I(y0), I(y) = integral over [max(x0, -r), min(x1, r)]
                 of clamp(y, -h(x), h(x)) dx, h = sqrt(r^2 - x^2); the arc pieces are a trapezoid under the chord plus the
                 circular segment r^2 / 2 (t - sin t), t = 2 asin(chord / 2r).  A pixel whose farthest corner is inside
                 the circle has area exactly 1, one whose nearest point is outside exactly 0.
aperture_photometry  r = ceil(2 fwhm), annulus r .. ceil(1.5 r).  A pixel belongs to the annulus when its centre has
                 r_in^2 <= d2 <= r_out^2 (both sides inclusive), d2 = dx * dx + dy * dy in float64, and lies in the image
                 (pixels outside the image are not part of the annulus).  The values, in row-major order, go through the
                 float32 noaxis clip (annulus_clip); bkg_median is its median.  aperture_sum_raw = sum overlap * data in
                 float64, row-major over the pixels with overlap > 0; aperture_sum = raw - float64(bkg_median) * pi r^2.
"""
import math

import numpy as np

NQ = 6                  # weight planes of the data cut-out, in this order:
Q_FP, Q_SUMD, Q_SUMGD_X, Q_SDDGD_X, Q_SUMGD_Y, Q_SDDGD_Y = range(NQ)
SHARPLO, SHARPHI, ROUNDLO, ROUNDHI = 0.2, 1.0, -1.0, 1.0     # photutils' defaults
REC = ('x_peak', 'y_peak', 'npix', 'peak', 'conv_peak', 'sharpness', 'roundness1', 'roundness2', 'dx', 'dy', 'hx', 'hy',
       'xcentroid', 'ycentroid', 'flux', 'mag')


def daofind_kernel(fwhm):
    """dict(sigma, R, g, fp (bool), npixels, K, relerr, w, consts (per axis), tables [NQ, (2R+1)^2], quad)."""
    sigma = fwhm / (2.0 * math.sqrt(2.0 * math.log(2.0)))
    R = max(2, int(1.5 * sigma))
    ax = np.arange(-R, R + 1, dtype=np.float64)
    r2 = ax[:, None] ** 2 + ax[None, :] ** 2
    g = np.exp(-r2 / (2.0 * sigma * sigma))
    fp = (g >= math.exp(-1.5 * 1.5 / 2.0)) | (r2 <= 4.0)
    npixels = int(fp.sum())
    gm = g * fp
    s1 = float(gm.sum())
    denom = float((gm * gm).sum()) - s1 * s1 / npixels
    K = ((gm - s1 / npixels) / denom) * fp
    relerr = 1.0 / math.sqrt(denom)
    n = 2 * R + 1
    w = R - np.abs(np.arange(n, dtype=np.float64) - R) + 1.0
    p = float(w.sum())
    vec = R - np.arange(n, dtype=np.float64)
    consts = {}
    tables = np.zeros((NQ, n, n), np.float64)
    tables[Q_FP] = fp
    ww = w[:, None] * w[None, :]
    tables[Q_SUMD] = ww
    for axis, (qg, qd) in (('x', (Q_SUMGD_X, Q_SDDGD_X)), ('y', (Q_SUMGD_Y, Q_SDDGD_Y))):
        sg = (g * w[:, None]).sum(axis=0) if axis == 'x' else (g * w[None, :]).sum(axis=1)
        dg = sg * vec
        consts[axis] = dict(sumg=float((w * sg).sum()), sumgsq=float((w * sg * sg).sum()), sdgd=float((w * dg).sum()),
                            sdgds=float((w * dg * dg).sum()), sgdgd=float((w * sg * dg).sum()))
        line = (lambda v: v[None, :]) if axis == 'x' else (lambda v: v[:, None])
        tables[qg] = ww * line(sg)
        tables[qd] = ww * line(dg)
    quad = np.zeros((n, n), np.float64)
    quad[0:R + 1, R + 1:] = -1.0
    quad[0:R, 0:R + 1] = 1.0
    quad[R:, 0:R] = -1.0
    quad[R + 1:, R:] = 1.0
    return dict(fwhm=fwhm, sigma=sigma, R=R, g=g, fp=fp, npixels=npixels, K=K, relerr=relerr, w=w, p=p, consts=consts,
                tables=tables.reshape(NQ, n * n), quad=quad)


def subtract_bg(data, bg_median):
    return np.asarray(data, np.float32) - np.float32(bg_median)


def convolve(d, K):
    """The contract's convolution of the float32 image d with the (2R+1)^2 float64 kernel K -> float32."""
    d = np.asarray(d, np.float32)
    H, W = d.shape
    R = K.shape[0] // 2
    pad = np.zeros((H + 2 * R, W + 2 * R), np.float64)
    pad[R:R + H, R:R + W] = d
    acc = np.zeros((H, W), np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(2 * R + 1):
            for b in range(2 * R + 1):
                # d[i + R - a, j + R - b] = pad[i + 2R - a, j + 2R - b]
                acc = acc + pad[2 * R - a:2 * R - a + H, 2 * R - b:2 * R - b + W] * K[a, b]
        return acc.astype(np.float32)


def find_peaks(v, footprint, threshold, mask=None, border=0):
    """Flat indices (int64, ascending) of the peaks of the float32 plane v."""
    v = np.asarray(v, np.float32)
    H, W = v.shape
    fp = np.asarray(footprint) != 0
    fh, fw = fp.shape
    ch, cw = fh // 2, fw // 2
    with np.errstate(invalid='ignore'):
        ok = v.astype(np.float64) > float(threshold)
    if mask is not None:
        ok &= np.asarray(mask) == 0
    inner = np.zeros((H, W), bool)
    if H > 2 * border and W > 2 * border:
        inner[border:H - border, border:W - border] = True
    ok &= inner
    idx = np.flatnonzero(ok)
    out = []
    for q in idx:
        i, j = divmod(int(q), W)
        c = v[i, j]
        good = True
        for a in range(fh):
            ii = i + a - ch
            for b in range(fw):
                if not fp[a, b]:
                    continue
                jj = j + b - cw
                nb = v[ii, jj] if (0 <= ii < H and 0 <= jj < W) else np.float32(0.0)
                if nb > c:
                    good = False
                    break
            if not good:
                break
        if good:
            out.append(q)
    return np.asarray(out, np.int64)


def _f(x):
    return np.float64(x)


def daofind_measure(d, conv, peaks, kernel, threshold_eff, sharplo=SHARPLO, sharphi=SHARPHI, roundlo=ROUNDLO, roundhi=ROUNDHI):
    """d: the float32 image the convolution saw (background subtracted).  Returns dict(rec [n, 16] float64 in REC order,
    keep [n] bool, sums [n, NQ + 2] float64 = the NQ data sums, sum2, sum4, abs [n, NQ + 2] = the sums of the absolute
    values of their terms)."""
    d = np.asarray(d, np.float32)
    conv = np.asarray(conv, np.float32)
    H, W = d.shape
    R = kernel['R']
    n = 2 * R + 1
    T = kernel['tables']
    quad = kernel['quad'].ravel()
    cx, cy, p = kernel['consts']['x'], kernel['consts']['y'], _f(kernel['p'])
    sigsq = _f(kernel['sigma']) * _f(kernel['sigma'])
    npm1 = _f(kernel['npixels'] - 1)
    thr = _f(threshold_eff)
    rec = np.full((len(peaks), len(REC)), np.nan)
    keep = np.zeros(len(peaks), bool)
    sums = np.zeros((len(peaks), NQ + 2))
    sabs = np.zeros((len(peaks), NQ + 2))
    with np.errstate(all='ignore'):
        for k, q in enumerate(peaks):
            i, j = divmod(int(q), W)
            D = d[i - R:i + R + 1, j - R:j + R + 1].astype(np.float64).ravel()
            C = conv[i - R:i + R + 1, j - R:j + R + 1].astype(np.float64).ravel()
            for t in range(NQ):
                prod = D * T[t]
                sums[k, t], sabs[k, t] = prod.sum(), np.abs(prod).sum()
            prod = C * quad
            sums[k, NQ], sabs[k, NQ] = prod.sum(), np.abs(prod).sum()
            Cz = np.abs(C)
            Cz[R * n + R] = 0.0
            sums[k, NQ + 1] = sabs[k, NQ + 1] = Cz.sum()
            r = derive(sums[k], _f(d[i, j]), _f(conv[i, j]), i, j, R, npm1, p, cx, cy, sigsq, thr)
            rec[k] = [r[nm] for nm in REC]
            keep[k] = keep_rule(r, R, sharplo, sharphi, roundlo, roundhi)
    return dict(rec=rec, keep=keep, sums=sums, abs=sabs)


def derive(s, peak, conv_peak, i, j, R, npm1, p, cx, cy, sigsq, thr):
    """The scalar arithmetic after the sums, in the order the kernel evaluates it (float64, one rounding per operation)."""
    with np.errstate(all='ignore'):
        sfp, sumd = _f(s[Q_FP]), _f(s[Q_SUMD])
        sharp = (peak - (sfp - peak) / npm1) / conv_peak
        sum2, sum4 = _f(s[NQ]), _f(s[NQ + 1])
        if sum2 == 0.0:
            round1 = _f(0.0)
        elif sum4 <= 0.0:
            round1 = _f(np.nan)
        else:
            round1 = 2.0 * sum2 / sum4
        out = {}
        for tag, c, qg, qd in (('x', cx, Q_SUMGD_X, Q_SDDGD_X), ('y', cy, Q_SUMGD_Y, Q_SDDGD_Y)):
            sumg, sumgsq = _f(c['sumg']), _f(c['sumgsq'])
            h = (_f(s[qg]) - sumg * sumd / p) / (sumgsq - sumg * sumg / p)
            dd = (_f(c['sgdgd']) - (_f(s[qd]) - _f(c['sdgd']) * sumd)) / (h * _f(c['sdgds']) / sigsq)
            out['h' + tag], out['d' + tag] = h, dd
        hx, hy = out['hx'], out['hy']
        round2 = 2.0 * (hx - hy) / (hx + hy)
        flux = conv_peak / thr
        mag = -2.5 * np.log10(flux) if flux > 0 else _f(np.nan)
        out.update(x_peak=_f(j), y_peak=_f(i), npix=_f((2 * R + 1) ** 2), peak=peak, conv_peak=conv_peak, sharpness=sharp,
                   roundness1=round1, roundness2=round2, xcentroid=_f(j) + out['dx'], ycentroid=_f(i) + out['dy'], flux=flux,
                   mag=mag)
        return out


def keep_rule(r, R, sharplo=SHARPLO, sharphi=SHARPHI, roundlo=ROUNDLO, roundhi=ROUNDHI):
    if not (r['hx'] > 0.0 and r['hy'] > 0.0):
        return False
    if not (sharplo < r['sharpness'] < sharphi and roundlo < r['roundness1'] < roundhi and roundlo < r['roundness2'] < roundhi):
        return False
    if abs(r['dx']) > R or abs(r['dy']) > R:
        return False
    return all(np.isfinite(r[k]) for k in ('xcentroid', 'ycentroid', 'sharpness', 'roundness1', 'roundness2', 'peak', 'flux'))


# ---- aperture photometry ------------------------------------------------------------------------------------------------
def _arc_integral(u, v, r):
    """integral of sqrt(r^2 - x^2) over [u, v], -r <= u <= v <= r: trapezoid under the chord + circular segment."""
    if not v > u:
        return 0.0
    hu = math.sqrt(max(r * r - u * u, 0.0))
    hv = math.sqrt(max(r * r - v * v, 0.0))
    w = v - u
    dh = hv - hu
    c = math.sqrt(w * w + dh * dh)
    s = c / (2.0 * r)
    if s > 1.0:
        s = 1.0
    t = 2.0 * math.asin(s)
    return w * (hu + hv) / 2.0 + r * r / 2.0 * (t - math.sin(t))


def _clamp_integral(y, X0, X1, r):
    """integral over [X0, X1] (inside [-r, r]) of clamp(y, -h(x), h(x))."""
    ya = abs(y)
    if ya >= r:
        val = _arc_integral(X0, X1, r)
    else:
        a = math.sqrt(r * r - ya * ya)
        val = 0.0
        lo, hi = X0, min(X1, -a)              # left of -a: the arc
        if hi > lo:
            val = val + _arc_integral(lo, hi, r)
        lo, hi = max(X0, -a), min(X1, a)      # between: the line y
        if hi > lo:
            val = val + ya * (hi - lo)
        lo, hi = max(X0, a), X1               # right of a: the arc
        if hi > lo:
            val = val + _arc_integral(lo, hi, r)
    return -val if y < 0 else val


def pixel_overlap(x0, x1, y0, y1, r):
    """Area of the circle of radius r about the origin inside [x0, x1] x [y0, y1] (a unit pixel)."""
    fx = max(abs(x0), abs(x1))
    fy = max(abs(y0), abs(y1))
    if fx * fx + fy * fy <= r * r:
        return 1.0
    nx = 0.0 if x0 <= 0.0 <= x1 else min(abs(x0), abs(x1))
    ny = 0.0 if y0 <= 0.0 <= y1 else min(abs(y0), abs(y1))
    if nx * nx + ny * ny >= r * r:
        return 0.0
    X0, X1 = max(x0, -r), min(x1, r)
    if not X1 > X0:
        return 0.0
    a = _clamp_integral(y1, X0, X1, r) - _clamp_integral(y0, X0, X1, r)
    return a if a > 0.0 else 0.0


def _bbox(c, r, n):
    lo = max(0, int(math.ceil(c - r - 0.5)))
    hi = min(n - 1, int(math.floor(c + r + 0.5)))
    return lo, hi


def circle_overlap(cx, cy, r, H, W):
    """[H, W] float64: area of the circle (centre x = cx, y = cy) inside every pixel of the image."""
    out = np.zeros((H, W), np.float64)
    i0, i1 = _bbox(cy, r, H)
    j0, j1 = _bbox(cx, r, W)
    for i in range(i0, i1 + 1):
        y0, y1 = (i - 0.5) - cy, (i + 0.5) - cy
        for j in range(j0, j1 + 1):
            out[i, j] = pixel_overlap((j - 0.5) - cx, (j + 0.5) - cx, y0, y1, r)
    return out


def annulus_clip(values, sigma=3.0, maxiters=5):
    """astropy.stats.sigma_clipped_stats(values) (noaxis path, median centre, std) on float32 values, with the rule
    ops.sigclip_global follows: non-finite values dropped, numpy's float32 median / mean / std, the bounds formed in
    float64 and demoted to float32 for the comparison.  Returns (mean, median, std) as float32 (NaN if nothing is left)."""
    x = np.asarray(values, np.float32).ravel()
    x = x[np.isfinite(x)]
    it = 0
    while x.size and (maxiters is None or it < maxiters):
        med, sd = np.median(x), np.std(x)
        lo = np.float32(np.float64(med) - np.float64(sd) * sigma)
        hi = np.float32(np.float64(med) + np.float64(sd) * sigma)
        y = x[(x >= lo) & (x <= hi)]
        changed = y.size != x.size
        x = y
        it += 1
        if not changed:
            break
    if x.size == 0:
        nan = np.float32(np.nan)
        return nan, nan, nan
    return np.float32(np.mean(x)), np.float32(np.median(x)), np.float32(np.std(x))


def aperture_radii(fwhm):
    r = math.ceil(2.0 * fwhm)
    return float(r), float(r), float(math.ceil(1.5 * r))


def annulus_values(data, xc, yc, r_in, r_out):
    data = np.asarray(data, np.float32)
    H, W = data.shape
    i0, i1 = _bbox(yc, r_out, H)
    j0, j1 = _bbox(xc, r_out, W)
    vals = []
    for i in range(i0, i1 + 1):
        dy = np.float64(i) - np.float64(yc)
        for j in range(j0, j1 + 1):
            dx = np.float64(j) - np.float64(xc)
            d2 = dx * dx + dy * dy
            if r_in * r_in <= d2 <= r_out * r_out:
                vals.append(data[i, j])
    return np.asarray(vals, np.float32)


def aperture_photometry(data, xc, yc, fwhm):
    """dict of arrays per source: aperture_sum_raw, abs (sum |overlap * data|), npix (pixels with overlap > 0), bkg_median
    (float32), n_annulus, area, aperture_sum."""
    data = np.asarray(data, np.float32)
    H, W = data.shape
    r, r_in, r_out = aperture_radii(fwhm)
    n = len(xc)
    out = dict(aperture_sum_raw=np.zeros(n), abs=np.zeros(n), npix=np.zeros(n, np.int64), bkg_median=np.zeros(n, np.float32),
               n_annulus=np.zeros(n, np.int64), area=np.zeros(n), aperture_sum=np.zeros(n))
    for k in range(n):
        ov = circle_overlap(float(xc[k]), float(yc[k]), r, H, W)
        sel = ov > 0
        with np.errstate(invalid='ignore'):
            prod = ov[sel] * data[sel].astype(np.float64)            # boolean indexing: row-major order
        s = np.float64(0.0)
        for t in prod:
            s = s + t
        out['aperture_sum_raw'][k] = s
        out['abs'][k] = np.abs(prod).sum()
        out['npix'][k] = sel.sum()
        a = np.float64(0.0)
        for t in ov[sel]:
            a = a + t
        out['area'][k] = a
        vals = annulus_values(data, float(xc[k]), float(yc[k]), r_in, r_out)
        out['n_annulus'][k] = vals.size
        out['bkg_median'][k] = annulus_clip(vals)[1]
        out['aperture_sum'][k] = s - np.float64(out['bkg_median'][k]) * (math.pi * r * r)
    return out


# ---- the class's flow ----------------------------------------------------------------------------------------------------
def saturation_boxes(sat_idx, W, H, fwhm):
    """The rectangles {r0, r1, c0, c1} (half-open) the reference masks round every saturated peak (ApFindStars.py:178-185)."""
    bw = int(4 * fwhm)
    rects = []
    for q in sat_idx:
        srow, scol = divmod(int(q), W)
        rects.append([max(0, srow - bw + 1), min(H, srow + bw), max(0, scol - bw + 1), min(W, scol + bw)])
    return np.asarray(rects, np.int32).reshape(-1, 4)


def find_stars(data, fwhm, threshold, bg_median=0.0, mask=None):
    """source_search on the model: dict(rec (kept rows only), idx, all)."""
    k = daofind_kernel(fwhm)
    d = subtract_bg(data, bg_median)
    conv = convolve(d, k['K'])
    thr_eff = threshold * k['relerr']
    peaks = find_peaks(conv, k['fp'], thr_eff, mask=mask, border=k['R'])
    m = daofind_measure(d, conv, peaks, k, thr_eff)
    return dict(rec=m['rec'][m['keep']], idx=peaks[m['keep']], all=m, peaks=peaks, conv=conv, kernel=k, threshold_eff=thr_eff)
