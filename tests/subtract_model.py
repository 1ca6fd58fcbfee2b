"""The optimal image subtraction (F23) restated in numpy: the kernel basis, the per-stamp normal equations, the host fit
with its stamp rejection, the composite kernels and the float32 application, each in the order of operations that DESIGN fixes
(csrc/subtract_core.h, csrc/subtract.hip and ops.subtract_* state the same).  Numpy only.  The GPU tests hold the kernels to this
file, tests/test_subtract_model_host.py holds this file to planted truth.

x = column, y = row.  (T (x) K)(x, y) = sum_{u, v} K(u, v) T(x - u, y - v); a kernel of radius r is an array [2 r + 1, 2 r + 1] with
K(u, v) at [v + r, u + r].
"""
import functools
import math

import numpy as np

MAX_RADIUS, MAX_BASIS, MAX_DEGREE, MAX_HALF = 15, 64, 3, 15
DEFAULT_SIGMAS, DEFAULT_DEGREES, DEFAULT_RADIUS = (0.7, 1.5, 3.0), (6, 4, 2), 10
ST_OUTSIDE, ST_TEMPLATE, ST_IMAGE, ST_MASK = 1, 2, 4, 8


def ipow(x, k):
    """x^k by repeated multiplication from 1."""
    p = np.ones_like(np.asarray(x, np.float64))
    for _ in range(k):
        p = p * x
    return p


def poly_exponents(d):
    return [(i, j) for i in range(d + 1) for j in range(d + 1 - i)]


def norm_coord(p, n):
    return (2 * np.asarray(p, np.int64) - (n - 1)) / float(max(n - 1, 1))


def poly_terms(d, X, Y):
    """[terms, ...]: X^i Y^j for i + j <= d, i then j ascending."""
    return np.stack([ipow(X, i) * ipow(Y, j) for i, j in poly_exponents(d)])


def basis(sigmas=DEFAULT_SIGMAS, degrees=DEFAULT_DEGREES, radius=DEFAULT_RADIUS):
    """The basis in its separable form and dense: a dict of filters [NF, kw], row, col, even (int), scale [Nb] and B [Nb, kw, kw]."""
    sigmas, degrees, r = [float(s) for s in sigmas], [int(d) for d in degrees], int(radius)
    if len(sigmas) != len(degrees) or not sigmas:
        raise ValueError('one degree per Gaussian')
    if not 1 <= r <= MAX_RADIUS or any(not (s > 0 and math.isfinite(s)) for s in sigmas) or any(d < 0 for d in degrees):
        raise ValueError('radius, sigma or degree out of range')
    if sum((d + 1) * (d + 2) // 2 for d in degrees) > MAX_BASIS:
        raise ValueError('more than %d basis functions' % MAX_BASIS)
    kw = 2 * r + 1
    filters, row, col, even, scale = [], [], [], [], []
    f0 = 0
    for s, d in zip(sigmas, degrees):
        for p in range(d + 1):
            line = []
            for u in range(-r, r + 1):
                du = float(u)
                pw = 1.0
                for _ in range(p):
                    pw = pw * du
                line.append(math.exp(-(du * du) / (2.0 * (s * s))) * pw)
            filters.append(line)
        for i in range(d + 1):
            for j in range(d + 1 - i):
                row.append(f0 + i)
                col.append(f0 + j)
                even.append(int(i % 2 == 0 and j % 2 == 0))
                sc = 1.0
                if even[-1]:
                    tot = 0.0
                    for v in range(kw):
                        ln = 0.0
                        for u in range(kw):
                            ln = ln + filters[row[-1]][u] * filters[col[-1]][v]
                        tot = tot + ln
                    sc = 1.0 / tot
                scale.append(sc)
        f0 += d + 1
    filters = np.array(filters, np.float64)
    scale = np.array(scale, np.float64)
    nb = len(row)
    B = np.empty((nb, kw, kw))
    for n in range(nb):
        B[n] = scale[n] * (filters[col[n]][:, None] * filters[row[n]][None, :])          # [v, u]
        if n > 0 and even[n]:
            B[n] = B[n] - B[0]
    return dict(filters=filters, row=np.array(row, np.int32), col=np.array(col, np.int32), even=np.array(even, np.int32), scale=scale,
                B=B, radius=r, nb=nb, sigmas=sigmas, degrees=degrees)


def stamp_vectors(T, cx, cy, h, bs):
    """[Nb, n, n] float64: T (x) B_n over the stamp about (cx, cy), in the kernel's order of operations."""
    r, n = bs['radius'], 2 * h + 1
    F = h + r
    foot = np.asarray(T[cy - F:cy + F + 1, cx - F:cx + F + 1], np.float64)
    if not np.all(np.isfinite(foot)):
        return np.full((bs['nb'], n, n), np.nan)
    rfs = []
    for f in range(bs['filters'].shape[0]):
        a = np.zeros((2 * F + 1, n))
        for u in range(-r, r + 1):
            a = a + bs['filters'][f, u + r] * foot[:, r - u:r - u + n]
        rfs.append(a)
    V = np.empty((bs['nb'], n, n))
    for k in range(bs['nb']):
        a = np.zeros((n, n))
        for v in range(-r, r + 1):
            a = a + bs['filters'][bs['col'][k], v + r] * rfs[bs['row'][k]][r - v:r - v + n, :]
        V[k] = bs['scale'][k] * a
    for k in range(1, bs['nb']):
        if bs['even'][k]:
            V[k] = V[k] - V[0]
    return V


def stamps(T, I, centers, h, bs, mask=None, gain=0.0, readnoise=0.0):
    """(gram float64 [S, Nb + 2, Nb + 2], status int32 [S], count int32 [S]) as apgpu_subtract_stamps_f32 defines them."""
    H, W = T.shape
    r, nb, n = bs['radius'], bs['nb'], 2 * h + 1
    F = h + r
    centers = np.asarray(centers, np.int64).reshape(-1, 2)
    S = len(centers)
    gram = np.zeros((S, nb + 2, nb + 2))
    status = np.zeros(S, np.int32)
    count = np.zeros(S, np.int32)
    for s, (cx, cy) in enumerate(centers):
        if cx - F < 0 or cx + F >= W or cy - F < 0 or cy + F >= H:
            status[s] = ST_OUTSIDE
            continue
        st = 0
        if not np.all(np.isfinite(T[cy - F:cy + F + 1, cx - F:cx + F + 1])):
            st |= ST_TEMPLATE
        iv = np.asarray(I[cy - h:cy + h + 1, cx - h:cx + h + 1], np.float64)
        if not np.all(np.isfinite(iv)):
            st |= ST_IMAGE
        if mask is not None and np.any(mask[cy - h:cy + h + 1, cx - h:cx + h + 1] != 0):
            st |= ST_MASK
        if st:
            status[s] = st
            continue
        vec = np.concatenate([stamp_vectors(T, cx, cy, h, bs), np.ones((1, n, n)), iv[None]]).reshape(nb + 2, n * n)
        w = 1.0 / ((readnoise * readnoise) / (gain * gain) + np.maximum(iv, 0.0) / gain) if gain > 0 else np.ones((n, n))
        wv = w.reshape(1, -1) * vec
        g = np.zeros((nb + 2, nb + 2))
        for p in range(n * n):                                   # row-major, one pixel after the other
            g = g + wv[:, p, None] * vec[None, :, p]
        iu = np.triu_indices(nb + 2)
        g[(iu[1], iu[0])] = g[iu]                                # the lower triangle is the upper one: (w V_a) V_b with a <= b
        gram[s] = g
        count[s] = n * n
    return gram, status, count


def stamp_abs_sums(T, I, centers, h, bs, gain=0.0, readnoise=0.0):
    """sum over the pixels of |(w V_a) V_b| per stamp, [S, Nb + 2, Nb + 2] (stamps inside the image): what the GPU tests' bound on the
    Gram sums is made of."""
    n = 2 * h + 1
    F = h + bs['radius']
    H, W = T.shape
    out = np.zeros((len(centers), bs['nb'] + 2, bs['nb'] + 2))
    for s, (cx, cy) in enumerate(np.asarray(centers, np.int64).reshape(-1, 2)):
        if cx - F < 0 or cx + F >= W or cy - F < 0 or cy + F >= H:
            continue
        iv = np.asarray(I[cy - h:cy + h + 1, cx - h:cx + h + 1], np.float64)
        vec = np.abs(np.concatenate([stamp_vectors(T, cx, cy, h, bs), np.ones((1, n, n)), iv[None]]).reshape(bs['nb'] + 2, n * n))
        w = 1.0 / ((readnoise * readnoise) / (gain * gain) + np.maximum(iv, 0.0) / gain) if gain > 0 else np.ones((n, n))
        with np.errstate(invalid='ignore'):
            out[s] = (w.reshape(1, -1) * vec) @ vec.T
    return out


def _design(nb, kdeg, bdeg, X, Y):
    """P [unknowns, Nb + 1] of a stamp centred at the normalised (X, Y): the unknowns are a_0, then a_{n,t} (n = 1 .. Nb - 1 outside, t
    inside), then c_t; column m is the fit vector V_m (V_Nb = 1)."""
    pk, pb = poly_terms(kdeg, X, Y), poly_terms(bdeg, X, Y)
    ntk, ntb = len(pk), len(pb)
    P = np.zeros((1 + (nb - 1) * ntk + ntb, nb + 1))
    P[0, 0] = 1.0
    for n in range(1, nb):
        P[1 + (n - 1) * ntk:1 + n * ntk, n] = pk
    P[1 + (nb - 1) * ntk:, nb] = pb
    return P


def fit(gram, status, count, centers, shape, kdeg=2, bdeg=1, k=3.0, rounds=3):
    """The host fit.  Returns a dict: theta (the unknowns in _design's order), a0, akt [Nb, ntk] (row 0: a_0 in column 0), bg [ntb],
    kept (bool [S]), chi2 [S] (per pixel; NaN for a refused stamp), cond (of the scaled normal matrix), rounds (fits made), margin
    (the smallest |chi2 - cut| / cut over the stamps of the last rejection round)."""
    H, W = shape
    S, nv = gram.shape[0], gram.shape[1]
    nb = nv - 2
    if not 0 <= kdeg <= MAX_DEGREE or not 0 <= bdeg <= MAX_DEGREE:
        raise ValueError('degrees outside 0 .. %d' % MAX_DEGREE)
    centers = np.asarray(centers, np.int64).reshape(-1, 2)
    ntk, ntb = (kdeg + 1) * (kdeg + 2) // 2, (bdeg + 1) * (bdeg + 2) // 2
    Ps = [_design(nb, kdeg, bdeg, float(norm_coord(cx, W)), float(norm_coord(cy, H))) for cx, cy in centers]
    kept = np.asarray(status) == 0
    chi2 = np.full(S, np.nan)
    margin, made = np.inf, 0
    while True:
        if kept.sum() < max(ntk, ntb):
            raise ArithmeticError('%d usable stamps for %d spatial terms' % (kept.sum(), max(ntk, ntb)))
        M = np.zeros((Ps[0].shape[0],) * 2)
        rhs = np.zeros(Ps[0].shape[0])
        for s in np.flatnonzero(kept):
            M = M + Ps[s] @ gram[s, :nb + 1, :nb + 1] @ Ps[s].T
            rhs = rhs + Ps[s] @ gram[s, :nb + 1, nb + 1]
        d = np.sqrt(np.diag(M))
        if not np.all(d > 0):
            raise ArithmeticError('the normal matrix has an empty row')
        Ms = M / d[:, None] / d[None, :]
        theta = np.linalg.solve(Ms, rhs / d) / d
        made += 1
        for s in np.flatnonzero(np.asarray(status) == 0):
            q = Ps[s].T @ theta
            chi2[s] = (gram[s, nb + 1, nb + 1] - 2.0 * (q @ gram[s, :nb + 1, nb + 1]) + q @ gram[s, :nb + 1, :nb + 1] @ q) / count[s]
        if made > rounds:
            break
        c = chi2[kept]
        med = np.median(c)
        cut = med + k * 1.4826 * np.median(np.abs(c - med))
        drop = kept & (chi2 > cut)
        margin = float(np.min(np.abs(c - cut)) / cut)
        if not drop.any():
            break
        kept = kept & ~drop
    akt = np.zeros((nb, ntk))
    akt[0, 0] = theta[0]
    akt[1:] = theta[1:1 + (nb - 1) * ntk].reshape(nb - 1, ntk)
    return dict(theta=theta, a0=float(theta[0]), akt=akt, bg=theta[1 + (nb - 1) * ntk:].copy(), kept=kept, chi2=chi2,
                cond=float(np.linalg.cond(Ms)), rounds=made, margin=margin, scale_diag=d)


def composites(akt, bs, dtype=np.float32):
    """A_t = sum_n a_{n,t} B_n, n ascending from +0 in float64, rounded to dtype: [ntk, kw, kw]."""
    out = np.zeros((akt.shape[1],) + bs['B'].shape[1:])
    for t in range(akt.shape[1]):
        for n in range(bs['nb']):
            out[t] = out[t] + akt[n, t] * bs['B'][n]
    return out.astype(dtype)


def kernel_at(akt, bs, kdeg, X, Y):
    """The float64 kernel at the normalised position (X, Y)."""
    return np.tensordot(poly_terms(kdeg, float(X), float(Y)), composites(akt, bs, np.float64), 1)


def apply(src, other, kernels, kdeg, bg, bdeg, convolved_image=False, a0=1.0, dtype=np.float32):
    """(diff, matched) as apgpu_subtract_apply_f32 defines them (dtype float32), or the same expressions in float64."""
    ft = np.dtype(dtype).type
    H, W = src.shape
    r = (kernels.shape[1] - 1) // 2
    kernels = np.asarray(kernels, dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        S = np.full((H + 2 * r, W + 2 * r), np.nan, dtype)
        S[r:r + H, r:r + W] = np.where(np.isfinite(src), src, np.nan)
        acc = [np.zeros((H, W), dtype) for _ in kernels]
        for u in range(-r, r + 1):
            for v in range(-r, r + 1):
                sh = S[r - v:r - v + H, r - u:r - u + W]
                for t in range(len(kernels)):
                    acc[t] = acc[t] + kernels[t, v + r, u + r] * sh
        X, Y = norm_coord(np.arange(W), W)[None, :], norm_coord(np.arange(H), H)[:, None]
        pk = poly_terms(kdeg, X + 0 * Y, Y + 0 * X)
        conv = np.zeros((H, W), dtype)
        for t in range(len(kernels)):
            conv = conv + pk[t].astype(dtype) * acc[t]
        B = np.zeros((H, W))
        for t, (i, j) in enumerate(poly_exponents(bdeg)):
            B = B + float(bg[t]) * (ipow(X, i) * ipow(Y, j))
        B = B.astype(dtype)
        o = np.asarray(other, dtype)
        matched = conv + B
        diff = (matched - o) / ft(a0) if convolved_image else (o - conv) - B
        diff = np.where(np.isfinite(o) & ~np.isnan(diff), diff, ft(np.nan)).astype(dtype)      # every NaN is the one quiet NaN
        matched = np.where(np.isnan(matched), ft(np.nan), matched).astype(dtype)
    return diff, matched


def select_stamps(x, y, flux, shape, h, r, peak=None, satlevel=None, nx=4, ny=4, per_region=5):
    """The stamp centres [S, 2] int (x, y) of a star list: stars with a peak at satlevel dropped, of two stars closer than 2 h the
    fainter dropped, stamps whose footprint h + r leaves the image dropped, the brightest per_region of each cell of an nx x ny
    grid kept; in the order of falling flux."""
    H, W = shape
    x, y, flux = (np.asarray(a, np.float64) for a in (x, y, flux))
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(flux)
    if peak is not None and satlevel is not None:
        ok &= ~(np.asarray(peak, np.float64) >= satlevel)
    order = [i for i in np.argsort(-np.where(ok, flux, -np.inf), kind='stable') if ok[i]]
    taken, cells, out = [], {}, []
    for i in order:
        cx, cy = int(np.rint(x[i])), int(np.rint(y[i]))
        if any(math.hypot(x[i] - x[j], y[i] - y[j]) < 2 * h for j in taken):
            continue
        taken.append(i)
        if cx - h - r < 0 or cx + h + r >= W or cy - h - r < 0 or cy + h + r >= H:
            continue
        cell = (min(cx * nx // W, nx - 1), min(cy * ny // H, ny - 1))
        if cells.get(cell, 0) >= per_region:
            continue
        cells[cell] = cells.get(cell, 0) + 1
        out.append((cx, cy))
    return np.array(out, np.int64).reshape(-1, 2)


# ---- the planted scene -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def true_kernel_field(shape, r):
    """The out-of-span planted kernel K_true(u, v; x, y) [kw, kw, H, W] (sum 1 at every pixel): a Gaussian whose covariance grows and
    tilts across the field - the kernel that takes a round sigma = 1.1 PSF to one that broadens and turns elliptical."""
    H, W = shape
    X, Y = norm_coord(np.arange(W), W)[None, :], norm_coord(np.arange(H), H)[:, None]
    sxx = 0.50 + 0.35 * (X + 1.0) + 0.0 * Y
    syy = 0.50 + 0.15 * (Y + 1.0) + 0.10 * (X + 1.0) * (Y + 1.0) * 0.5
    sxy = 0.20 * X * Y
    det = sxx * syy - sxy * sxy
    u = np.arange(-r, r + 1, dtype=np.float64)
    uu, vv = u[None, :, None, None], u[:, None, None, None]
    K = np.exp(-0.5 * (syy * uu * uu - 2.0 * sxy * uu * vv + sxx * vv * vv) / det)
    return K / K.sum(axis=(0, 1))


def convolve_field(T, K):
    """sum_{u,v} K[v + r, u + r, y, x] T(x - u, y - v) in float64, the template extended by its edge values."""
    r = (K.shape[0] - 1) // 2
    H, W = T.shape
    Tp = np.pad(np.asarray(T, np.float64), r, mode='edge')
    out = np.zeros((H, W))
    for v in range(-r, r + 1):
        for u in range(-r, r + 1):
            out = out + K[v + r, u + r] * Tp[r - v:r - v + H, r - u:r - u + W]
    return out


def make_scene(seed=0, size=256, grid=8, scale=0.8, noise_image=5.0, noise_template=2.0, r_true=6, variable=None, variable_ratio=1.5,
               peak_lo=800.0, peak_hi=4000.0):
    """The planted pair.  Returns a dict: image, template (float32), stars x, y, flux (of the template), K (the planted kernel field),
    scale, bg (the planted sky difference [H, W]), conv (the noise-free scale T0 (x) K_true + bg).  Stars sit on a jittered grid,
    at least 26 pixels apart and 21 from the edges; the template's PSF is a round Gaussian of sigma 1.1."""
    rng = np.random.default_rng(seed)
    H = W = size
    pitch = (size - 46) / (grid - 1)
    gx, gy = np.meshgrid(np.arange(grid), np.arange(grid))
    x = 23.0 + pitch * gx.ravel() + rng.uniform(-2.0, 2.0, grid * grid)
    y = 23.0 + pitch * gy.ravel() + rng.uniform(-2.0, 2.0, grid * grid)
    peak = np.exp(rng.uniform(np.log(peak_lo), np.log(peak_hi), grid * grid))
    sig = 1.1
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    star_img = [np.zeros((H, W)), np.zeros((H, W))]                  # [the others, the variable]
    for i in range(len(x)):
        x0, x1, y0, y1 = max(int(x[i]) - 9, 0), min(int(x[i]) + 10, W), max(int(y[i]) - 9, 0), min(int(y[i]) + 10, H)
        g = peak[i] * np.exp(-((xx[y0:y1, x0:x1] - x[i]) ** 2 + (yy[y0:y1, x0:x1] - y[i]) ** 2) / (2 * sig * sig))
        star_img[int(variable is not None and i == variable)][y0:y1, x0:x1] += g
    sky_t = 100.0
    T0 = sky_t + star_img[0] + star_img[1]
    K = true_kernel_field((H, W), r_true)
    X, Y = norm_coord(np.arange(W), W)[None, :], norm_coord(np.arange(H), H)[:, None]
    bg = 40.0 + 15.0 * X + 8.0 * Y
    conv = scale * convolve_field(T0, K) + bg
    if variable is not None:
        conv = conv + (variable_ratio - scale) * convolve_field(star_img[1], K)
    image = conv + noise_image * rng.standard_normal((H, W))
    template = T0 + noise_template * rng.standard_normal((H, W))
    return dict(image=image.astype(np.float32), template=template.astype(np.float32), x=x, y=y, flux=peak * 2 * np.pi * sig * sig, peak=peak,
                K=K, scale=scale, bg=bg, conv=conv, noise_image=noise_image, noise_template=noise_template)


def optimal_subtract(image, template, centers, h, bs, kdeg=2, bdeg=1, mask=None, gain=0.0, readnoise=0.0, k=3.0, rounds=3,
                     convolve='template', dtype=np.float32):
    """End to end on given stamp centres: stamps, fit, composites, apply.  Returns the fit's dict with diff, matched, kernels added."""
    src, oth = (template, image) if convolve == 'template' else (image, template)
    gram, status, count = stamps(src, oth, centers, h, bs, mask=mask, gain=gain, readnoise=readnoise)
    f = fit(gram, status, count, centers, image.shape, kdeg, bdeg, k, rounds)
    kernels = composites(f['akt'], bs, dtype)
    diff, matched = apply(src, oth, kernels, kdeg, f['bg'], bdeg, convolve == 'image', f['a0'], dtype)
    return dict(f, diff=diff, matched=matched, kernels=kernels, gram=gram, status=status, count=count)
