"""NumPy model of F13, the starlet (B3-spline a trous) denoise and sharpen step (include/apgpu.h F13).  The reference
has no such stage: this file is the definition the kernels of csrc/multiscale.hip are held to, bit for bit.

  taps     h = [1, 4, 6, 4, 1] / 16 at offsets (k - 2) s, s = 2^j.  valid(y, x): inside the image and finite in the input.
  step     row pass: a = sum_k h[k] double(c(y, x + (k - 2) s)), m = sum_k h[k] over the valid taps, k ascending, float64 from +0;
           column pass: A = sum_k h[k] a(y + (k - 2) s, x), M = sum_k h[k] m(y + (k - 2) s, x) over the rows inside the image;
           c' = float32(A / M) where valid, NaN elsewhere.  Every multiply and add rounds on its own.
  planes   w_{j+1} = c_j - c_{j+1} in float32
  noise    sigma_e[j]: the 2-norm of the impulse response of plane j + 1, float64, from the taps
  treat    t_j = float32(k_j sigma sigma_e[j-1]); hard: w where |w| >= t, else +0; soft: w - t above t, w + t below -t, else +0
  sum      float32: acc = +0; acc = acc + g_j T(w_j), j = 1 .. J; out = acc + g_res c_J
"""
import math

import numpy as np

F = np.float32
TAPS = np.array([1.0, 4.0, 6.0, 4.0, 1.0], np.float64) / 16.0
MAX_SCALES = 6
DEFAULT_K = (3.0, 3.0, 2.0, 1.0)


def step(c, s):
    """c_j -> c_{j+1} at spacing s."""
    c = np.asarray(c, F)
    H, W = c.shape
    ok = np.isfinite(c)
    v = np.where(ok, c, F(0)).astype(np.float64)
    a, m = np.zeros((H, W)), np.zeros((H, W))
    for k in range(5):
        d = (k - 2) * s
        if abs(d) >= W:
            continue
        dst, src = slice(max(0, -d), min(W, W - d)), slice(max(0, d), min(W, W + d))
        okk = ok[:, src]
        a[:, dst] = np.where(okk, a[:, dst] + TAPS[k] * v[:, src], a[:, dst])
        m[:, dst] = np.where(okk, m[:, dst] + TAPS[k], m[:, dst])
    A, M = np.zeros((H, W)), np.zeros((H, W))
    for k in range(5):
        d = (k - 2) * s
        if abs(d) >= H:
            continue
        dst, src = slice(max(0, -d), min(H, H - d)), slice(max(0, d), min(H, H + d))
        A[dst] = A[dst] + TAPS[k] * a[src]
        M[dst] = M[dst] + TAPS[k] * m[src]
    with np.errstate(invalid='ignore', divide='ignore'):
        out = (A / M).astype(F)
    return np.where(ok, out, F(np.nan))


def planes(image, J):
    """([w_1 .. w_J], c_J); holes are NaN in all of them."""
    if not 1 <= J <= MAX_SCALES:
        raise ValueError('J must be 1 .. %d' % MAX_SCALES)
    c = np.asarray(image, F)
    c = np.where(np.isfinite(c), c, F(np.nan))
    ws = []
    for j in range(J):
        nxt = step(c, 1 << j)
        with np.errstate(invalid='ignore'):
            ws.append((c - nxt).astype(F))
        c = nxt
    return ws, c


def noise_constants(J):
    """sigma_e[0 .. J-1], float64: the standard deviation of planes 1 .. J for unit white noise far from borders and holes."""
    kern = np.ones(1)
    out = []
    for j in range(J):
        up = np.zeros(4 * (1 << j) + 1)
        up[::1 << j] = TAPS
        nxt = np.convolve(kern, up)
        prev = np.pad(kern, (nxt.size - kern.size) // 2)
        plane = np.outer(prev, prev) - np.outer(nxt, nxt)
        out.append(math.sqrt(float((plane * plane).sum())))
        kern = nxt
    return np.array(out)


def estimate_sigma(image):
    """The image noise from plane 1: the std of its finite values after clipping at 3 sigma about the median (at most 5 iterations),
    divided by sigma_e[0] (float64 statistics)."""
    w1 = planes(image, 1)[0][0]
    x = w1[np.isfinite(w1)].astype(np.float64)
    for _ in range(5):
        if x.size == 0:
            break
        med, sd = np.median(x), x.std()
        keep = (x >= med - 3.0 * sd) & (x <= med + 3.0 * sd)
        if keep.all():
            break
        x = x[keep]
    return float(x.std() / noise_constants(1)[0]) if x.size else float('nan')


def _per_scale(v, J, name):
    v = np.asarray(v, np.float64).reshape(-1)
    if v.size == 1:
        v = np.repeat(v, J)
    if v.size != J:
        raise ValueError('%s needs %d values, got %d' % (name, J, v.size))
    return v


def thresholds(k, sigma, J):
    """t_1 .. t_J as float32."""
    k, se = _per_scale(k, J, 'k'), noise_constants(J)
    return np.array([F(float(k[j]) * float(sigma) * float(se[j])) for j in range(J)], F)


def treat(w, t, mode):
    w, t = np.asarray(w, F), F(t)
    with np.errstate(invalid='ignore'):
        if mode == 'hard':
            return np.where(np.abs(w) >= t, w, F(0))
        if mode == 'soft':
            return np.where(w > t, w - t, np.where(w < -t, w + t, F(0))).astype(F)
    raise ValueError('mode must be hard or soft')


def reconstruct(ws, cJ, t, gains, g_res, mode):
    acc = np.zeros(cJ.shape, F)
    with np.errstate(invalid='ignore'):
        for j, w in enumerate(ws):
            acc = acc + F(gains[j]) * treat(w, t[j], mode)
        out = acc + F(g_res) * cJ
    return np.where(np.isfinite(cJ), out, F(np.nan)).astype(F)


def multiscale(image, J=4, k=DEFAULT_K, gains=1.0, g_res=1.0, mode='hard', sigma=None):
    """(out, report): report has sigma, t (float32 [J]), J, mode."""
    ws, cJ = planes(image, J)
    if sigma is None:
        sigma = estimate_sigma(image)
    t = thresholds(k, sigma, J)
    out = reconstruct(ws, cJ, t, _per_scale(gains, J, 'gains'), g_res, mode)
    return out, dict(sigma=float(sigma), t=t, J=J, mode=mode)


# ---- the synthetic scene of the host and end-to-end tests -----------------------------------------------------------------------
SCENE_NOISE = 5.0


def scene(seed=13, H=192, W=256):
    """A smooth nebula on a sky level, Gaussian stars of FWHM 3.5 and white noise of SCENE_NOISE, with a NaN border (as a co-add's
    footprint leaves) and a NaN block.  Returns dict(d, truth, noise, holes)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    truth = 100.0 + 60.0 * np.exp(-(((x - 0.55 * W) / (0.30 * W)) ** 2 + ((y - 0.45 * H) / (0.35 * H)) ** 2))
    truth += 25.0 * np.exp(-(((x - 0.25 * W) / (0.12 * W)) ** 2 + ((y - 0.7 * H) / (0.15 * H)) ** 2))
    s = 3.5 / 2.3548200450309493
    for _ in range(12):
        sx, sy, amp = rng.uniform(12, W - 12), rng.uniform(12, H - 12), rng.uniform(60.0, 400.0)
        truth += amp * np.exp(-((x - sx) ** 2 + (y - sy) ** 2) / (2.0 * s * s))
    d = (truth + rng.normal(0.0, SCENE_NOISE, (H, W))).astype(F)
    holes = np.zeros((H, W), bool)
    holes[:3], holes[-2:], holes[:, :2], holes[:, -4:] = True, True, True, True
    holes[70:84, 120:141] = True
    d[holes] = np.nan
    return dict(d=d, truth=truth.astype(F), noise=SCENE_NOISE, holes=holes)
