"""NumPy model of F14, the drizzle co-add of dithered frames and its blot-and-compare rejection (include/apgpu.h F14).
The reference has no such stage: this file restates the project's own definition, operation by operation, and the host test holds
it to synthetic truth (tests/test_drizzle_model_host.py); the kernels are held to it bit for bit (tests/test_gpu_drizzle.py).
No torch here.

Precisions: the output pixel's centre in the input frame, the footprint's edges and the window origin in float64; the overlaps in
float32 on coordinates relative to the window origin; cover, weighted cover and scaled value in float32; the two sums in float64
(the product they add is exact).  The rejection maps in float64 and compares in float32.  Every operation rounds on its own.
"""
import math

import numpy as np

F = np.float32
NAN = F(np.nan)
COLOURS = {'RGGB': (0, 1, 3, 2), 'BGGR': (2, 1, 3, 0), 'GRBG': (1, 0, 2, 3), 'GBRG': (1, 2, 0, 3)}   # R 0, G1 1, B 2, G2 3 at (r & 1) 2 + (c & 1)


def default_out_shape(in_shape, scale):
    return int(math.ceil(in_shape[0] * float(scale))), int(math.ceil(in_shape[1] * float(scale)))


def compose(affines, scale, n):
    """float64 [n, 6]: output pixel (u, v) of the grid with `scale` pixels per reference pixel -> input coordinates; output pixel
    (u, v) sits at reference coordinate ((u + 0.5) / s - 0.5, (v + 0.5) / s - 0.5)."""
    s = float(scale)
    a = np.array(affines, dtype=np.float64).reshape(-1, 6)
    if a.shape[0] == 1 and n > 1:
        a = np.repeat(a, n, 0)
    if a.shape[0] != n:
        raise ValueError('affines must hold one 2x3 transform per frame')
    off = 0.5 / s - 0.5
    fine = a.copy()
    fine[:, 0] = a[:, 0] / s
    fine[:, 1] = a[:, 1] / s
    fine[:, 2] = a[:, 2] + (a[:, 0] + a[:, 1]) * off
    fine[:, 3] = a[:, 3] / s
    fine[:, 4] = a[:, 4] / s
    fine[:, 5] = a[:, 5] + (a[:, 3] + a[:, 4]) * off
    return fine


def frame_params(affines, scale, n, fscale=None, weights=None, conserve_flux=False):
    """float64 [n, 10]: A0 .. A5, hx, hy, w, g - what the kernel reads per frame.  ValueError as ops.drizzle raises it."""
    if not (isinstance(scale, (int, float, np.floating, np.integer)) and math.isfinite(float(scale)) and float(scale) > 0.0):
        raise ValueError('scale must be a positive number, got %r' % (scale,))
    A = compose(affines, scale, n)
    if not np.all(np.isfinite(A)):
        raise ValueError('the transforms must be finite')
    hx = 0.5 * np.hypot(A[:, 0], A[:, 3])
    hy = 0.5 * np.hypot(A[:, 1], A[:, 4])
    lx, ly = 2.0 * hx, 2.0 * hy
    if not (np.all(lx > 0.0) and np.all(lx <= 2.0) and np.all(ly > 0.0) and np.all(ly <= 2.0)):
        raise ValueError('the footprint of an output pixel must be within (0, 2] input pixels per axis, got %s x %s: '
                         'use a larger scale' % (lx.tolist(), ly.tolist()))
    fs = np.ones(n, F) if fscale is None else np.broadcast_to(np.asarray(fscale, np.float64).reshape(-1), (n,)).astype(F)
    if not np.all(np.isfinite(fs)):
        raise ValueError('fscale must be finite')
    w = np.ones(n, F) if weights is None else np.asarray(weights, np.float64).reshape(-1).astype(F)
    if w.size != n:
        raise ValueError('weights must hold one value per frame')
    if not (np.all(np.isfinite(w)) and np.all(w > 0)):
        raise ValueError('weights must be finite and positive')
    g = fs
    if conserve_flux:
        det = np.abs(A[:, 0] * A[:, 4] - A[:, 1] * A[:, 3])
        g = (fs.astype(np.float64) * det).astype(F)
    if not np.all(np.isfinite(g)):
        raise ValueError('the flux factors overflow float32')
    return np.concatenate([A, hx[:, None], hy[:, None], w.astype(np.float64)[:, None], g.astype(np.float64)[:, None]], 1)


def _check_pixfrac(pixfrac):
    p = F(pixfrac)
    if not (p > 0 and p <= 1):
        raise ValueError('pixfrac must be in (0, 1], got %r' % (pixfrac,))
    return p


def _overlaps(l0, l1, hp):
    """[4] arrays: the overlap of [l0, l1] with the drop t - hp .. t + hp, float32."""
    out = []
    for t in range(4):
        lo = np.maximum(l0, F(t) - hp)
        hi = np.minimum(l1, F(t) + hp)
        out.append(np.maximum(F(0), hi - lo))
    return out


def cfa_accept(cfa):
    """cfa = (pattern, channel) -> bool [2, 2]: cell position (j & 1, i & 1) feeds the plane; None: all."""
    if cfa is None:
        return np.ones((2, 2), bool)
    pattern, channel = cfa
    pat = [int(x) for x in pattern]
    if sorted(pat) != [0, 1, 2, 3] or int(channel) not in (0, 1, 2):
        raise ValueError('cfa must be (a permutation of 0 .. 3, a channel 0 .. 2), got %r' % (cfa,))
    return np.array([(1 if c == 3 else c) == int(channel) for c in pat]).reshape(2, 2)


def drizzle(frames, affines, scale=2.0, pixfrac=0.5, fscale=None, weights=None, mask=None, frame_masks=None, out_shape=None,
            conserve_flux=False, cfa=None):
    """frames [N, H, W] float32 -> dict(image, weight), float32 [h, w]; the arguments of ops.drizzle."""
    frames = np.asarray(frames, F)
    if frames.ndim == 2:
        frames = frames[None]
    N, H, W = frames.shape
    p = _check_pixfrac(pixfrac)
    prm = frame_params(affines, scale, N, fscale, weights, conserve_flux)
    if mask is not None and tuple(np.shape(mask)) != (H, W):
        raise ValueError('mask must be [H,W]')
    if frame_masks is not None and tuple(np.shape(frame_masks)) != (N, H, W):
        raise ValueError('frame_masks must be [N,H,W]')
    accept = cfa_accept(cfa)
    h, w = default_out_shape((H, W), scale) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
    hp = F(0.5) * p
    hp64 = np.float64(hp)
    q = F(1.0 / (np.float64(p) * np.float64(p)))
    u = np.arange(w, dtype=np.float64)[None, :]
    v = np.arange(h, dtype=np.float64)[:, None]
    num = np.zeros((h, w), np.float64)
    den = np.zeros((h, w), np.float64)
    bad = None if mask is None else (np.asarray(mask) != 0)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        for f in range(N):
            A = prm[f]
            hx, hy, wf, g = A[6], A[7], F(A[8]), F(A[9])
            xc = (A[0] * u + A[1] * v) + A[2]
            yc = (A[3] * u + A[4] * v) + A[5]
            x0, y0 = xc - hx, yc - hy
            i0d, j0d = np.ceil(x0 - hp64), np.ceil(y0 - hp64)
            on = (i0d >= -3.0) & (i0d <= W - 1) & (j0d >= -3.0) & (j0d <= H - 1)
            if not on.any():
                continue
            i0d, j0d = np.where(on, i0d, 0.0), np.where(on, j0d, 0.0)
            ox = _overlaps((x0 - i0d).astype(F), ((xc + hx) - i0d).astype(F), hp)
            oy = _overlaps((y0 - j0d).astype(F), ((yc + hy) - j0d).astype(F), hp)
            i0, j0 = i0d.astype(np.int64), j0d.astype(np.int64)
            fbad = None if frame_masks is None else (np.asarray(frame_masks[f]) != 0)
            for tj in range(4):
                j = j0 + tj
                for ti in range(4):
                    i = i0 + ti
                    a = (ox[ti] * oy[tj]) * q
                    ok = on & (a != 0) & (i >= 0) & (i < W) & (j >= 0) & (j < H)
                    jj, ii = np.clip(j, 0, H - 1), np.clip(i, 0, W - 1)
                    ok &= accept[jj & 1, ii & 1]
                    if bad is not None:
                        ok &= ~bad[jj, ii]
                    if fbad is not None:
                        ok &= ~fbad[jj, ii]
                    val = frames[f][jj, ii]
                    ok &= np.isfinite(val)
                    aw = (a * wf).astype(np.float64)
                    gv = (g * val).astype(np.float64)
                    den = np.where(ok, den + aw, den)
                    num = np.where(ok, num + aw * gv, num)
        image = np.where(den == 0.0, np.float64(np.nan), num / np.where(den == 0.0, 1.0, den)).astype(F)
    image[den == 0.0] = NAN
    return dict(image=image, weight=den.astype(F))


def invert(affines):
    """float64 [n, 6]: the inverses of 2x3 transforms."""
    a = np.array(affines, dtype=np.float64).reshape(-1, 6)
    det = a[:, 0] * a[:, 4] - a[:, 1] * a[:, 3]
    if not np.all(np.isfinite(det)) or np.any(det == 0.0):
        raise ValueError('a transform is singular')
    inv = np.empty_like(a)
    inv[:, 0], inv[:, 1] = a[:, 4] / det, -a[:, 1] / det
    inv[:, 3], inv[:, 4] = -a[:, 3] / det, a[:, 0] / det
    inv[:, 2] = -(inv[:, 0] * a[:, 2] + inv[:, 1] * a[:, 5])
    inv[:, 5] = -(inv[:, 3] * a[:, 2] + inv[:, 4] * a[:, 5])
    return inv


def reject_params(affines, ref_scale, n, fscale=None, sigmas=None):
    """float64 [n, 8]: B0 .. B5 (input pixel -> pixel of a reference image with `ref_scale` pixels per reference pixel), g, sigma."""
    rs = float(ref_scale)
    if not (math.isfinite(rs) and rs > 0.0):
        raise ValueError('ref_scale must be a positive number, got %r' % (ref_scale,))
    a = np.array(affines, dtype=np.float64).reshape(-1, 6)
    if a.shape[0] == 1 and n > 1:
        a = np.repeat(a, n, 0)
    if a.shape[0] != n:
        raise ValueError('affines must hold one 2x3 transform per frame')
    inv = invert(a)
    off = 0.5 * rs - 0.5                                       # reference coordinate x -> pixel (x + 0.5) rs - 0.5
    B = inv * rs
    B[:, 2] += off
    B[:, 5] += off
    fs = np.ones(n, F) if fscale is None else np.broadcast_to(np.asarray(fscale, np.float64).reshape(-1), (n,)).astype(F)
    sg = np.zeros(n, F) if sigmas is None else np.broadcast_to(np.asarray(sigmas, np.float64).reshape(-1), (n,)).astype(F)
    if not (np.all(np.isfinite(fs)) and np.all(np.isfinite(sg)) and np.all(sg >= 0)):
        raise ValueError('fscale must be finite and sigmas finite and >= 0')
    return np.concatenate([B, fs.astype(np.float64)[:, None], sg.astype(np.float64)[:, None]], 1)


def drizzle_reject(frames, affines, ref, ref_scale=1.0, fscale=None, sigmas=None, k=3.5, grow=1.2):
    """uint8 [N, H, W]: 1 where a pixel differs from the bilinear value of `ref` under it by more than k sigma_i + grow d."""
    frames = np.asarray(frames, F)
    if frames.ndim == 2:
        frames = frames[None]
    ref = np.asarray(ref, F)
    N, H, W = frames.shape
    hr, wr = ref.shape
    k, grow = F(k), F(grow)
    if not (np.isfinite(k) and np.isfinite(grow) and k >= 0 and grow >= 0):
        raise ValueError('k and grow must be finite and >= 0')
    prm = reject_params(affines, ref_scale, N, fscale, sigmas)
    c = np.arange(W, dtype=np.float64)[None, :]
    r = np.arange(H, dtype=np.float64)[:, None]
    out = np.zeros((N, H, W), np.uint8)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        for f in range(N):
            B = prm[f]
            g, sigma = F(B[6]), F(B[7])
            xr = (B[0] * c + B[1] * r) + B[2]
            yr = (B[3] * c + B[4] * r) + B[5]
            X, Y = np.floor(xr), np.floor(yr)
            inside = (X >= 0.0) & (X <= wr - 2) & (Y >= 0.0) & (Y <= hr - 2)
            if not inside.any():
                continue
            X, Y = np.where(inside, X, 0.0), np.where(inside, Y, 0.0)
            fx, fy = (xr - X).astype(F), (yr - Y).astype(F)
            xi, yi = X.astype(np.int64), Y.astype(np.int64)
            x1, y1 = np.minimum(xi + 1, wr - 1), np.minimum(yi + 1, hr - 1)
            p00, p01, p10, p11 = ref[yi, xi], ref[yi, x1], ref[y1, xi], ref[y1, x1]
            val = frames[f]
            fin = inside & np.isfinite(p00) & np.isfinite(p01) & np.isfinite(p10) & np.isfinite(p11) & np.isfinite(val)
            top = p00 + fx * (p01 - p00)
            bot = p10 + fx * (p11 - p10)
            b = top + fy * (bot - top)
            d = np.maximum(np.maximum(p00, p01), np.maximum(p10, p11)) - np.minimum(np.minimum(p00, p01), np.minimum(p10, p11))
            out[f] = (fin & (np.abs(g * val - b) > k * sigma + grow * d)).astype(np.uint8)
    return out


# ---- synthetic truth -----------------------------------------------------------------------------------------------------------
def shift_affine(dx, dy, theta_deg=0.0, mag=1.0):
    """The 2x3 transform reference pixel -> input pixel of a frame whose content is the reference's moved by (dx, dy), rotated by
    theta about the origin and magnified: xin = mag (cos x - sin y) + dx, yin = mag (sin x + cos y) + dy."""
    t = math.radians(theta_deg)
    return [mag * math.cos(t), -mag * math.sin(t), dx, mag * math.sin(t), mag * math.cos(t), dy]


def lattice(n=4):
    """The exact n x n lattice of 1/n-pixel dithers, as (dx, dy) pairs."""
    return [(i / n, j / n) for j in range(n) for i in range(n)]


def star_frame(shape, stars, sigma0, dx=0.0, dy=0.0):
    """Gaussian stars (x, y, flux) of width sigma0 in reference coordinates, seen by a frame shifted by (dx, dy) and integrated over
    its pixels analytically: float64 [H, W]."""
    from math import erf
    H, W = shape
    verf = np.vectorize(erf)
    xe = np.arange(W + 1, dtype=np.float64) - 0.5
    ye = np.arange(H + 1, dtype=np.float64) - 0.5
    img = np.zeros((H, W))
    rt = sigma0 * math.sqrt(2.0)
    for x, y, flux in stars:
        cx = 0.5 * verf((xe - (x + dx)) / rt)
        cy = 0.5 * verf((ye - (y + dy)) / rt)
        img += flux * np.outer(np.diff(cy), np.diff(cx))
    return img


STARS = [(12.3, 11.6, 4000.0), (30.55, 14.2, 2500.0), (21.8, 29.45, 6000.0), (37.1, 35.7, 1500.0)]


def scene(shape=(48, 52), sigma0=0.5, noise=0.0, sky=0.0, seed=3, dithers=None):
    """The star scene of the host and end-to-end tests: 16 frames on the quarter-pixel lattice (plus whole-pixel offsets that keep
    the lattice but move the stars about the detector), float32, with their transforms."""
    dithers = lattice(4) if dithers is None else dithers
    rng = np.random.default_rng(seed)
    whole = [((3 * k) % 5 - 2, (2 * k) % 3 - 1) for k in range(len(dithers))]
    shifts = [(dx + ox, dy + oy) for (dx, dy), (ox, oy) in zip(dithers, whole)]
    frames = np.stack([star_frame(shape, STARS, sigma0, dx, dy) + sky for dx, dy in shifts])
    if noise:
        frames = frames + rng.normal(0.0, noise, frames.shape)
    return dict(frames=frames.astype(F), affines=np.array([shift_affine(dx, dy) for dx, dy in shifts]), shifts=shifts, stars=STARS,
                sigma0=sigma0, noise=noise, sky=sky)


def star_variance(image, scale, x, y, half=4.0):
    """Second-moment variance per axis, in input pixels^2, of the star at reference (x, y) in an image drizzled at `scale`, over a
    stamp of +- half input pixels; the centroid is measured, not assumed."""
    s = float(scale)
    h, w = image.shape
    uc, vc = (x + 0.5) * s - 0.5, (y + 0.5) * s - 0.5
    r = int(round(half * s))
    u0, v0 = int(round(uc)), int(round(vc))
    st = np.nan_to_num(image[v0 - r:v0 + r + 1, u0 - r:u0 + r + 1].astype(np.float64))
    uu = (np.arange(u0 - r, u0 + r + 1) + 0.5) / s - 0.5
    vv = (np.arange(v0 - r, v0 + r + 1) + 0.5) / s - 0.5
    tot = st.sum()
    mx, my = (st.sum(0) * uu).sum() / tot, (st.sum(1) * vv).sum() / tot
    return (st.sum(0) * (uu - mx) ** 2).sum() / tot, (st.sum(1) * (vv - my) ** 2).sum() / tot
