"""NumPy restatement of F19, lens distortion as a polynomial map per frame (csrc/distortion_core.h, csrc/distortion.hip, the polynomial
instance of csrc/register.hip's neighbour search, the per-tile instances of csrc/drizzle.hip; DESIGN 4.3e').

PARITY UNPINNED: nothing in the reference does this; the rule is the project's own and the truth a planted map.  Every expression
below rounds where the kernels round (float64, no fused operation), so the GPU tests ask for bit equality.
"""
import numpy as np

import drizzle_model as drm
import register_model as rm


# -- the map -----------------------------------------------------------------------------------------------------------------
def ncoef(d):
    return (d + 1) * (d + 2) // 2


def exponents(d):
    """[(i, j)]: the powers of u and v of coefficient k - by total degree t, within t by j = 0 .. t, i = t - j."""
    return [(t - j, j) for t in range(d + 1) for j in range(t + 1)]


def degree_of(c):
    n = np.asarray(c).shape[-1]
    d = [d for d in range(1, 6) if ncoef(d) == n]
    assert d, 'not a coefficient count of degree 1 .. 5: %d' % n
    return d[0]


def _powers(u, d):
    p = [np.ones_like(u)]
    for _ in range(d):
        p.append(p[-1] * u)                                              # repeated multiplication
    return p


def _uv(x, y, x0, y0, L, d):
    x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
    return _powers((x - x0) / L, d), _powers((y - y0) / L, d)


def _plain(c, up, vp, d):
    s = np.zeros_like(up[0])                                             # from +0, in coefficient order
    for k, (i, j) in enumerate(exponents(d)):
        s = s + c[k] * (up[i] * vp[j])
    return s


def _du(c, up, vp, d):
    s = np.zeros_like(up[0])
    for k, (i, j) in enumerate(exponents(d)):
        if i >= 1:
            s = s + (np.float64(i) * c[k]) * (up[i - 1] * vp[j])
    return s


def _dv(c, up, vp, d):
    s = np.zeros_like(up[0])
    for k, (i, j) in enumerate(exponents(d)):
        if j >= 1:
            s = s + (np.float64(j) * c[k]) * (up[i] * vp[j - 1])
    return s


def evaluate(c, x0, y0, L, x, y):
    """c [2, ncoef] -> (X, Y)."""
    d = degree_of(c)
    up, vp = _uv(x, y, x0, y0, L, d)
    return _plain(c[0], up, vp, d), _plain(c[1], up, vp, d)


def jacobian(c, x0, y0, L, x, y):
    """-> (dX/dx, dX/dy, dY/dx, dY/dy)."""
    d = degree_of(c)
    up, vp = _uv(x, y, x0, y0, L, d)
    return _du(c[0], up, vp, d) / L, _dv(c[0], up, vp, d) / L, _du(c[1], up, vp, d) / L, _dv(c[1], up, vp, d) / L


def from_affine(A, d, x0, y0, L):
    A = np.asarray(A, np.float64)
    c = np.zeros((2, ncoef(d)))
    c[0, :3] = (A[0] * x0 + A[1] * y0) + A[2], A[0] * L, A[1] * L
    c[1, :3] = (A[3] * x0 + A[4] * y0) + A[5], A[3] * L, A[4] * L
    return c


def affine_part(c, x0, y0, L):
    a0, a1, a3, a4 = c[0, 1] / L, c[0, 2] / L, c[1, 1] / L, c[1, 2] / L
    return np.array([a0, a1, c[0, 0] - (a0 * x0 + a1 * y0), a3, a4, c[1, 0] - (a3 * x0 + a4 * y0)])


def inverse(c, x0, y0, L, xi, yi, tol=1e-12, max_steps=20):
    """Newton from the inverse of the affine part; a step below max(tol, 8 ulp of the coordinate) ends it; NaN after max_steps."""
    xi, yi = np.broadcast_arrays(np.asarray(xi, np.float64), np.asarray(yi, np.float64))
    A = affine_part(c, x0, y0, L)
    det = A[0] * A[4] - A[1] * A[3]
    x = (A[4] * (xi - A[2]) - A[1] * (yi - A[5])) / det
    y = (A[0] * (yi - A[5]) - A[3] * (xi - A[2])) / det
    done = np.zeros(x.shape, bool)
    with np.errstate(all='ignore'):
        for _ in range(max_steps):
            X, Y = evaluate(c, x0, y0, L, x, y)
            xx, xy, yx, yy = jacobian(c, x0, y0, L, x, y)
            rx, ry = X - xi, Y - yi
            dd = xx * yy - xy * yx
            dx, dy = (yy * rx - xy * ry) / dd, (xx * ry - yx * rx) / dd
            x, y = np.where(done, x, x - dx), np.where(done, y, y - dy)
            done = done | (np.hypot(dx, dy) < np.maximum(tol, 8.0 * np.spacing(np.maximum(np.abs(x), np.abs(y)))))
            if done.all():
                break
    return np.where(done, x, np.nan), np.where(done, y, np.nan)


def design(r, d, x0, y0, L):
    up, vp = _powers((r[:, 0] - x0) / L, d), _powers((r[:, 1] - y0) / L, d)
    return np.stack([up[i] * vp[j] for i, j in exponents(d)], axis=1)


def fit(r, s, d, x0, y0, L):
    """-> (c [2, ncoef] or None, rank, 2-D rms)."""
    r, s = np.asarray(r, np.float64), np.asarray(s, np.float64)
    D = design(r, d, x0, y0, L)
    if D.shape[0] < D.shape[1]:
        return None, 0, np.nan
    cx, _, rank, _ = np.linalg.lstsq(D, s[:, 0], rcond=None)
    cy = np.linalg.lstsq(D, s[:, 1], rcond=None)[0]
    if rank < D.shape[1]:
        return None, int(rank), np.nan
    c = np.stack([cx, cy])
    X, Y = evaluate(c, x0, y0, L, r[:, 0], r[:, 1])
    return c, int(rank), float(np.sqrt(np.mean((X - s[:, 0]) ** 2 + (Y - s[:, 1]) ** 2)))


# -- tile affines ------------------------------------------------------------------------------------------------------------
def tile_centres(out_shape, tile_scale=1):
    th, tw = 16 * tile_scale, 64 * tile_scale
    ty, tx = -(-out_shape[0] // th), -(-out_shape[1] // tw)
    yc = np.arange(ty, dtype=np.float64)[:, None] * th + (th - 1.0) / 2.0 + np.zeros((1, tx))
    xc = np.arange(tx, dtype=np.float64)[None, :] * tw + (tw - 1.0) / 2.0 + np.zeros((ty, 1))
    return xc, yc


def tile_affines(coef, x0, y0, L, out_shape, tile_scale=1, scale=1.0, composed=True):
    """coef [N, 2, ncoef] -> float64 [N, tiles_y, tiles_x, 6] (apgpu_poly_tile_affines)."""
    xc, yc = tile_centres(out_shape, tile_scale)
    s = np.float64(scale)
    xr, yr = (xc + 0.5) / s - 0.5, (yc + 0.5) / s - 0.5
    out = []
    for c in np.asarray(coef, np.float64):
        X, Y = evaluate(c, x0, y0, L, xr, yr)
        J = jacobian(c, x0, y0, L, xr, yr)
        if composed:
            a0, a1, a3, a4 = J[0] / s, J[1] / s, J[2] / s, J[3] / s
            px, py = xc, yc
        else:
            a0, a1, a3, a4 = J
            px, py = xr, yr
        out.append(np.stack([a0, a1, (X - a0 * px) - a1 * py, a3, a4, (Y - a3 * px) - a4 * py], axis=-1))
    return np.stack(out)


def input_tile_affines(coef, x0, y0, L, in_shape):
    """float64 [N, ty, tx, 6]: reference pixel -> input pixel about the reference point that maps to the centre of each 16 x 64 tile of
    the INPUT frame (ops.poly_input_tile_affines)."""
    xc, yc = tile_centres(in_shape)
    out = []
    for c in np.asarray(coef, np.float64):
        px, py = inverse(c, x0, y0, L, xc, yc)
        a0, a1, a3, a4 = jacobian(c, x0, y0, L, px, py)
        out.append(np.stack([a0, a1, (xc - a0 * px) - a1 * py, a3, a4, (yc - a3 * px) - a4 * py], axis=-1))
    return np.stack(out)


# -- neighbour search and the refinement (step 7) ------------------------------------------------------------------------------
def nearest_match(xy, count, coef, x0, y0, L, radius):
    """register_model.nearest_match with T_f the polynomial of frame f: a brute-force search.  -> (fwd_idx, fwd_d2, bwd_idx, bwd_d2,
    margin)."""
    xy = np.asarray(xy, np.float64)
    F, M = xy.shape[:2]
    margin = rm.Margin()
    r2 = np.float64(radius) * np.float64(radius)
    fwd_idx, bwd_idx = np.full((F, M), -1, np.int32), np.full((F, M), -1, np.int32)
    fwd_d2, bwd_d2 = np.full((F, M), np.inf), np.full((F, M), np.inf)
    n0 = max(0, min(int(count[0]), M))
    for f in range(F):
        nf = max(0, min(int(count[f]), M))
        if n0 == 0 or nf == 0:
            continue
        px, py = evaluate(coef[f], x0, y0, L, xy[0, :n0, 0], xy[0, :n0, 1])
        s = xy[f, :nf]
        dx, dy = s[None, :, 0] - px[:, None], s[None, :, 1] - py[:, None]
        d2 = dx * dx + dy * dy
        for idx_out, d2_out, axis, n in ((fwd_idx, fwd_d2, 1, n0), (bwd_idx, bwd_d2, 0, nf)):
            best = d2.argmin(axis=axis)
            bd = np.take_along_axis(d2, np.expand_dims(best, axis), axis).squeeze(axis)
            margin.update(bd, r2)
            ok = bd <= r2
            idx_out[f, :n] = np.where(ok, best, -1)
            d2_out[f, :n] = np.where(ok, bd, np.inf)
    return fwd_idx, fwd_d2, bwd_idx, bwd_d2, margin.value


def bbox_frame(ref):
    """(x0, y0, L): the midpoint of the bounding box of the reference stars and half its diagonal."""
    lo, hi = ref.min(axis=0), ref.max(axis=0)
    return float(0.5 * (lo[0] + hi[0])), float(0.5 * (lo[1] + hi[1])), float(0.5 * np.hypot(hi[0] - lo[0], hi[1] - lo[1]))


def refine(ref, frm, A, rms, d, match_radius=3.0, max_rounds=4, frame=None):
    """Step 7 for one frame: from the affine A (rms its residual) to a polynomial of degree d.  -> dict(coef, order, rms, pairs, x0, y0,
    L, margin); order 1 and coef = the affine's when the frame keeps its affine."""
    x0, y0, L = bbox_frame(ref) if frame is None else frame
    xy, count = rm.pad_lists([ref, frm])
    c = from_affine(A, d, x0, y0, L)
    ident = from_affine(rm.IDENTITY, d, x0, y0, L)
    out = dict(coef=c, order=1, rms=rms, pairs=None, x0=x0, y0=y0, L=L, margin=np.inf)
    pairs = None
    for _ in range(max_rounds):
        radius = float(np.clip(3.0 * rms, 0.5, match_radius))
        fi, _, bi, _, mg = nearest_match(xy, count, np.stack([ident, c]), x0, y0, L, radius)
        out['margin'] = min(out['margin'], mg)
        new = rm.mutual_pairs(fi[1], bi[1])
        if pairs is not None and np.array_equal(new, pairs):
            break
        pairs = new
        cn = None
        if len(pairs) >= 3 * ncoef(d):
            cn, _, r = fit(ref[pairs[:, 0]], frm[pairs[:, 1]], d, x0, y0, L)
        if cn is None:
            return dict(out, coef=from_affine(A, d, x0, y0, L), order=1, pairs=None)
        c, rms = cn, r
        out.update(coef=c, order=d, rms=rms, pairs=pairs)
    return out


# -- drizzle with per-tile transforms -------------------------------------------------------------------------------------------
def drizzle_tiles(frames, tiles, scale=2.0, out_shape=None, **kw):
    """ops.drizzle with transforms [N, ty, tx, 6] per 16 x 64 OUTPUT tile: for each tile the per-frame model with that tile's
    transforms, of which the tile's pixels are kept."""
    frames = np.asarray(frames, np.float32)
    frames = frames[None] if frames.ndim == 2 else frames
    h, w = drm.default_out_shape(frames.shape[1:], scale) if out_shape is None else out_shape
    tiles = np.asarray(tiles, np.float64)
    assert tiles.shape == (frames.shape[0], -(-h // 16), -(-w // 64), 6)
    image, weight = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    for ty in range(tiles.shape[1]):
        for tx in range(tiles.shape[2]):
            r = drm.drizzle(frames, tiles[:, ty, tx], scale=scale, out_shape=(h, w), **kw)
            sl = (slice(16 * ty, 16 * ty + 16), slice(64 * tx, 64 * tx + 64))
            image[sl], weight[sl] = r['image'][sl], r['weight'][sl]
    return dict(image=image, weight=weight)


def drizzle_reject_tiles(frames, tiles, ref, **kw):
    """ops.drizzle_reject with transforms [N, ty, tx, 6] per 16 x 64 INPUT tile."""
    frames = np.asarray(frames, np.float32)
    frames = frames[None] if frames.ndim == 2 else frames
    N, H, W = frames.shape
    tiles = np.asarray(tiles, np.float64)
    assert tiles.shape == (N, -(-H // 16), -(-W // 64), 6)
    out = np.empty((N, H, W), np.uint8)
    for ty in range(tiles.shape[1]):
        for tx in range(tiles.shape[2]):
            r = drm.drizzle_reject(frames, tiles[:, ty, tx], ref, **kw)
            sl = (slice(None), slice(16 * ty, 16 * ty + 16), slice(64 * tx, 64 * tx + 64))
            out[sl] = r[sl]
    return out


# -- the planted scene of the issue's probe -----------------------------------------------------------------------------------
def planted_map(size=4096, rot_deg=1.2, cubic_px=3.0, quad_px=1.5, shift=(7.3, -4.1)):
    """A rotation about the centre after a cubic radial term of cubic_px at the corner and a quadratic (sensor tilt) term of quad_px at
    the corner, then a shift, as a function (x, y) -> (X, Y)."""
    cx = cy = (size - 1) / 2.0
    R = np.hypot(cx, cy)
    th = np.deg2rad(rot_deg)

    def f(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        u, v = (x - cx) / R, (y - cy) / R
        r2 = u * u + v * v
        q = np.sqrt(2.0) * quad_px                             # (tilt of the sensor: u v and v^2, together quad_px at the corner)
        du, dv = cubic_px * r2 * u + q * u * v, cubic_px * r2 * v + q * v * v
        xx, yy = x - cx + du, y - cy + dv
        return cx + np.cos(th) * xx - np.sin(th) * yy + shift[0], cy + np.sin(th) * xx + np.cos(th) * yy + shift[1]
    return f


def planted_scene(seed=20261, n=600, size=4096, sigma=0.05, **kw):
    """-> (ref [n, 2], frm [n, 2], the planted function): frm = planted(sky), and both lists carry centroid noise sigma / sqrt 2 per
    axis, so that a pair's difference has sigma per axis and a perfect map leaves a 2-D rms of sigma sqrt 2."""
    rng = np.random.default_rng(seed)
    f = planted_map(size, **kw)
    sky = rng.uniform(0.0, size - 1.0, size=(n, 2))
    X, Y = f(sky[:, 0], sky[:, 1])
    ref = sky + rng.normal(0.0, sigma / np.sqrt(2.0), size=(n, 2))
    frm = np.stack([X, Y], axis=1) + rng.normal(0.0, sigma / np.sqrt(2.0), size=(n, 2))
    return ref, frm, f
