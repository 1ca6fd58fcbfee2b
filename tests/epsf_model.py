"""The empirical PSF (F22) in float64 NumPy, operation by operation: what csrc/epsf_core.h, csrc/epsf.hip and the host
side of ops.epsf_* compute.  The expressions and their order are those of the kernels; only the order of the sums over stars and
pixels differs (sequential here, lane-strided butterflies there).

Every decision the device has to take the same way is recorded in a `Margin` (the closest call, relative as in
tests/register_model.py): the node of a sample (distance of (p - x) o + 0.5 from an integer), the clip bounds, min_count.
"""
import math

import numpy as np

REC = 8
TILE = 32


class Margin:
    def __init__(self):
        self.value = np.inf

    def update(self, lhs, rhs):
        lhs, rhs = np.broadcast_arrays(np.asarray(lhs, np.float64), np.asarray(rhs, np.float64))
        with np.errstate(all='ignore'):
            d = np.abs(lhs - rhs) / np.where(rhs != 0.0, np.abs(rhs), 1.0)
        d = d[np.isfinite(d)]
        if d.size:
            self.value = min(self.value, float(d.min()))

    def absolute(self, d):
        d = np.abs(np.asarray(d, np.float64))
        d = d[np.isfinite(d)]
        if d.size:
            self.value = min(self.value, float(d.min()))


def grid_size(o, R):
    return 2 * o * R + 1


def radius_of(E, o):
    return (E.shape[0] - 1) // (2 * o)


# ---- the interpolant (csrc/epsf_core.h) -------------------------------------------------------------------------------------------------
def keys(t):
    w = [((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * t * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * t * t]
    d = [(-1.5 * t + 2.0) * t - 0.5, (4.5 * t - 5.0) * t, (-4.5 * t + 4.0) * t + 0.5, (1.5 * t - 1.0) * t]
    return w, d


def evaluate(E, o, dx, dy, grad=False):
    """E(dx, dy) for arrays of offsets (pixels); with grad also dE/ddx, dE/ddy.  0 outside |dx|, |dy| <= R (NaN included)."""
    E = np.asarray(E)
    G = E.shape[0]
    R = radius_of(E, o)
    dx, dy = np.broadcast_arrays(np.asarray(dx, np.float64), np.asarray(dy, np.float64))
    with np.errstate(invalid='ignore'):
        inside = (np.abs(dx) <= R) & (np.abs(dy) <= R)
    sx, sy = np.where(inside, dx, 0.0), np.where(inside, dy, 0.0)
    u, v = sx * float(o) + float(o * R), sy * float(o) + float(o * R)
    fu, fv = np.floor(u), np.floor(v)
    iu, iv = fu.astype(np.int64), fv.astype(np.int64)
    wx, dwx = keys(u - fu)
    wy, dwy = keys(v - fv)
    xi = [np.clip(iu - 1 + b, 0, G - 1) for b in range(4)]
    row, drow = [], []
    for a in range(4):
        yi = np.clip(iv - 1 + a, 0, G - 1)
        e = [E[yi, xi[b]].astype(np.float64) for b in range(4)]
        row.append(((wx[0] * e[0] + wx[1] * e[1]) + wx[2] * e[2]) + wx[3] * e[3])
        drow.append(((dwx[0] * e[0] + dwx[1] * e[1]) + dwx[2] * e[2]) + dwx[3] * e[3])
    val = np.where(inside, ((wy[0] * row[0] + wy[1] * row[1]) + wy[2] * row[2]) + wy[3] * row[3], 0.0)
    if not grad:
        return val
    gx = np.where(inside, (((wy[0] * drow[0] + wy[1] * drow[1]) + wy[2] * drow[2]) + wy[3] * drow[3]) * float(o), 0.0)
    gy = np.where(inside, (((dwy[0] * row[0] + dwy[1] * row[1]) + dwy[2] * row[2]) + dwy[3] * row[3]) * float(o), 0.0)
    return val, gx, gy


def star_usable(f, x, y, sky):
    with np.errstate(invalid='ignore'):
        return bool(f > 0.0 and f < np.inf and abs(sky) < np.inf and abs(x) <= 1e9 and abs(y) <= 1e9)


# ---- accumulate -------------------------------------------------------------------------------------------------------------------------
def samples(image, stars, E, o, margin=None):
    """(node index j * G + i, residual, star) of every sample, in star order: the forward form of the sample -> node rule."""
    margin = margin if margin is not None else Margin()
    image = np.asarray(image)
    H, W = image.shape
    G = E.shape[0]
    R = radius_of(E, o)
    half = o * R
    nodes, res, who = [], [], []
    for s, (f, x, y, sky) in enumerate(np.asarray(stars, np.float64).reshape(-1, 4)):
        if not star_usable(f, x, y, sky):
            continue
        px = np.arange(max(int(math.floor(x - R - 2)), 0), min(int(math.ceil(x + R + 2)), W - 1) + 1, dtype=np.int64)
        py = np.arange(max(int(math.floor(y - R - 2)), 0), min(int(math.ceil(y + R + 2)), H - 1) + 1, dtype=np.int64)
        if px.size == 0 or py.size == 0:
            continue
        ax, ay = (px.astype(np.float64) - x) * float(o) + 0.5, (py.astype(np.float64) - y) * float(o) + 0.5
        kx, ky = np.floor(ax) + half, np.floor(ay) + half
        okx, oky = (kx >= 0) & (kx <= G - 1), (ky >= 0) & (ky <= G - 1)
        margin.absolute((ax - np.rint(ax))[(kx >= -1) & (kx <= G)])               # every pixel that could fall into a node or just past
        margin.absolute((ay - np.rint(ay))[(ky >= -1) & (ky <= G)])
        px, kx, py, ky = px[okx], kx[okx].astype(np.int64), py[oky], ky[oky].astype(np.int64)
        if px.size == 0 or py.size == 0:
            continue
        PY, PX = np.meshgrid(py, px, indexing='ij')
        KY, KX = np.meshgrid(ky, kx, indexing='ij')
        d = image[PY, PX].astype(np.float64)
        with np.errstate(all='ignore'):
            r = (d - sky) / f - evaluate(E, o, PX.astype(np.float64) - x, PY.astype(np.float64) - y)
        ok = np.isfinite(d) & np.isfinite(r)
        nodes.append((KY * G + KX)[ok])
        res.append(r[ok])
        who.append(np.full(int(ok.sum()), s, np.int64))
    if not nodes:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64)
    return np.concatenate(nodes), np.concatenate(res), np.concatenate(who)


def accumulate(image, stars, E, o, sigma=2.5, maxiters=5, margin=None):
    """(mean float64 [G, G], count int32 [G, G], kept: bool per sample, (node, residual, star) of the samples, sum |r| of the kept
    per node)."""
    margin = margin if margin is not None else Margin()
    G = E.shape[0]
    node, r, who = samples(image, stars, E, o, margin)
    N = G * G
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    mean, kept_n, prev = np.zeros(N), np.zeros(N), np.full(N, -1.0)
    live = np.ones(N, bool)                                                      # nodes whose clip has not ended
    kept = np.ones(r.size, bool)
    for rnd in range(maxiters + 1):
        inside = (r >= lo[node]) & (r <= hi[node])
        kept = np.where(live[node], inside, kept)
        c = np.bincount(node[kept], minlength=N).astype(np.float64)
        s1 = np.bincount(node[kept], weights=r[kept], minlength=N)
        ended = live & (c == prev)
        live = live & ~ended
        kept_n = np.where(live, c, kept_n)
        empty = live & (c == 0.0)
        mean = np.where(empty, 0.0, mean)
        live = live & ~empty
        with np.errstate(all='ignore'):
            mean = np.where(live, s1 / c, mean)
        if rnd == maxiters or not live.any():
            break
        dev = r - mean[node]
        s2 = np.bincount(node[kept], weights=(dev * dev)[kept], minlength=N)
        with np.errstate(all='ignore'):
            sd = np.sqrt(s2 / c)
        lo = np.where(live, mean - sigma * sd, lo)
        hi = np.where(live, mean + sigma * sd, hi)
        prev = np.where(live, c, prev)
        # the next round tests every sample of these nodes against these bounds.  Bounds from one or two samples are left out: their
        # sums have one order only, so the device holds the same bits (a single sample sits exactly on both of its bounds)
        near = (live & (c > 2.0))[node]
        margin.update(r[near], lo[node][near])
        margin.update(r[near], hi[node][near])
    sabs = np.bincount(node[kept], weights=np.abs(r[kept]), minlength=N)
    return (mean.reshape(G, G), kept_n.astype(np.int32).reshape(G, G), kept, (node, r, who), sabs.reshape(G, G))


# ---- update -----------------------------------------------------------------------------------------------------------------------------
def smoothing_taps(kind='quartic'):
    deg = {'quartic': 4, 'quadratic': 2, 'none': None}[kind]
    taps = np.zeros((5, 5))
    if deg is None:
        taps[2, 2] = 1.0
        return taps
    yy, xx = np.mgrid[-2:3, -2:3].astype(np.float64)
    A = np.stack([xx.ravel() ** a * yy.ravel() ** b for a in range(deg + 1) for b in range(deg + 1 - a)], axis=1)
    coef = np.linalg.lstsq(A, np.eye(25), rcond=None)[0]                        # the fit's coefficients for every unit neighbourhood
    return coef[0].reshape(5, 5)


def add_smooth(E, mean, count, taps, min_count=1, margin=None):
    """float64 [G, G]: the smoothed E + mean (before the rounding to float32)."""
    margin = margin if margin is not None else Margin()
    G = E.shape[0]
    margin.absolute(np.asarray(count, np.float64) - (min_count - 0.5))           # (integers: never below 0.5)
    T = np.where(count >= min_count, E.astype(np.float64) + mean, E.astype(np.float64))
    idx = np.arange(G)
    acc = np.zeros((G, G))
    for a in range(5):
        jj = np.clip(idx + a - 2, 0, G - 1)
        for b in range(5):
            ii = np.clip(idx + b - 2, 0, G - 1)
            acc = acc + taps[a, b] * T[np.ix_(jj, ii)]
    return acc


def shift(E, o, dx, dy, scale=1.0):
    """float64 [G, G]: E(u + (dx, dy)) scale at the nodes u (before the rounding to float32)."""
    G = E.shape[0]
    half = (G - 1) // 2
    off = (np.arange(G) - half).astype(np.float64) / float(o)
    return evaluate(E, o, off[None, :] + dx, off[:, None] + dy) * scale


def centroid(E, o, r_fit=None):
    E = np.asarray(E, np.float64)
    G = E.shape[0]
    off = (np.arange(G) - (G - 1) // 2) / float(o)
    w = np.maximum(E, 0.0)
    if r_fit is not None:
        w = np.where(off[:, None] ** 2 + off[None, :] ** 2 <= float(r_fit) ** 2, w, 0.0)
    tot = w.sum()
    if not (tot > 0 and np.isfinite(tot)):
        return 0.0, 0.0
    return float((w.sum(axis=0) * off).sum() / tot), float((w.sum(axis=1) * off).sum() / tot)


def update(E, mean, count, o, taps, min_count=1, r_fit=None, recentre=True, normalise=True, margin=None):
    """(the new float32 grid, (dx, dy)): add + smooth, recentre, normalise, each step rounded to float32 as the kernels store it."""
    out = add_smooth(E, mean, count, taps, min_count, margin).astype(np.float32)
    delta = (0.0, 0.0)
    if recentre:
        delta = centroid(out, o, r_fit)
        if math.hypot(*delta) >= 1e-6:
            out = shift(out, o, delta[0], delta[1]).astype(np.float32)
    if normalise:
        tot = float(out.astype(np.float64).sum()) / (o * o)
        if tot > 0 and math.isfinite(tot):
            out = shift(out, o, 0.0, 0.0, 1.0 / tot).astype(np.float32)
    return out, delta


# ---- fit --------------------------------------------------------------------------------------------------------------------------------
def _fit_pass(E, o, px, py, d, p, nf, rn2, inv_gain, pw=None):
    """J^T W J, J^T W r, chi^2 at p; pw: the weights are those of the model at pw (frozen over a trial step)."""
    e, ex, ey = evaluate(E, o, px - p[1], py - p[2], grad=True)
    m = p[0] * e + p[3]
    mw = m if pw is None else pw[0] * evaluate(E, o, px - pw[1], py - pw[2]) + pw[3]
    w = 1.0 / (rn2 + np.maximum(mw, 0.0) * inv_gain)
    r = m - d
    J = [e, -(p[0] * ex), -(p[0] * ey), np.ones_like(e)][:nf]
    JtJ = np.array([[np.sum((w * J[i]) * J[j]) for j in range(nf)] for i in range(nf)])
    Jtr = np.array([np.sum((w * J[i]) * r) for i in range(nf)])
    return JtJ, Jtr, float(np.sum(w * (r * r)))


def _fit_run(E, o, px, py, d, p, nf, rn2, inv_gain, max_iter):
    """The damped Gauss-Newton of epsf.hip's fit_run: (ok, p, chi2, iterations)."""
    with np.errstate(all='ignore'):
        JtJ, Jtr, chi2 = _fit_pass(E, o, px, py, d, p, nf, rn2, inv_gain)
        iters = 0
        if not chi2 < 1e300:
            return False, p, chi2, iters
        lam, nu = 1e-3, 2.0
        for it in range(1, max_iter + 1):
            iters = it
            diag = np.diag(JtJ)
            if not np.all((diag > 0.0) & (diag < 1e300)):
                return False, p, chi2, iters
            D = np.sqrt(diag)
            M = JtJ / np.outer(D, D)
            M[np.diag_indices(nf)] = 1.0 + lam
            try:
                L = np.linalg.cholesky(M)
                chol_ok = bool(np.all(np.isfinite(L)))
            except np.linalg.LinAlgError:
                chol_ok = False
            if not chol_ok:
                lam *= nu
                nu *= 2.0
                if lam > 1e30:
                    return False, p, chi2, iters
                continue
            gs = Jtr / D
            u = np.linalg.solve(L.T, np.linalg.solve(L, -gs))
            step = u / D
            pt = p.copy()
            pt[:nf] = p[:nf] + step
            small = lam <= 1.0 and abs(step[1]) < 1e-7 and abs(step[2]) < 1e-7 and abs(step[0]) <= 1e-9 * abs(p[0])
            JtJt, Jtrt, chi2t = _fit_pass(E, o, px, py, d, pt, nf, rn2, inv_gain, p if inv_gain != 0.0 else None)
            if chi2t <= chi2 * (1.0 + 1e-14):
                p, JtJ, Jtr = pt, JtJt, Jtrt
                pred = float(np.sum(u * (lam * u - gs)))
                rho = (chi2 - chi2t) / pred if pred > 1e-12 * chi2 else 1.0
                t = 2.0 * rho - 1.0
                chi2 = chi2t
                lam = max(lam * max(1.0 / 3.0, 1.0 - t * t * t), 1e-15)
                nu = 2.0
                if inv_gain != 0.0:                                      # the accepted point's sums with its own weights
                    JtJ, Jtr, chi2 = _fit_pass(E, o, px, py, d, p, nf, rn2, inv_gain)
                    if not chi2 < 1e300:
                        return False, p, chi2, iters
            else:
                lam *= nu
                nu *= 2.0
                if lam > 1e30:
                    return False, p, chi2, iters
            if small:
                break
    return True, p, chi2, iters


def fit(image, init, E, o, r_fit, fit_sky=False, gain=0.0, readnoise=0.0, max_iter=50, prev=None):
    """The records float64 [n, 8] = f, x, y, sky, chi^2, pixels used, iterations, ok."""
    image = np.asarray(image)
    H, W = image.shape
    init = np.asarray(init, np.float64).reshape(-1, 4)
    rec = np.zeros((len(init), REC))
    half = int(math.floor(r_fit))
    rn2, inv_gain = (readnoise * readnoise, 1.0 / gain) if gain > 0 else (1.0, 0.0)
    for s, p0 in enumerate(init):
        ok = bool(np.all(np.isfinite(p0))) and abs(p0[1]) <= 1e9 and abs(p0[2]) <= 1e9
        if prev is not None:
            q = np.asarray(prev, np.float64).reshape(-1, 3)[s]
            ok = ok and bool(np.all(np.isfinite(q))) and abs(q[1]) <= 1e9 and abs(q[2]) <= 1e9
        cnt, iters, chi2, p = 0, 0, np.nan, p0.copy()
        if ok:
            cx, cy = int(np.rint(p0[1])), int(np.rint(p0[2]))
            yy, xx = np.mgrid[-half:half + 1, -half:half + 1]
            sel = (xx.astype(np.float64) ** 2 + yy.astype(np.float64) ** 2 <= r_fit * r_fit)
            px, py = (cx + xx)[sel], (cy + yy)[sel]
            inimg = (px >= 0) & (px < W) & (py >= 0) & (py < H)
            px, py = px[inimg], py[inimg]
            d = image[py, px].astype(np.float64)
            px, py = px.astype(np.float64), py.astype(np.float64)
            if prev is not None:
                with np.errstate(all='ignore'):
                    d = d + q[0] * evaluate(E, o, px - q[1], py - q[2])
            use = np.isfinite(d)
            px, py, d = px[use], py[use], d[use]
            cnt = int(d.size)
            ok = cnt >= 6
            if ok:
                ok, p, chi2, iters = _fit_run(E, o, px, py, d, p0.copy(), 4 if fit_sky else 3, rn2, inv_gain, max_iter)
                ok = ok and bool(np.all(np.isfinite(p))) and bool(chi2 < np.inf)
        rec[s] = list(p if ok else p0) + [chi2 if ok else np.nan, cnt, iters, 1.0 if ok else 0.0]
    return rec


# ---- render -----------------------------------------------------------------------------------------------------------------------------
def tile_lists(x, y, R, shape):
    """(offsets [tiles + 1], stars): the CSR lists of ops.epsf_tile_lists, by a search over the tiles."""
    H, W = shape
    ty, tx = -(-H // TILE), -(-W // TILE)
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    offsets, stars = [0], []
    for b in range(ty):
        for a in range(tx):
            x0, x1, y0, y1 = a * TILE, min(a * TILE + TILE, W) - 1, b * TILE, min(b * TILE + TILE, H) - 1
            for s in range(x.size):
                if np.isfinite(x[s]) and np.isfinite(y[s]) and math.ceil(x[s] - R) <= x1 and math.floor(x[s] + R) >= x0 \
                        and math.ceil(y[s] - R) <= y1 and math.floor(y[s] + R) >= y0:
                    stars.append(s)
            offsets.append(len(stars))
    return np.asarray(offsets, np.int32), np.asarray(stars, np.int32)


def render(image, stars, E, o, shape=None):
    """(model float64 [H, W], sum |f E| float64, residual float64 or None): every star's stamp summed in star order."""
    H, W = shape if image is None else np.asarray(image).shape
    R = radius_of(E, o)
    model, mabs = np.zeros((H, W)), np.zeros((H, W))
    for f, x, y in np.asarray(stars, np.float64).reshape(-1, 3):
        if not (np.isfinite(f) and np.isfinite(x) and np.isfinite(y)) or x + R < 0 or x - R > W - 1 or y + R < 0 or y - R > H - 1:
            continue
        x0, x1 = max(int(math.ceil(x - R)), 0), min(int(math.floor(x + R)), W - 1)
        y0, y1 = max(int(math.ceil(y - R)), 0), min(int(math.floor(y + R)), H - 1)
        if x1 < x0 or y1 < y0:
            continue
        px, py = np.arange(x0, x1 + 1, dtype=np.float64), np.arange(y0, y1 + 1, dtype=np.float64)
        v = f * evaluate(E, o, px[None, :] - x, py[:, None] - y)
        model[y0:y1 + 1, x0:x1 + 1] = model[y0:y1 + 1, x0:x1 + 1] + v
        mabs[y0:y1 + 1, x0:x1 + 1] += np.abs(v)
    resid = None if image is None else np.asarray(image).astype(np.float64) - model
    return model, mabs, resid


# ---- build ------------------------------------------------------------------------------------------------------------------------------
def select_stars(x, y, flux, shape, R, r_fit, psbl_sat=None, max_stars=500):
    H, W = shape
    x, y, flux = (np.asarray(v, np.float64).reshape(-1) for v in (x, y, flux))
    sat = np.zeros(x.size, bool) if psbl_sat is None else np.asarray(psbl_sat).astype(bool)
    keep = []
    for s in range(x.size):
        if sat[s] or not (np.isfinite(x[s]) and np.isfinite(y[s]) and np.isfinite(flux[s]) and flux[s] > 0):
            continue
        if not (R + 2 <= x[s] <= W - 1 - (R + 2) and R + 2 <= y[s] <= H - 1 - (R + 2)):
            continue
        with np.errstate(invalid='ignore'):
            d2 = (x - x[s]) ** 2 + (y - y[s]) ** 2
        if np.count_nonzero(d2 < float(R + r_fit) ** 2) <= 1:
            keep.append(s)
    keep = np.asarray(keep, np.int64)
    return keep[np.argsort(-flux[keep], kind='stable')][:max_stars]


def build(image, x, y, flux, sky, o=4, R=12, r_fit=None, psbl_sat=None, max_stars=500, n_iter=8, tol=1e-4, sigma=2.5, maxiters=5,
          smoothing='quartic', min_count=1, fit_sky=False, gain=0.0, readnoise=0.0, max_iter=50, margin=None):
    """ops.epsf_build on the host: dict(epsf float32 [G, G], index, stars [n, 8], change, count, niter, margin)."""
    margin = margin if margin is not None else Margin()
    image = np.asarray(image)
    G = grid_size(o, R)
    r_fit = 2.0 if r_fit is None else float(r_fit)
    x, y, flux = (np.asarray(v, np.float64).reshape(-1) for v in (x, y, flux))
    sky = np.broadcast_to(np.asarray(sky, np.float64).reshape(-1), x.shape)
    index = select_stars(x, y, flux, image.shape, R, r_fit, psbl_sat, max_stars)
    cur = np.stack([flux[index], x[index], y[index], sky[index]], axis=1) if index.size else np.zeros((0, 4))
    taps = smoothing_taps(smoothing)
    E = np.zeros((G, G), np.float32)
    rec, change, count, done = np.zeros((0, REC)), [], np.zeros((G, G), np.int32), 0
    for _ in range(n_iter if index.size else 0):
        mean, cnt = accumulate(image, cur, E, o, sigma, maxiters, margin)[:2]
        E_new, _ = update(E, mean, cnt, o, taps, min_count, r_fit, margin=margin)
        peak = float(E_new.astype(np.float64).max())
        change.append(float(np.abs(E_new.astype(np.float64) - E.astype(np.float64)).max()) / peak if peak > 0 else float('inf'))
        E, count, done = E_new, cnt, done + 1
        rec = fit(image, cur, E, o, r_fit, fit_sky, gain, readnoise, max_iter)
        cur = rec[:, :4].copy()
        if change[-1] <= tol:
            break
    return dict(epsf=E, o=o, R=R, r_fit=r_fit, index=index, stars=rec, change=change, count=count, niter=done, margin=margin.value)


def stamp(E, o):
    p = np.maximum(np.asarray(E, np.float64)[::o, ::o], 0.0)
    return (p / p.sum()).astype(np.float32)


# ---- the planted truth of the tests -----------------------------------------------------------------------------------------------------
def planted_psf(dx, dy, fwhm=3.2):
    """An elliptical Moffat (beta = 2.5, axis ratio 0.8, rotated 30 degrees) plus a faint offset Gaussian lobe; not normalised."""
    beta, q, th = 2.5, 0.8, np.deg2rad(30.0)
    alpha = fwhm / (2.0 * math.sqrt(2.0 ** (1.0 / beta) - 1.0))
    c, s = math.cos(th), math.sin(th)
    a, b = c * dx + s * dy, -s * dx + c * dy
    moffat = (1.0 + (a * a + (b / q) * (b / q)) / (alpha * alpha)) ** (-beta)
    lobe = 0.04 * np.exp(-0.5 * ((dx - 2.2) ** 2 + (dy + 1.4) ** 2) / (1.1 * 1.1))
    return moffat + lobe


def planted_grid(o, R, r_fit, fwhm=3.2):
    """The truth on the grid, float64 [G, G]: the planted PSF moved so that its centre of mass within r_fit (the builder's
    convention for a star's position) is the origin, normalised to sum / o^2 = 1.  Returns (grid, the function of (dx, dy))."""
    G = grid_size(o, R)
    off = (np.arange(G) - o * R) / float(o)
    c = np.zeros(2)
    for _ in range(60):
        g = planted_psf(off[None, :] + c[0], off[:, None] + c[1], fwhm)
        d = centroid(g, o, r_fit)
        c += d
        if math.hypot(*d) < 1e-13:
            break
    g = planted_psf(off[None, :] + c[0], off[:, None] + c[1], fwhm)
    norm = g.sum() / (o * o)
    return g / norm, (lambda dx, dy: planted_psf(dx + c[0], dy + c[1], fwhm) / norm)


def planted_field(shape, n, o, R, r_fit, seed, noise=0.0, sky=100.0, min_sep=None, fwhm=3.2):
    """A field of n isolated stars under the planted effective PSF (evaluated at pixel centres minus the star's position, inside
    the stamp |dx|, |dy| <= R): dict(image float32, x, y, flux: the truth; x0, y0, flux0: a star list as a finder would give it -
    centres off by up to 0.15 px, fluxes 8 % low; sky; truth: the grid)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    truth, fn = planted_grid(o, R, r_fit, fwhm)
    min_sep = float(2 * R + r_fit + 1) if min_sep is None else min_sep
    xs, ys = [], []
    while len(xs) < n:
        cx, cy = rng.uniform(R + 3, W - 1 - (R + 3)), rng.uniform(R + 3, H - 1 - (R + 3))
        if all((cx - a) ** 2 + (cy - b) ** 2 >= min_sep ** 2 for a, b in zip(xs, ys)):
            xs.append(cx)
            ys.append(cy)
    x, y = np.array(xs), np.array(ys)
    flux = 10.0 ** rng.uniform(3.7, 4.7, n)
    img = np.full((H, W), sky)
    for f, cx, cy in zip(flux, x, y):
        x0, x1, y0, y1 = int(math.ceil(cx - R)), int(math.floor(cx + R)), int(math.ceil(cy - R)), int(math.floor(cy + R))
        px, py = np.arange(x0, x1 + 1, dtype=np.float64), np.arange(y0, y1 + 1, dtype=np.float64)
        img[y0:y1 + 1, x0:x1 + 1] += f * fn(px[None, :] - cx, py[:, None] - cy)
    if noise > 0:
        img = img + rng.normal(0.0, noise, img.shape)
    return dict(image=img.astype(np.float32), x=x, y=y, flux=flux, sky=sky, truth=truth,
                x0=x + rng.uniform(-0.15, 0.15, n), y0=y + rng.uniform(-0.15, 0.15, n), flux0=0.92 * flux)
