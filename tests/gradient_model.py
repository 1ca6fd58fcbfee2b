"""The sky-gradient removal (F20) in NumPy: samples, both fits, the rejection, the lattice, the interpolant and the
apply pass.  *** TEST INFRASTRUCTURE ONLY ***  *** PARITY UNPINNED *** (the reference has no such stage).

Written once; csrc/gradient.hip, ops.py and core/ApRemoveGradient.py are held to it.  Everything is float64 unless it says float32, and
NumPy rounds after every operation, as the kernels do (no contraction).

Coordinates: a pixel centre is (x, y) = (column, row), 0-based; u = (x - x0) / L, v = (y - y0) / L with x0 = (W - 1) / 2,
y0 = (H - 1) / 2, L = max(W, H) / 2.
"""
import numpy as np

MAX_SAMPLES, MAX_RADIUS, MAX_DEGREE, MIN_STEP, MAX_STEP = 4096, 32, 6, 4, 64
F = np.float32


def frame(shape):
    H, W = shape
    return (W - 1) / 2.0, (H - 1) / 2.0, max(W, H) / 2.0


# ---- 1. samples -------------------------------------------------------------------------------------------------------------------
def _median(v):
    """The middle element, or half the sum of the two middle ones (a median of -0.0 stays -0.0, where np.median returns +0.0)."""
    s = np.sort(v)
    n = s.size
    return float(s[n // 2]) if n & 1 else float((s[n // 2 - 1] + s[n // 2]) / 2.0)


def clipped_stats(values, sigma=3.0, maxiters=5):
    """astropy's SigmaClip(sigma, maxiters, cenfunc='median', stdfunc='std') of a line of values (its C loop: the working set is
    packed in place, sums run in order from 0), then nanmedian / nanstd of everything inside the last bounds.  maxiters 0: until
    nothing changes.  Returns median, std, survivors."""
    v = np.asarray(values, np.float64).reshape(-1)
    v = v[np.isfinite(v)]
    buf, lo, hi, it = v, np.nan, np.nan, 0
    while buf.size:
        n = buf.size
        med = _median(buf)
        mean = np.cumsum(buf)[-1] / n                          # (cumsum adds in order, np.sum does not)
        std = np.sqrt(np.cumsum((mean - buf) ** 2)[-1] / n)
        lo, hi = med - sigma * std, med + sigma * std
        new = buf[(buf >= lo) & (buf <= hi)]
        if new.size == n:
            break
        buf, it = new, it + 1
        if maxiters and it >= maxiters:
            break
    keep = v[~(v < lo) & ~(v > hi)]                            # NaN bounds (everything was clipped away) keep every value
    if keep.size == 0:
        return np.nan, np.nan, 0
    mean = np.cumsum(keep)[-1] / keep.size
    return _median(keep), float(np.sqrt(np.cumsum((keep - mean) ** 2)[-1] / keep.size)), int(keep.size)


def cut_box(data, mask, x, y, r):
    """The (2 r + 1)^2 values of the box about (x, y), row by row: NaN outside the image, under the mask and where not finite."""
    H, W = data.shape
    out = np.full((2 * r + 1, 2 * r + 1), np.nan, F)
    y0, y1, x0, x1 = max(y - r, 0), min(y + r, H - 1), max(x - r, 0), min(x + r, W - 1)
    if y0 <= y1 and x0 <= x1:
        cut = data[y0:y1 + 1, x0:x1 + 1].astype(F)
        bad = ~np.isfinite(cut)
        if mask is not None:
            bad |= np.asarray(mask)[y0:y1 + 1, x0:x1 + 1] != 0
        out[y0 - (y - r):y1 - (y - r) + 1, x0 - (x - r):x1 - (x - r) + 1] = np.where(bad, np.nan, cut)
    return out


def sample_stats(data, mask, centres, r, sigma=3.0, maxiters=5):
    """float64 [K, 4]: median, std, survivors, pixels of the box that were outside, masked or not finite."""
    out = np.zeros((len(centres), 4))
    for k, (x, y) in enumerate(np.asarray(centres, np.int64).reshape(-1, 2)):
        box = cut_box(data, mask, int(x), int(y), r)
        med, std, n = clipped_stats(box, sigma, maxiters)
        out[k] = med, std, n, np.isnan(box).sum()
    return out


def sample_pixels(shape, centres, r):
    H, W = shape
    c = np.asarray(centres, np.int64).reshape(-1, 2)
    nx = np.clip(np.minimum(c[:, 0] + r, W - 1) - np.maximum(c[:, 0] - r, 0) + 1, 0, None)
    ny = np.clip(np.minimum(c[:, 1] + r, H - 1) - np.maximum(c[:, 1] - r, 0) + 1, 0, None)
    return nx * ny


def grid_samples(shape, samples_per_row=16, exclude=()):
    """int32 [K, 2] (x, y): samples_per_row columns at the pitch W / samples_per_row, the same pitch in y, centred in the image."""
    H, W = shape
    n = samples_per_row
    pitch = W / float(n)
    rows = max(1, int(np.floor(H / pitch)))
    xs = np.floor((W - 1) / 2.0 + (np.arange(n) - (n - 1) / 2.0) * pitch + 0.5)
    ys = np.floor((H - 1) / 2.0 + (np.arange(rows) - (rows - 1) / 2.0) * pitch + 0.5)
    xy = np.array([(x, y) for y in ys for x in xs], np.float64).reshape(-1, 2)
    keep = np.ones(len(xy), bool)
    for x0, y0, x1, y1 in exclude:
        keep &= ~((xy[:, 0] >= min(x0, x1)) & (xy[:, 0] <= max(x0, x1)) & (xy[:, 1] >= min(y0, y1)) & (xy[:, 1] <= max(y0, y1)))
    return xy[keep].astype(np.int32)


def sample_sigmas(std, n):
    """sigma_k = 1.2533 std / sqrt(n); a zero (a constant box) takes the smallest positive one, 1 if there is none."""
    with np.errstate(divide='ignore', invalid='ignore'):
        sg = 1.2533 * np.asarray(std, np.float64) / np.sqrt(np.asarray(n, np.float64))
    pos = np.isfinite(sg) & (sg > 0)
    return np.where(pos, sg, sg[pos].min() if pos.any() else 1.0)


def usable(stats, shape, centres, r, min_fraction=0.5):
    inside = sample_pixels(shape, centres, r)
    return (stats[:, 2] >= 1) & (stats[:, 2] >= min_fraction * inside) & np.isfinite(stats[:, 0])


# ---- 2. the fit -------------------------------------------------------------------------------------------------------------------
def poly_terms(degree):
    return [(t - j, j) for t in range(degree + 1) for j in range(t + 1)]


def powers(u, degree):
    p = [np.ones_like(np.asarray(u, np.float64))]
    for _ in range(degree):
        p.append(p[-1] * u)
    return p


def phi(q):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(q == 0.0, 0.0, 0.5 * q * np.log(q))


def evaluate(surface, u, v, want_bound=False):
    """The surface at normalised coordinates, the terms added in index order from +0 as the lattice kernel adds them; with
    want_bound also (n + 8) 2^-53 sum |term|, n the number of terms: any order of the sum, at most 4 roundings a term, a 1-ulp log."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    acc, mag = np.zeros(np.broadcast(u, v).shape), np.zeros(np.broadcast(u, v).shape)
    if surface['model'] == 'poly':
        d = surface['degree']
        pu, pv = powers(u, d), powers(v, d)
        for c, (i, j) in zip(surface['coef'], poly_terms(d)):
            t = c * (pu[i] * pv[j])
            acc, mag = acc + t, mag + np.abs(t)
        n = len(surface['coef'])
    else:
        for (uk, vk), wk in zip(surface['uv'], surface['w']):
            du, dv = u - uk, v - vk
            t = wk * phi(du * du + dv * dv)
            acc, mag = acc + t, mag + np.abs(t)
        a = surface['a']
        acc = ((acc + a[0]) + a[1] * u) + a[2] * v
        mag = mag + abs(a[0]) + np.abs(a[1] * u) + np.abs(a[2] * v)
        n = len(surface['w'])
    return (acc, (n + 8) * 2.0 ** -53 * mag) if want_bound else acc


def surface_at(surface, x, y):
    x0, y0, L = surface['frame']
    return evaluate(surface, (np.asarray(x, np.float64) - x0) / L, (np.asarray(y, np.float64) - y0) / L)


def _mad_sigma(res):
    return 1.4826 * float(np.median(np.abs(res - np.median(res))))


def fit(xy, values, sigmas, shape, model='poly', degree=3, smoothing=0.1, k_high=2.0, k_low=3.0, max_rounds=5, use=None):
    """Weighted fit with rejection; returns (surface, kept, sigma_r).  ValueError: fewer than P + 3 (poly) or 8 (tps) samples."""
    if model not in ('poly', 'tps'):
        raise ValueError('unknown model %r' % (model,))
    x0, y0, L = frame(shape)
    xy, z, sg = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(values, np.float64), np.asarray(sigmas, np.float64)
    u, v = (xy[:, 0] - x0) / L, (xy[:, 1] - y0) / L
    kept = np.isfinite(z) & np.isfinite(sg) & (sg > 0)
    if use is not None:
        kept &= np.asarray(use, bool)
    need = (degree + 1) * (degree + 2) // 2 + 3 if model == 'poly' else 8
    for rnd in range(max_rounds + 1):
        i = np.flatnonzero(kept)
        if i.size < need:
            raise ValueError('%d samples left, %d needed' % (i.size, need))
        om = 1.0 / sg[i] ** 2
        if model == 'poly':
            pu, pv = powers(u[i], degree), powers(v[i], degree)
            A = np.stack([pu[a] * pv[b] for a, b in poly_terms(degree)], axis=1)
            coef = np.linalg.lstsq(A * np.sqrt(om)[:, None], z[i] * np.sqrt(om), rcond=None)[0]
            surface = dict(model='poly', degree=degree, coef=coef, frame=(x0, y0, L))
            model_z = A @ coef
        else:
            n = i.size
            Phi = phi((u[i][:, None] - u[i][None, :]) ** 2 + (v[i][:, None] - v[i][None, :]) ** 2)
            T = np.stack([np.ones(n), u[i], v[i]], axis=1)
            M = np.block([[Phi + np.diag(smoothing * n * om.mean() / om), T], [T.T, np.zeros((3, 3))]])
            sol = np.linalg.solve(M, np.concatenate([z[i], np.zeros(3)]))
            surface = dict(model='tps', w=sol[:n], a=sol[n:], uv=np.stack([u[i], v[i]], axis=1), frame=(x0, y0, L))
            model_z = Phi @ sol[:n] + T @ sol[n:]
        res = z[i] - model_z
        sigma_r = _mad_sigma(res)
        drop = (res > k_high * sigma_r) | (res < -k_low * sigma_r)
        if rnd == max_rounds or not sigma_r > 0 or not drop.any():
            break
        kept = kept.copy()
        kept[i[drop]] = False
    return surface, kept, sigma_r


# ---- 3. the lattice and its interpolant -----------------------------------------------------------------------------------------------
def lattice_shape(shape, step):
    return (shape[0] - 1) // step + 4, (shape[1] - 1) // step + 4


def lattice(surface, shape, step, want_bound=False):
    """The surface at the nodes: node (iy, ix) at pixel ((ix - 1) step, (iy - 1) step)."""
    ny, nx = lattice_shape(shape, step)
    x0, y0, L = surface['frame']
    u = ((np.arange(nx, dtype=np.float64) - 1.0) * step - x0) / L
    v = ((np.arange(ny, dtype=np.float64) - 1.0) * step - y0) / L
    return evaluate(surface, u[None, :] + 0.0 * v[:, None], v[:, None] + 0.0 * u[None, :], want_bound)


def keys_weights(t):
    """Keys' cubic convolution, a = -1/2: the weights of the four nodes about a point t in [0, 1) past the second one."""
    return (((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * t * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * t * t)


def interpolate(lat, shape, step):
    """float64 [H, W]: x first (per lattice row), then y."""
    H, W = shape
    assert lat.shape == lattice_shape(shape, step)
    x, y = np.arange(W), np.arange(H)
    ix, iy = x // step, y // step
    wx = keys_weights((x - ix * step).astype(np.float64) / float(step))
    wy = keys_weights((y - iy * step).astype(np.float64) / float(step))
    rows = ((wx[0] * lat[:, ix] + wx[1] * lat[:, ix + 1]) + wx[2] * lat[:, ix + 2]) + wx[3] * lat[:, ix + 3]          # [ny, W]
    return ((wy[0][:, None] * rows[iy] + wy[1][:, None] * rows[iy + 1]) + wy[2][:, None] * rows[iy + 2]) + wy[3][:, None] * rows[iy + 3]


INTERPOLANT_GAIN = 1.25 ** 2            # sum |w| of the Keys weights is at most 1.25 (at t = 1/2), in x and in y


# ---- 4. apply ---------------------------------------------------------------------------------------------------------------------
def apply(data, S, mode='subtract', pedestal=0.0):
    """float32 [H, W] and float32(S)."""
    if mode not in ('subtract', 'divide'):
        raise ValueError('unknown mode %r' % (mode,))
    d = np.asarray(data, F).astype(np.float64)
    with np.errstate(all='ignore'):
        if mode == 'subtract':
            out = ((d - S) + pedestal).astype(F)
        else:
            out = np.where((S > 0) & np.isfinite(S), (d / S) * pedestal, np.nan).astype(F)
        out[~np.isfinite(data)] = np.nan
        return out, S.astype(F)


def remove(data, mask, centres=None, model='poly', degree=3, smoothing=0.1, samples_per_row=16, box_radius=12, exclude=(), mode='subtract',
           pedestal=None, k_high=2.0, k_low=3.0, max_rounds=5, step=16, sigma=3.0, maxiters=5, min_fraction=0.5):
    """The whole stage on the host; dict(image, surface, stats, centres, used, kept, model, pedestal, sigma_r, lattice)."""
    shape = data.shape
    c = grid_samples(shape, samples_per_row, exclude) if centres is None else np.asarray(centres, np.int32).reshape(-1, 2)
    st = sample_stats(data, mask, c, box_radius, sigma, maxiters)
    use = usable(st, shape, c, box_radius, min_fraction)
    sg = sample_sigmas(np.where(use, st[:, 1], np.nan), st[:, 2])
    surface, kept, sigma_r = fit(c, st[:, 0], sg, shape, model, degree, smoothing, k_high, k_low, max_rounds, use)
    p = float(np.median(st[kept, 0])) if pedestal is None else float(pedestal)
    lat = lattice(surface, shape, step)
    image, surf = apply(data, interpolate(lat, shape, step), mode, p)
    return dict(image=image, surface=surf, stats=st, centres=c, used=use, kept=kept, model=surface, pedestal=p, sigma_r=sigma_r, lattice=lat)
