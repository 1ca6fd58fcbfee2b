import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def load_g11():
    """G11 is stored as two archives (each under the size limit of a committed file); one mapping of all its arrays."""
    return {**load_golden('g11_calibrate_f64.npz'), **load_golden('g11_calibrate_f64_cases.npz')}


def meta(g, key):
    return json.loads(str(g[key]))


def f32_ordered(a):
    """float32 -> int64 keys with the same ordering (for ulp distances)."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


def ulp_diff(a, b):
    """max |ulp distance| between float32 arrays; NaN must match NaN exactly in position."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), 'NaN positions differ: %d vs %d' % (na.sum(), nb.sum())
    d = np.abs(f32_ordered(a) - f32_ordered(b))
    d[na] = 0
    return d


def assert_ulp(a, b, tol=1, what=''):
    d = ulp_diff(a, b)
    assert d.max(initial=0) <= tol, '%s: max ulp diff %d (>%d) at %s; %d of %d differ' % (
        what, d.max(), tol, np.unravel_index(d.argmax(), d.shape), (d > 0).sum(), d.size)
    return float((d == 0).mean()) if d.size else 1.0


def assert_biteq(a, b, what=''):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind == 'f':
        v = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        ok = (a.view(v) == b.view(v)) | (np.isnan(a) & np.isnan(b))
    else:
        ok = a == b
    assert ok.all(), '%s: %d of %d differ, first at %s' % (what, (~ok).sum(), ok.size, np.argwhere(~ok)[:3].tolist())


def np_clip_stats(x, sigma=3.0, maxiters=5):
    """astropy's noaxis sigma_clipped_stats restated with the numpy functions it calls (host reference for samples)."""
    x = x[np.isfinite(x)]
    for _ in range(maxiters):
        if x.size == 0:
            break
        med = np.nanmedian(x)
        sd = np.nanstd(x)
        # SigmaClip._compute_bounds: scalar of the dtype * python float is float64 under the reference's numpy; the array
        # comparison demotes the bound to the dtype (csrc/autobadcol.hip, findstars_model.annulus_clip)
        with np.errstate(all='ignore'):
            lo = x.dtype.type(np.float64(med) - np.float64(sd) * sigma)
            hi = x.dtype.type(np.float64(med) + np.float64(sd) * sigma)
        y = x[(x >= lo) & (x <= hi)]
        changed = y.size != x.size
        x = y
        if not changed:
            break
    return x


def synth_cube(rng, N, shape, nan_frac=0.0, dtype=np.float32):
    """Frames with Gaussian noise, cosmic-ray-like positive outliers and a few low outliers."""
    cube = rng.normal(500, 20, (N,) + tuple(shape))
    hits = rng.random(cube.shape) < 0.02
    cube[hits] += rng.uniform(100, 5000, hits.sum())
    lows = rng.random(cube.shape) < 0.005
    cube[lows] -= rng.uniform(100, 400, lows.sum())
    if dtype == np.uint16:
        return np.clip(np.rint(cube), 0, 65535).astype(np.uint16)
    cube = cube.astype(np.float32)
    if nan_frac > 0:
        bad = rng.random(cube.shape) < nan_frac
        vals = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), bad.sum())
        cube[bad] = vals
    return cube


def synth_masters(rng, shape):
    bias = rng.normal(1000, 5, shape).astype(np.float32)
    dark = rng.normal(20, 3, shape).astype(np.float32)
    hot = rng.random(shape) < 0.002
    dark[hot] = rng.uniform(2000, 6000, hot.sum()).astype(np.float32)
    flat = rng.normal(30000, 300, shape).astype(np.float32)
    return bias, dark, flat


G15_FILES = ('g15_boxstats_a.npz', 'g15_boxstats_b.npz', 'g15_boxstats_c.npz')


def g15_image(g, key):
    """An image of G15 as float32: stored as is, or as integers times a power-of-two scale with NaN / +-inf / -0.0 listed."""
    a = g[key]
    if a.dtype == np.float32:
        return a
    img = (a.astype(np.float64) * float(g[key + '_scale'])).astype(np.float32)
    img.ravel()[g[key + '_special_idx']] = g[key + '_special_val']
    return img


def g15_cases():
    """Every case of golden group G15 (tests/golden/make_golden_boxstats.py), none left out: dicts with the float32 image, the
    uint8 mask or None, box, sigma, maxiters and what astropy computed per box."""
    for name in G15_FILES:
        g = load_golden(name)
        for m in meta(g, '_meta'):
            k = m['case']
            c = dict(m, file=name, img=g15_image(g, m['image']), mask_arr=None if m['mask'] is None else g[m['mask']])
            for f in ('median', 'std', 'std_hp', 'count', 'nmasked0', 'lo', 'hi'):
                c[f] = g[f'c{k}_{f}']
            yield c


# Largest relative deviation of the oracle's per-box std (sequential float64 sums, apref.c) from G15's high-precision std
# (math.fsum), measured over all 72 cases of G15: 1.229e-13 (case 'flat', 182 x 184 boxes, sigma 3, maxiters 5).
G15_ORACLE_STD_DEV = 1.3e-13
