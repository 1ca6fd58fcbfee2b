"""The NumPy restatement of APGPU_STACK_FRAME_PARAMS (include/apgpu.h, csrc/stack_reject.hip): per-frame scale, offset and
weight inside the two rejection rules of small stacks.

Per frame i: scale a_i, offset b_i, weight w_i (float32).  x = the raw value as float32, v = float32(float32(a_i * x) + b_i).
S = the finite v of the column in frame order; the rule (tests/stack_reject_model.py: winsorized / minmax, unchanged) runs on S.
count = m and std_f64 = np.std(surv) are the rule's own, unweighted.  mean_f64 = num / den with

    num += float64(w_k) * float64(v_k)          # exact: the product of two widened float32 values
    den += float64(w_k)

over the survivors in frame order, sequentially from +0.0 - which is np.cumsum(terms)[-1], not NumPy's pairwise sum.
"""
import numpy as np

from tests import stack_reject_model as reject

F = np.float32


def frame_map(cube, a, b):
    """v = float32(float32(a_i * x) + b_i): two NumPy operations, two roundings."""
    cube = np.asarray(cube)
    x = cube.astype(F)
    N = x.shape[0]
    bc = (N,) + (1,) * (x.ndim - 1)
    a = np.asarray(a, F).reshape(bc)
    b = np.asarray(b, F).reshape(bc)
    with np.errstate(over='ignore', invalid='ignore'):
        return (a * x).astype(F) + b


def frame_params(cube, a, b, w, method, pixmask=None, **rule):
    """-> dict(mean_f64, std_f64, count, keep [N, ...] bool, v: the mapped cube).  method: 'winsorized' (kl, kh, maxiters) or
    'minmax' (nlow, nhigh)."""
    if method not in ('winsorized', 'minmax'):
        raise ValueError(method)
    v = frame_map(cube, a, b)
    N = v.shape[0]
    w = np.asarray(w, F).reshape(N)
    r = (reject.winsorized if method == 'winsorized' else reject.minmax)(v, pixmask=pixmask, **rule)
    keep = r['keep'].reshape(N, -1)
    vd = v.reshape(N, -1).astype(np.float64)
    wd = w.astype(np.float64)[:, None]
    # a term that is not a survivor's is left out of the sequence, not added as a zero: +0.0 + -0.0 would differ otherwise
    num = np.zeros(vd.shape[1])
    den = np.zeros(vd.shape[1])
    for k in range(N):
        num = np.where(keep[k], num + wd[k] * vd[k], num)
        den = np.where(keep[k], den + wd[k], den)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(keep.any(0), num / den, np.nan)
    return dict(mean_f64=mean.reshape(r['count'].shape), std_f64=r['std_f64'], count=r['count'], keep=r['keep'], v=v)


TRAIL_ROW, TRAIL_FRAMES, TRAIL_ADU, SCENE_SHAPE, SCENE_NOISE = 20, (2, 5), 120.0, (48, 64), 8.0


def star_field(shape=SCENE_SHAPE, nstars=12, seed=1):
    """A few Gaussian stars (FWHM about 3 pixels, peaks 200 .. 3000 ADU) on zero sky: float64 [H, W]."""
    rng = np.random.default_rng(seed)
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.zeros(shape)
    for _ in range(nstars):
        y, x, peak = rng.uniform(3, H - 3), rng.uniform(3, W - 3), 10.0 ** rng.uniform(2.3, 3.5)
        img += peak * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * 1.3 ** 2))
    return img


def trail_scene(N, seed, sky_lo=100.0, sky_hi=400.0, noise=SCENE_NOISE):
    """The scene the normalisation was added for: the star field, noise sigma 8, sky levels spread evenly over sky_lo .. sky_hi
    across the N frames, and a +120 ADU trail along row TRAIL_ROW of frames 2 and 5.
    -> (cube float32 [N, 48, 64], stars float64 [48, 64], sky float64 [N])"""
    rng = np.random.default_rng(seed)
    stars = star_field()
    sky = np.linspace(sky_lo, sky_hi, N)
    cube = stars[None] + sky[:, None, None] + rng.normal(0.0, noise, (N,) + stars.shape)
    for f in TRAIL_FRAMES:
        cube[f, TRAIL_ROW] += TRAIL_ADU
    return cube.astype(F), stars, sky


def clipped_stats(frame, sigma=3.0, maxiters=5):
    """(median, std) of a frame's finite values after astropy-style sigma clipping about the median: the host's stand-in for
    ops.frame_stats where no device is at hand (float64 arithmetic; not bit-pinned to the A3 kernels)."""
    x = np.asarray(frame, np.float64).ravel()
    x = x[np.isfinite(x)]
    for _ in range(maxiters):
        med, sd = np.median(x), np.std(x)
        k = (x >= med - sigma * sd) & (x <= med + sigma * sd)
        if k.all():
            break
        x = x[k]
    return np.median(x), np.std(x)


def column_1d(column, a, b, w, method, kl=3.0, kh=3.0, maxiters=None, nlow=1, nhigh=1):
    """One column in the definition's own words: plain 1-D NumPy and Python loops -> (mean_f64, std_f64, count, keep list)."""
    column = np.asarray(column)
    N = column.size
    v = [F(F(F(a[i]) * F(column[i])) + F(b[i])) for i in range(N)]
    idx = [i for i in range(N) if np.isfinite(v[i])]                       # S, by frame index
    if method == 'minmax':
        order = sorted(idx, key=lambda i: (int(reject.order_key(np.array([v[i]], F))[0]), i))
        idx = sorted(order[nlow:len(order) - nhigh]) if len(order) > nlow + nhigh else []
    else:
        it = 0
        while len(idx) >= 3 and (maxiters is None or maxiters < 0 or it < maxiters):
            S = np.array([v[i] for i in idx], np.float64)
            med, sig = np.median(S), np.std(S)
            for _ in range(reject.MAX_INNER):
                W = np.minimum(np.maximum(S, med - 1.5 * sig), med + 1.5 * sig)
                s0 = sig
                sig = 1.134 * np.std(W)
                if abs(sig - s0) <= 0.0005 * s0:
                    break
            lo, hi = med - kl * sig, med + kh * sig
            kept = [i for i, s in zip(idx, S) if lo <= s <= hi]
            it += 1
            if len(kept) == len(idx):
                break
            idx = kept
    keep = [i in idx for i in range(N)]
    if not idx:
        return np.nan, np.nan, 0, keep
    num, den = 0.0, 0.0
    for i in idx:
        num = num + float(F(w[i])) * float(v[i])
        den = den + float(F(w[i]))
    sd = reject.column_stats_1d([v[i] for i in idx])[1]
    return num / den, sd, len(idx), keep
