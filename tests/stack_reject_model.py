"""The NumPy restatement of the two rejection rules of small stacks (include/apgpu.h, csrc/stack_reject.hip).

Per pixel: S = the finite values of the column (float32 values, after any calibration), widened to float64, in frame order.  A
masked pixel or an empty S gives NaN and count 0.  Every product and sum below is a NumPy operation of its own, so it rounds on
its own; np.median of an even count is the two middle values summed from +0 and halved (tests/orderstat_cases.py).

Winsorized (kl, kh >= 0; maxiters rounds, < 0 or None: until a round removes nothing):

    round:  n = len(S); if n < 3: stop
            med = np.median(S); sig = np.std(S)
            repeat at most MAX_INNER = 16 times:
                W   = min(max(S, med - 1.5*sig), med + 1.5*sig)      # clamped from S each time, never from the previous W
                s0  = sig; sig = 1.134 * np.std(W)
                if |sig - s0| <= 0.0005 * s0: break
            keep x with  med - kl*sig <= x <= med + kh*sig           # inclusive
            if nothing was removed: stop;  S = the kept values, still in frame order

Min/max (nlow, nhigh whole numbers): order S by (order_key of the value - -0.0 below +0.0 -, frame index), drop the first nlow
and the last nhigh; n <= nlow + nhigh leaves nothing.

Outputs over the survivors in frame order: count = m, mean_f64 = np.add.reduce(surv) / m, std_f64 = np.std(surv).

The functions work on whole cubes [N, ...]: columns with the same number of survivors are gathered into a C-contiguous
[columns, n] array and reduced along its last axis, which is NumPy's pairwise sum of a 1-D array row by row (column_stats_1d does
the same one column at a time with 1-D calls; tests/test_stack_reject_model_host.py compares the two).
"""
import numpy as np

from tests.orderstat_cases import order_key

MAX_INNER = 16                      # APGPU_STACK_WINSOR_MAX_INNER
REJECT_MAX = 128                    # APGPU_STACK_REJECT_MAX


def _columns(cube, pixmask):
    cube = np.asarray(cube)
    if cube.dtype != np.float32:
        raise TypeError('the model takes the float32 values the kernel forms (calibrate first; uint16 frames: astype(float32))')
    N = cube.shape[0]
    shp = cube.shape[1:]
    x = np.ascontiguousarray(cube.reshape(N, -1).T)                 # [P, N]: a column is a row
    keep = np.isfinite(x)
    if pixmask is not None:
        keep &= (np.asarray(pixmask).reshape(-1) == 0)[:, None]
    return x, keep, shp


def _gather(x, keep, idx, n):
    """The kept values of the columns idx (each has n of them) in frame order, float64 [len(idx), n]."""
    return np.ascontiguousarray(x[idx][keep[idx]].reshape(len(idx), n).astype(np.float64))


def _final(x, keep, shp, extra):
    P = x.shape[0]
    cnt = keep.sum(1).astype(np.int32)
    mean = np.full(P, np.nan)
    std = np.full(P, np.nan)
    for n in np.unique(cnt):
        if n == 0:
            continue
        idx = np.flatnonzero(cnt == n)
        S = _gather(x, keep, idx, n)
        mean[idx] = np.add.reduce(S, axis=1) / n
        std[idx] = np.std(S, axis=1)
    out = dict(mean_f64=mean.reshape(shp), std_f64=std.reshape(shp), count=cnt.reshape(shp),
               keep=np.ascontiguousarray(keep.T).reshape((x.shape[1],) + shp))
    out.update(extra)
    return out


def winsorized(cube, kl=3.0, kh=3.0, maxiters=None, pixmask=None):
    """-> dict(mean_f64, std_f64, count, keep [N, ...] bool, inner [...]: inner steps summed over the column's rounds,
    inner_max [...]: the most inner steps one round took, capped [...] bool: a round reached MAX_INNER, rounds [...])."""
    x, keep, shp = _columns(cube, pixmask)
    P = x.shape[0]
    maxiters = -1 if maxiters is None else int(maxiters)
    inner = np.zeros(P, np.int64)
    inner_max = np.zeros(P, np.int64)
    capped = np.zeros(P, bool)
    rounds = np.zeros(P, np.int64)
    active = np.ones(P, bool)
    it = 0
    while True:
        cnt = keep.sum(1)
        active &= cnt >= 3
        if not active.any() or (maxiters >= 0 and it >= maxiters):
            break
        for n in np.unique(cnt[active]):
            idx = np.flatnonzero(active & (cnt == n))
            S = _gather(x, keep, idx, n)
            med = np.median(S, axis=1)
            sig = np.std(S, axis=1)
            going = np.ones(len(idx), bool)
            steps = np.zeros(len(idx), np.int64)
            for _ in range(MAX_INNER):
                lo, hi = med - 1.5 * sig, med + 1.5 * sig
                W = np.minimum(np.maximum(S, lo[:, None]), hi[:, None])
                s0 = sig
                sig = np.where(going, 1.134 * np.std(W, axis=1), sig)
                steps += going
                going = going & ~(np.abs(sig - s0) <= 0.0005 * s0)
                if not going.any():
                    break
            inner[idx] += steps
            inner_max[idx] = np.maximum(inner_max[idx], steps)
            capped[idx] |= going
            rounds[idx] += 1
            lo, hi = med - kl * sig, med + kh * sig
            ok = (S >= lo[:, None]) & (S <= hi[:, None])
            removed = ~ok.all(1)
            sub = keep[idx]
            sub[sub.copy()] = ok.reshape(-1)
            keep[idx] = sub
            active[idx] = removed
        it += 1
    return _final(x, keep, shp, dict(inner=inner.reshape(shp), inner_max=inner_max.reshape(shp), capped=capped.reshape(shp),
                                     rounds=rounds.reshape(shp)))


def minmax(cube, nlow=1, nhigh=1, pixmask=None):
    """-> dict(mean_f64, std_f64, count, keep [N, ...] bool, inner [...] (zeros: the rule has no inner steps))."""
    nlow, nhigh = int(nlow), int(nhigh)
    if not (0 <= nlow <= 127 and 0 <= nhigh <= 127):
        raise ValueError('nlow and nhigh are whole numbers in 0 .. 127')
    x, keep, shp = _columns(cube, pixmask)
    P, N = x.shape
    key = order_key(x).astype(np.uint64)
    key[~keep] = np.uint64(1) << np.uint64(40)                       # behind every value's key
    order = np.argsort(key, axis=1, kind='stable')                   # ties: by frame index
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(N), (P, N)), axis=1)
    n = keep.sum(1)[:, None]
    keep = keep & (rank >= nlow) & (rank < n - nhigh)
    return _final(x, keep, shp, dict(inner=np.zeros(shp, np.int64)))


def column_stats_1d(values):
    """(mean_f64, std_f64) of one column's survivors with 1-D NumPy calls only - the definition's own words."""
    s = np.ascontiguousarray(values, dtype=np.float64)
    return np.add.reduce(s) / s.size, np.std(s)
