"""The NumPy restatement of the generalized ESD rejection rule of the stack (include/apgpu.h APGPU_STACK_REJECT_ESD,
csrc/stack_esd.hip; Rosner 1983).

Per pixel: S = the finite values of the column (float32 values, after any calibration or frame map), widened to float64,
n = len(S).  A masked pixel or an empty S gives NaN and count 0.  Every product, quotient and sum below is a NumPy operation of
its own, so it rounds on its own.  With the table lam [N + 1, max_outliers] of critical values (ops.esd_lambda):

    K = min(floor(frac * n), n - 3, max_outliers)        # frac * n: one float64 product; K <= 0: nothing is removed
    y = S ordered by (order_key of the value: -0.0 below +0.0, then frame index);  lo, hi = 0, n;  L = H = 0
    for i in 0 .. K-1:
        w = y[lo:hi];  m = hi - lo
        mean = np.add.reduce(w) / m;  d = w - mean;  sd = np.sqrt(np.add.reduce(d * d) / (m - 1))
        if not (sd > 0): break
        dl = (mean - w[0]) / relax;  dh = w[m-1] - mean
        if dh >= dl: R = dh / sd; hi -= 1     else: R = dl / sd; lo += 1
        if R > lam[n][i]: L, H = lo, n - hi
    survivors = the min/max rule (tests/stack_reject_model.py) with nlow = L, nhigh = H on S, same ties

Outputs over the survivors in frame order as for min/max: count = m, mean_f64 = np.add.reduce(surv) / m, std_f64 =
np.std(surv); with per-frame weights (APGPU_STACK_FRAME_PARAMS / APGPU_STACK_FRAME_LOCAL: esd_weighted) mean_f64 = num / den
summed sequentially in frame order, as tests/stack_frame_model.py has it.

esd works on whole cubes: the columns with the same n are gathered into a C-contiguous [columns, n] array, their windows into
[columns, m] (every step shortens every window by one), and reduced along the last axis - NumPy's pairwise sum of a 1-D array
row by row.  column_1d is the same one column at a time, plain loops and 1-D calls: the definition's own words.
"""
import numpy as np

from tests import stack_reject_model as reject
from tests.orderstat_cases import order_key

F = np.float32


def steps_of(n, frac, max_outliers):
    """K of a column with n finite values."""
    return max(min(int(np.floor(np.float64(frac) * np.float64(n))), n - 3, int(max_outliers)), 0)


def _sorted_columns(x, keep):
    """-> (order [P, N]: frame indices by (key, frame index), finite ones first; rank [P, N]; n [P])"""
    P, N = x.shape
    key = order_key(x).astype(np.uint64)
    key[~keep] = np.uint64(1) << np.uint64(40)                       # behind every value's key
    order = np.argsort(key, axis=1, kind='stable')                   # ties: by frame index
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(N), (P, N)), axis=1)
    return order, rank, keep.sum(1)


def esd(cube, lam, frac=0.3, relax=1.5, pixmask=None):
    """-> dict(mean_f64, std_f64, count, keep [N, ...] bool, L [...], H [...]: the values dropped at either end, steps [...]: the
    steps the column ran, R [...]: its largest test statistic or NaN)."""
    lam = np.asarray(lam, np.float64)
    x, keep, shp = reject._columns(cube, pixmask)
    P, N = x.shape
    if lam.ndim != 2 or lam.shape[0] != N + 1:
        raise ValueError('lam must be [N + 1, max_outliers]')
    maxout = lam.shape[1]
    relax = np.float64(relax)
    order, rank, cnt = _sorted_columns(x, keep)
    L = np.zeros(P, np.int64)
    H = np.zeros(P, np.int64)
    steps = np.zeros(P, np.int64)
    Rmax = np.full(P, np.nan)
    with np.errstate(all='ignore'):
        for n in np.unique(cnt):
            K = steps_of(int(n), frac, maxout)
            if K <= 0:
                continue
            idx = np.flatnonzero(cnt == n)
            y = np.ascontiguousarray(np.take_along_axis(x[idx], order[idx][:, :n], axis=1).astype(np.float64))
            lo = np.zeros(len(idx), np.int64)
            hi = np.full(len(idx), n, np.int64)
            going = np.ones(len(idx), bool)
            for i in range(K):
                m = n - i
                g = np.flatnonzero(going)
                if g.size == 0:
                    break
                w = np.ascontiguousarray(np.take_along_axis(y[g], lo[g][:, None] + np.arange(m)[None, :], axis=1))
                mean = np.add.reduce(w, axis=1) / m
                d = w - mean[:, None]
                sd = np.sqrt(np.add.reduce(d * d, axis=1) / (m - 1))
                ok = sd > 0
                going[g[~ok]] = False
                g, w, mean, sd = g[ok], w[ok], mean[ok], sd[ok]
                dl = (mean - w[:, 0]) / relax
                dh = w[:, m - 1] - mean
                high = dh >= dl
                R = np.where(high, dh, dl) / sd
                hi[g] -= high
                lo[g] += ~high
                sig = R > lam[n, i]
                L[idx[g[sig]]] = lo[g[sig]]
                H[idx[g[sig]]] = n - hi[g[sig]]
                steps[idx[g]] += 1
                Rmax[idx[g]] = np.fmax(Rmax[idx[g]], R)
    keep = keep & (rank >= L[:, None]) & (rank < (cnt - H)[:, None])
    return reject._final(x, keep, shp, dict(L=L.reshape(shp), H=H.reshape(shp), steps=steps.reshape(shp), R=Rmax.reshape(shp)))


def esd_weighted(v, w, lam, frac=0.3, relax=1.5, pixmask=None):
    """The rule on a mapped cube v (stack_frame_model.frame_map / stack_local_model.local_values) with per-frame weights w:
    count and std_f64 are the rule's own, mean_f64 = num / den over the survivors in frame order, sequentially from +0.0."""
    v = np.asarray(v)
    N = v.shape[0]
    r = esd(v, lam, frac=frac, relax=relax, pixmask=pixmask)
    keep = r['keep'].reshape(N, -1)
    vd = v.reshape(N, -1).astype(np.float64)
    wd = np.asarray(w, F).reshape(N).astype(np.float64)[:, None]
    num = np.zeros(vd.shape[1])
    den = np.zeros(vd.shape[1])
    for k in range(N):
        num = np.where(keep[k], num + wd[k] * vd[k], num)
        den = np.where(keep[k], den + wd[k], den)
    with np.errstate(invalid='ignore', divide='ignore'):
        r['mean_f64'] = np.where(keep.any(0), num / den, np.nan).reshape(r['count'].shape)
    return r


def column_1d(column, lam, frac=0.3, relax=1.5):
    """One column (float32 values, any non-finite ones included) in the definition's own words: plain loops and 1-D NumPy calls
    -> dict(mean_f64, std_f64, count, keep: list of bool, L, H, R: the test statistic of every step run, sides: 'h' or 'l', the
    end each step took its candidate from)."""
    column = np.asarray(column, F)
    lam = np.asarray(lam, np.float64)
    N = column.size
    idx = [i for i in range(N) if np.isfinite(column[i])]
    n = len(idx)
    order = sorted(idx, key=lambda i: (int(order_key(column[i:i + 1])[0]), i))
    y = np.array([column[i] for i in order], np.float64)
    K = steps_of(n, frac, lam.shape[1])
    lo, hi, L, H = 0, n, 0, 0
    Rs, sides = [], []
    with np.errstate(all='ignore'):
        for i in range(K):
            w = np.ascontiguousarray(y[lo:hi])
            m = hi - lo
            mean = np.add.reduce(w) / m
            d = w - mean
            sd = np.sqrt(np.add.reduce(d * d) / (m - 1))
            if not (sd > 0):
                break
            dl = (mean - w[0]) / np.float64(relax)
            dh = w[m - 1] - mean
            if dh >= dl:
                R = dh / sd
                hi -= 1
            else:
                R = dl / sd
                lo += 1
            Rs.append(float(R))
            sides.append('h' if dh >= dl else 'l')
            if R > lam[n][i]:
                L, H = lo, n - hi
    surv = sorted(order[L:n - H])
    keep = [i in surv for i in range(N)]
    if not surv:
        return dict(mean_f64=np.nan, std_f64=np.nan, count=0, keep=keep, L=L, H=H, R=Rs, sides=sides)
    mean, sd = reject.column_stats_1d([column[i] for i in surv])
    return dict(mean_f64=mean, std_f64=sd, count=len(surv), keep=keep, L=L, H=H, R=Rs, sides=sides)
