"""NumPy restatement of F8, the star-list registration (csrc/register.hip, ops.register_lists).

PARITY UNPINNED: the reference has no such step (it sends its source list to astrometry.net), and neither astroalign nor
skimage is available here.  The rule is the triangle-similarity match of Groth (1986) and Valdes et al. (1995) as DESIGN 4.3e
states it; this file is its executable form, and the truth the tests hold it to is a known synthetic transform.

Every function also reports its *margin*: the smallest relative distance |lhs - rhs| / |rhs| of any threshold comparison it
made (the four keep rules of a triangle, eps, the match radius) whose outcome could change the result.  Where the margin is
far above 2^-52 a last-bit difference in lhs cannot flip a decision, and the device must give the same integers.

All float64; every expression is written with one rounding per operation, in the order the kernels use.
"""
import numpy as np

MAX_K = 64
MARGIN_CAP = 1.0e-6            # vote(): pairs outside the candidate window are at least this far from eps


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


# -- triangles -------------------------------------------------------------------------------------------------------------
def triangle_build_frame(pts, K=40, min_side=5.0, margin=None):
    """pts [n, 2] brightest first -> dict(x, y float64 [T]; v int64 [T, 3] = v0, v1, v2; orient int64 [T]) of the kept
    triangles among the first K stars, in (i, j, k) lexical order."""
    assert 3 <= K <= MAX_K, 'K = %d is outside 3 .. %d' % (K, MAX_K)
    margin = margin if margin is not None else Margin()
    pts = np.asarray(pts, np.float64).reshape(-1, 2)[:K]
    n = len(pts)
    ii, jj, kk = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing='ij')
    sel = (ii < jj) & (jj < kk)
    idx = np.stack([ii[sel], jj[sel], kk[sel]], axis=1)                 # [T, 3] vertices i < j < k
    if len(idx) == 0:
        return dict(x=np.zeros(0), y=np.zeros(0), v=np.zeros((0, 3), np.int64), orient=np.zeros(0, np.int64))

    def d2(a, b):
        dx, dy = pts[a, 0] - pts[b, 0], pts[a, 1] - pts[b, 1]
        return dx * dx + dy * dy

    # the side opposite i, j, k in that order; stable descending sort = ties keep the lower opposite vertex first
    sides = np.stack([d2(idx[:, 1], idx[:, 2]), d2(idx[:, 0], idx[:, 2]), d2(idx[:, 0], idx[:, 1])], axis=1)
    order = np.argsort(-sides, axis=1, kind='stable')
    srt = np.take_along_axis(sides, order, axis=1)
    opp = np.take_along_axis(idx, order, axis=1)
    a2, b2, c2 = srt[:, 0], srt[:, 1], srt[:, 2]
    v2, v1, v0 = opp[:, 0], opp[:, 1], opp[:, 2]
    with np.errstate(all='ignore'):
        x, y = np.sqrt(b2 / a2), np.sqrt(c2 / a2)
        ms2 = np.float64(min_side) * np.float64(min_side)
        lim = 0.98 * x
        r1, r2, r3, r4 = c2 >= ms2, y >= 0.1, x <= 0.98, y <= lim
    # a rule's comparison matters for a triangle that passes all the other rules
    for rule, lhs, rhs in ((r1, c2, ms2), (r2, y, 0.1), (r3, x, 0.98), (r4, y, lim)):
        others = np.ones(len(idx), bool)
        for o in (r1, r2, r3, r4):
            if o is not rule:
                others &= o
        margin.update(lhs[others], np.broadcast_to(rhs, lhs.shape)[others])
    keep = r1 & r2 & r3 & r4
    p0, p1, p2 = pts[v0], pts[v1], pts[v2]
    cross = (p1[:, 0] - p0[:, 0]) * (p2[:, 1] - p0[:, 1]) - (p1[:, 1] - p0[:, 1]) * (p2[:, 0] - p0[:, 0])
    orient = np.sign(cross).astype(np.int64)
    return dict(x=x[keep], y=y[keep], v=np.stack([v0, v1, v2], axis=1)[keep].astype(np.int64), orient=orient[keep])


def triangle_build(xy, count, K=40, min_side=5.0):
    """xy [F, M, 2], count [F] -> (list of F triangle dicts, margin)."""
    margin = Margin()
    xy = np.asarray(xy, np.float64)
    return [triangle_build_frame(xy[f, :max(0, int(count[f]))], K, min_side, margin) for f in range(len(xy))], margin.value


def triangle_set(t):
    """A frame's triangles as a dict (v0, v1, v2, orientation) -> (x, y): the order of the list carries no meaning."""
    return {(int(a), int(b), int(c), int(o)): (float(x), float(y))
            for (a, b, c), o, x, y in zip(t['v'], t['orient'], t['x'], t['y'])}


def _matches_window(ref, tgt, eps, allow_mirror, margin):
    """(indices into ref, indices into tgt) of all matching pairs.  Candidates come from a window in x that is wider than
    eps by more than any rounding; the rule itself is applied to them exactly as the brute force would."""
    if len(ref['x']) == 0 or len(tgt['x']) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    order = np.argsort(ref['x'], kind='stable')
    xs = ref['x'][order]
    wide = eps * (1.0 + 2.0 * MARGIN_CAP) + 1e-300
    lo = np.searchsorted(xs, tgt['x'] - wide, side='left')
    hi = np.searchsorted(xs, tgt['x'] + wide, side='right')
    n = hi - lo
    ti = np.repeat(np.arange(len(tgt['x'])), n)
    ri = order[np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]) if n.sum() else np.zeros(0, np.int64)]
    margin.value = min(margin.value, MARGIN_CAP)
    dx = np.abs(ref['x'][ri] - tgt['x'][ti])
    dy = np.abs(ref['y'][ri] - tgt['y'][ti])
    mx, my = dx <= eps, dy <= eps
    margin.update(dx[my], eps)
    margin.update(dy[mx], eps)
    m = mx & my
    if not allow_mirror:
        m &= ref['orient'][ri] == tgt['orient'][ti]
    return ri[m], ti[m]


def _matches_brute(ref, tgt, eps, allow_mirror, margin):
    dx = np.abs(ref['x'][:, None] - tgt['x'][None, :])
    dy = np.abs(ref['y'][:, None] - tgt['y'][None, :])
    mx, my = dx <= eps, dy <= eps
    margin.update(dx[my], eps)
    margin.update(dy[mx], eps)
    m = mx & my
    if not allow_mirror:
        m &= ref['orient'][:, None] == tgt['orient'][None, :]
    return np.nonzero(m)


def triangle_vote(tris, K=40, eps=0.002, allow_mirror=False, brute=False):
    """tris: the list triangle_build returns -> (votes int32 [F, K, K], margin).  brute=True compares every pair (small K)."""
    margin = Margin()
    votes = np.zeros((len(tris), K, K), np.int32)
    for f in range(1, len(tris)):
        ri, ti = (_matches_brute if brute else _matches_window)(tris[0], tris[f], eps, allow_mirror, margin)
        for c in range(3):
            np.add.at(votes[f], (tris[0]['v'][ri, c], tris[f]['v'][ti, c]), 1)
    return votes, margin.value


# -- nearest neighbours ----------------------------------------------------------------------------------------------------
def apply_affine(A, pts):
    A = np.asarray(A, np.float64)
    x, y = pts[..., 0], pts[..., 1]
    return np.stack([(A[0] * x + A[1] * y) + A[2], (A[3] * x + A[4] * y) + A[5]], axis=-1)


def nearest_match(xy, count, transforms, radius):
    """-> (fwd_idx int32 [F, M], fwd_d2 [F, M], bwd_idx, bwd_d2, margin); finite coordinates only."""
    xy = np.asarray(xy, np.float64)
    F, M = xy.shape[:2]
    margin = Margin()
    r2 = np.float64(radius) * np.float64(radius)
    fwd_idx, bwd_idx = np.full((F, M), -1, np.int32), np.full((F, M), -1, np.int32)
    fwd_d2, bwd_d2 = np.full((F, M), np.inf), np.full((F, M), np.inf)
    n0 = max(0, min(int(count[0]), M))
    for f in range(F):
        nf = max(0, min(int(count[f]), M))
        if n0 == 0 or nf == 0:
            continue
        p = apply_affine(transforms[f], xy[0, :n0])
        s = xy[f, :nf]
        dx, dy = s[None, :, 0] - p[:, None, 0], s[None, :, 1] - p[:, None, 1]
        d2 = dx * dx + dy * dy                                           # [n0, nf]
        for idx_out, d2_out, axis, n in ((fwd_idx, fwd_d2, 1, n0), (bwd_idx, bwd_d2, 0, nf)):
            best = d2.argmin(axis=axis)                                  # the first minimum: the lower index on ties
            bd = np.take_along_axis(d2, np.expand_dims(best, axis), axis).squeeze(axis)
            margin.update(bd, r2)
            ok = bd <= r2
            idx_out[f, :n] = np.where(ok, best, -1)
            d2_out[f, :n] = np.where(ok, bd, np.inf)
    return fwd_idx, fwd_d2, bwd_idx, bwd_d2, margin.value


# -- host procedure --------------------------------------------------------------------------------------------------------
def find_seeds(V):
    """votes [K, K] of one frame -> [n, 2] (reference star, frame star): mutual arg-max pairs (lowest index on ties) that hold
    at least half the largest vote."""
    vmax = int(V.max()) if V.size else 0
    if vmax <= 0:
        return np.zeros((0, 2), np.int64)
    row_best, col_best = V.argmax(axis=1), V.argmax(axis=0)
    i = np.arange(V.shape[0])
    ok = (col_best[row_best] == i) & (V[i, row_best] > 0) & (2 * V[i, row_best].astype(np.int64) >= vmax)
    return np.stack([i[ok], row_best[ok]], axis=1).astype(np.int64)


def fit_transform(r, s, kind):
    """Least-squares s ~ T(r) on coordinates centred on r's mean.  kind: 'similarity', 'mirror' (a similarity after a
    reflection) or 'affine'.  -> (coefficients [6], rms of the 2-D residuals)."""
    r, s = np.asarray(r, np.float64), np.asarray(s, np.float64)
    m = r.mean(axis=0)
    xc, yc = r[:, 0] - m[0], r[:, 1] - m[1]
    one, zero = np.ones_like(xc), np.zeros_like(xc)
    if kind == 'affine':
        D = np.stack([xc, yc, one], axis=1)
        cx = np.linalg.lstsq(D, s[:, 0], rcond=None)[0]
        cy = np.linalg.lstsq(D, s[:, 1], rcond=None)[0]
        lin = np.array([[cx[0], cx[1]], [cy[0], cy[1]]])
        t = np.array([cx[2], cy[2]])
    else:
        if kind == 'similarity':                                         # x' = a x - b y + tx ; y' = b x + a y + ty
            D = np.concatenate([np.stack([xc, -yc, one, zero], axis=1), np.stack([yc, xc, zero, one], axis=1)])
        else:                                                            # x' = a x + b y + tx ; y' = b x - a y + ty
            D = np.concatenate([np.stack([xc, yc, one, zero], axis=1), np.stack([-yc, xc, zero, one], axis=1)])
        a, b, tx, ty = np.linalg.lstsq(D, np.concatenate([s[:, 0], s[:, 1]]), rcond=None)[0]
        lin = np.array([[a, -b], [b, a]]) if kind == 'similarity' else np.array([[a, b], [b, -a]])
        t = np.array([tx, ty])
    t = t - lin @ m
    A = np.array([lin[0, 0], lin[0, 1], t[0], lin[1, 0], lin[1, 1], t[1]])
    res = apply_affine(A, r) - s
    return A, float(np.sqrt(np.mean(res[:, 0] ** 2 + res[:, 1] ** 2)))


def first_fit(r, s, allow_mirror):
    A, rms = fit_transform(r, s, 'similarity')
    kind = 'similarity'
    if allow_mirror:
        Am, rmsm = fit_transform(r, s, 'mirror')
        if rmsm < rms:
            A, rms, kind = Am, rmsm, 'mirror'
    return A, rms, kind


def mutual_pairs(fwd, bwd):
    i = np.nonzero(fwd >= 0)[0]
    i = i[bwd[fwd[i]] == i]
    return np.stack([i, fwd[i]], axis=1).astype(np.int64)


IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])


def register_lists(xy, count, K=40, eps=0.002, min_side=5.0, match_radius=3.0, model='affine', allow_mirror=False,
                   max_rounds=4):
    """-> (dict(coeffs [F, 6], ok, n_seed, n_matched, rms, pairs: list of [n, 2] (reference index, frame index)), margin)."""
    assert model in ('affine', 'similarity')
    xy = np.asarray(xy, np.float64)
    count = np.asarray(count)
    F, M = xy.shape[:2]
    tris, m1 = triangle_build(xy, count, K, min_side)
    votes, m2 = triangle_vote(tris, K, eps, allow_mirror)
    margin = min(m1, m2)
    out = dict(coeffs=np.full((F, 6), np.nan), ok=np.zeros(F, bool), n_seed=np.zeros(F, np.int64), n_matched=np.zeros(F, np.int64),
               rms=np.full(F, np.nan), pairs=[np.zeros((0, 2), np.int64) for _ in range(F)], votes=votes)
    n0 = max(0, min(int(count[0]), M))
    out['coeffs'][0], out['ok'][0], out['rms'][0], out['n_matched'][0] = IDENTITY, True, 0.0, n0
    out['pairs'][0] = np.stack([np.arange(n0), np.arange(n0)], axis=1)
    for f in range(1, F):
        seeds = find_seeds(votes[f])
        out['n_seed'][f] = len(seeds)
        if len(seeds) < 3:
            continue
        A, rms, kind = first_fit(xy[0, seeds[:, 0]], xy[f, seeds[:, 1]], allow_mirror)
        pairs = None
        for rnd in range(max_rounds):
            radius = match_radius if rnd == 0 else float(np.clip(3.0 * rms, 0.5, match_radius))
            T = np.tile(IDENTITY, (2, 1))
            T[1] = A
            fi, _, bi, _, mg = nearest_match(xy[[0, f]], count[[0, f]], T, radius)
            margin = min(margin, mg)
            new = mutual_pairs(fi[1], bi[1])
            if pairs is not None and np.array_equal(new, pairs):
                break
            pairs = new
            if len(pairs) < 3:
                break
            A, rms = fit_transform(xy[0, pairs[:, 0]], xy[f, pairs[:, 1]], 'affine' if model == 'affine' and len(pairs) >= 6 else kind)
        out['n_matched'][f] = len(pairs)
        out['pairs'][f] = pairs
        if len(pairs) >= max(3, len(seeds)):
            out['coeffs'][f], out['ok'][f], out['rms'][f] = A, True, rms
    return out, margin


# -- synthetic fields --------------------------------------------------------------------------------------------------------
def make_affine(rot_deg=0.0, scale=1.0, shift=(0.0, 0.0), shear=0.0, mirror=False, centre=(1023.5, 1023.5)):
    """Rotation by rot_deg and scale about `centre`, then `shift`; shear adds shear * y to x before the rotation; mirror flips x
    about the centre first."""
    th = np.deg2rad(rot_deg)
    R = scale * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    L = R @ np.array([[1.0, shear], [0.0, 1.0]]) @ (np.diag([-1.0, 1.0]) if mirror else np.eye(2))
    c = np.asarray(centre, np.float64)
    t = c - L @ c + np.asarray(shift, np.float64)
    return np.array([L[0, 0], L[0, 1], t[0], L[1, 0], L[1, 1], t[1]])


def make_field(seed, A, n=300, size=2048, common=0.55, sigma=0.1, jitter=3, extent=None):
    """Two brightness-ordered lists of one sky, drawn 300 px beyond the image on every side so that a moderately shifted or
    rotated frame is filled too.  Each frame sees a star with probability `common`, so about that share of a list is in the
    other one; the brightness ranks are jittered by a few places and the positions by Gaussian noise sigma.
    -> (ref [n0, 2], frame [n1, 2], truth pairs [m, 2], sigma)."""
    rng = np.random.default_rng(seed)
    big = 6 * n
    lo, hi = (-300.0, size + 300.0) if extent is None else extent
    sky = rng.uniform(lo, hi, size=(big, 2))
    mag = rng.permutation(big).astype(np.float64)                        # brightness rank on the sky
    frames = []
    for which in range(2):
        pos = sky if which == 0 else apply_affine(A, sky)
        inside = (pos[:, 0] >= 0) & (pos[:, 0] <= size - 1) & (pos[:, 1] >= 0) & (pos[:, 1] <= size - 1)
        seen = inside & (rng.uniform(size=big) < common)
        ids = np.nonzero(seen)[0]
        rank = mag[ids] + rng.uniform(-jitter, jitter, size=len(ids)) * 2.5
        ids = ids[np.argsort(rank, kind='stable')][:n]
        frames.append((ids, pos[ids] + rng.normal(0.0, sigma, size=(len(ids), 2))))
    (id0, p0), (id1, p1) = frames
    where1 = {int(s): j for j, s in enumerate(id1)}
    truth = np.array([[i, where1[int(s)]] for i, s in enumerate(id0) if int(s) in where1], np.int64).reshape(-1, 2)
    return p0, p1, truth, sigma


def pad_lists(lists, M=None):
    """lists of [n, 2] -> (xy [F, M, 2] zero-padded, count [F] int32)."""
    M = M or max(1, max(len(a) for a in lists))
    xy = np.zeros((len(lists), M, 2))
    for f, a in enumerate(lists):
        xy[f, :len(a)] = np.asarray(a, np.float64).reshape(-1, 2)
    return xy, np.array([len(a) for a in lists], np.int32)


def corner_error(A, B, size=2048):
    """The largest distance between the images of the four corners under the maps A and B."""
    c = np.array([[0.0, 0.0], [size - 1.0, 0.0], [0.0, size - 1.0], [size - 1.0, size - 1.0]])
    return float(np.sqrt(((apply_affine(A, c) - apply_affine(B, c)) ** 2).sum(axis=1)).max())
