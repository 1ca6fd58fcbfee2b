"""F3 - an independent statement of the affine Lanczos-3 resample (host only: NumPy + Python integers).

Written from the definition in the header comment of csrc/resample.hip and DESIGN 4.4, not from oracle/apref.c:

    F[k] = A[k] * 2^32 rounded to the nearest integer, ties to even (llrint in the default rounding mode);
    X = F0 u + F1 v + F2, Y = F3 u + F4 v + F5 as exact integers for the (fine) output pixel (u, v);
    ix = floor(X / 2^32) (an arithmetic shift: also for negative X), fraction fr = X mod 2^32,
    phase px = (fr + 2^(sh-1)) >> sh with sh = 32 - log2(n_phases): the top bits of the fraction, rounded, 0 .. n_phases;
    the 6 x 6 window of taps ix-2 .. ix+3, iy-2 .. iy+3 weighted by the table rows lut[px], lut[py];
    value = fs * (wy . win . wx), fs = fscale[f], under conserve_flux times |A0 A4 - A1 A3| (float64) rounded to float32;
    a pixel is DEFINED when all 36 taps are inside the frame, unmasked and finite, and its 64 x 16 output tile is sane:
    every coefficient finite and below 2^30 in magnitude and the float64 coordinates fma(A0, x, fma(A1, y, A2)) of the
    tile's four corner pixels strictly inside +-1e9;
    OVERSAMPLING n: the transform is that of the n-times finer grid (fine_affines below), an output pixel is the mean of
    its n x n sub-samples.

The model evaluates the window sum in float64 (the library's float32 table rows widened), so it has no float32 rounding
of its own except that of fs; beside the value it returns the error scale S = |fs| (|wy| . |win| . |wx|), the quantity a
float32 evaluation's rounding error is proportional to.

classify_tiles() is a different thing: it RESTATES the tile rule of resample_tiles_kernel (csrc/resample_core.h) so that
tests can assert which code path their cases reach.  It never decides what is correct."""
from fractions import Fraction

import numpy as np

TILE_W, TILE_H = 64, 16
U = 2.0 ** -24                     # unit roundoff of float32


def lanczos3_table_f64(n_phases):
    """[n_phases + 1, 6] float64: row p = Lanczos-3 weights L(d) = sinc(d) sinc(d / 3) of the taps at d = k - 2 - p / n_phases,
    k = 0 .. 5, normalised to sum 1 per row.  Whole-pixel offsets (rows 0 and n_phases) are set from the closed form - L(0) = 1,
    L(integer) = 0 - instead of sin(pi k) ~ 1e-17."""
    n = int(n_phases)
    t = np.arange(n + 1, dtype=np.float64)[:, None] / n
    d = np.arange(6, dtype=np.float64)[None, :] - 2.0 - t
    with np.errstate(invalid='ignore', divide='ignore'):
        pd = np.pi * d
        w = np.where(d == 0.0, 1.0, 3.0 * np.sin(pd) * np.sin(pd / 3.0) / (pd * pd))
    w[np.abs(d) >= 3.0] = 0.0
    w[0] = [0, 0, 1, 0, 0, 0]
    w[n] = [0, 0, 0, 1, 0, 0]
    return w / w.sum(axis=1, keepdims=True)


def fine_affines(affines, n):
    """The transform of the n-times finer grid, as ops.oversampled_affines documents it: fine pixel (u, v) has its centre at
    output coordinates ((u + 0.5) / n - 0.5, (v + 0.5) / n - 0.5).  float64 arithmetic in the documented order."""
    a = np.asarray(affines, np.float64).reshape(-1, 6)
    off = 0.5 / n - 0.5
    f = a.copy()
    f[:, 0] = a[:, 0] / n
    f[:, 1] = a[:, 1] / n
    f[:, 2] = a[:, 2] + (a[:, 0] + a[:, 1]) * off
    f[:, 3] = a[:, 3] / n
    f[:, 4] = a[:, 4] / n
    f[:, 5] = a[:, 5] + (a[:, 3] + a[:, 4]) * off
    return f


def _fma(a, b, c):
    """float64 fma(a, b, c): the exact a * b + c rounded once."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all='ignore'):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    try:
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    except OverflowError:
        return float('inf')


def fixed_point(a, ties='even'):
    """F = A * 2^32 rounded to an integer, ties to even.  ties='away' is a deliberately wrong variant (perturbation tests)."""
    q = Fraction(float(a)) * (1 << 32)
    if ties == 'even':
        return int(round(q))                                   # Python rounds a Fraction half to even
    fl = q.numerator // q.denominator
    r = q - fl
    if r == Fraction(1, 2):
        return fl + 1 if q > 0 else fl                        # away from zero
    return fl + 1 if r > Fraction(1, 2) else fl


def tile_sane(A, x0, y0, w_out, h_out, os=1):
    """The defined-tile rule for the 64 x 16 output tile at (x0, y0)."""
    A = [float(v) for v in A]
    if not all(np.isfinite(v) and abs(v) < 2.0 ** 30 for v in A):
        return False
    xl, yl = min(x0 + TILE_W - 1, w_out - 1), min(y0 + TILE_H - 1, h_out - 1)
    xa, xb, ya, yb = x0 * os, xl * os + os - 1, y0 * os, yl * os + os - 1
    # far from the limit the plain float64 evaluation (within ~1e-6 of the fused one here) decides; near it, the exact one
    far = max(abs(A[0]) * xb + abs(A[1]) * yb + abs(A[2]), abs(A[3]) * xb + abs(A[4]) * yb + abs(A[5]))
    if far < 9.99e8:
        return True
    for cx, cy in ((xa, ya), (xb, ya), (xa, yb), (xb, yb)):
        xi = _fma(A[0], cx, _fma(A[1], cy, A[2]))
        yi = _fma(A[3], cx, _fma(A[4], cy, A[5]))
        if not (-1e9 < xi < 1e9 and -1e9 < yi < 1e9):
            return False
    return True


def _coords(F, u, v):
    """X = F0 u + F1 v + F2: int64 where no partial sum can overflow, Python integers (wrapped to 64 bits at the end) otherwise."""
    umax, vmax = int(np.abs(u).max()), int(np.abs(v).max())
    out = []
    for k in (0, 3):
        if abs(F[k]) * umax + abs(F[k + 1]) * vmax + abs(F[k + 2]) < (1 << 62):
            out.append(np.int64(F[k]) * u[None, :] + np.int64(F[k + 1]) * v[:, None] + np.int64(F[k + 2]))
        else:
            uo, vo = u.astype(object), v.astype(object)
            X = F[k] * uo[None, :] + F[k + 1] * vo[:, None] + F[k + 2]
            # 64-bit two's-complement sums, as the definition says: a sane tile's true sums fit, the wrap touches undefined tiles only
            X = (X + (1 << 63)) % (1 << 64) - (1 << 63)
            out.append(X.astype(np.int64))
    return out


def _split(X, sh, perturb):
    """integer part and phase of 32.32 fixed-point coordinates"""
    if perturb == 'floor_to_zero':
        # the window's first tap ix - 2 from a division that rounds towards zero: wrong exactly where X - 2 * 2^32 is negative,
        # which is where "ix - 2 >= 0" is decided (a defined pixel has X >= 2 * 2^32, so nothing else can show this mistake)
        Xs = X - (np.int64(2) << 32)
        ix = np.where(Xs < 0, -((-Xs) >> 32), Xs >> 32) + 2
    else:
        ix = X >> 32                                           # arithmetic: floor, also below zero
    fr = X & np.int64(0xffffffff)
    if perturb == 'phase_trunc':
        p = fr >> sh
    else:
        p = (fr + (np.int64(1) << (sh - 1))) >> sh
    if perturb == 'phase_plus_one':
        p = np.minimum(p + 1, np.int64(1) << (32 - sh))
    return ix, p


def resample_model(frames, affines, fscale=None, mask=None, out_shape=None, n_phases=1024, lut=None, conserve_flux=False,
                   oversampling=1, perturb=None):
    """-> (defined [N,h,w] bool, value [N,h,w] float64 (NaN where not defined), S [N,h,w] float64).

    frames [N,H,W] or [H,W] float32; affines [N,6] or one per 64 x 16 output tile [N,ty,tx,6] (float64); with oversampling n > 1
    they are the FINE grid's transforms (fine_affines) and fscale is applied as given; value is then the float64 mean of the
    n x n sub-sample values in row-major order (np.float32(value) is the definition's single rounding), S the mean of theirs.
    lut: the float32 table to widen (default: lanczos3_table_f64 rounded to float32).
    perturb: None, or one deliberately WRONG variant - 'phase_plus_one', 'phase_trunc', 'swap_wx_wy', 'floor_to_zero',
    'ties_away' - used to show that a comparison against the model can see such a mistake."""
    frames = np.asarray(frames, np.float32)
    if frames.ndim == 2:
        frames = frames[None]
    N, H, W = frames.shape
    h, w = (H, W) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
    os = int(oversampling)
    A = np.asarray(affines, np.float64)
    per_tile = A.ndim == 4
    ty, tx = -(-h // TILE_H), -(-w // TILE_W)
    if per_tile:
        assert A.shape == (N, ty, tx, 6)
    else:
        A = A.reshape(-1, 6)
        if A.shape[0] == 1 and N > 1:
            A = np.repeat(A, N, 0)
        assert A.shape == (N, 6)
    n_phases = int(n_phases)
    log2p = n_phases.bit_length() - 1
    assert n_phases >= 2 and (1 << log2p) == n_phases
    sh = 32 - log2p
    lut64 = (lanczos3_table_f64(n_phases).astype(np.float32) if lut is None else np.asarray(lut, np.float32)).astype(np.float64)
    assert lut64.shape == (n_phases + 1, 6)
    fsc = np.ones(N, np.float32) if fscale is None else np.asarray(fscale, np.float32).reshape(-1)
    if fsc.size == 1 and N > 1:
        fsc = np.repeat(fsc, N)
    ties = 'away' if perturb == 'ties_away' else 'even'

    defined = np.zeros((N, h, w), bool)
    value = np.full((N, h, w), np.nan)
    S = np.full((N, h, w), np.nan)
    for f in range(N):
        src = frames[f].astype(np.float64)
        bad = ~np.isfinite(frames[f])
        if mask is not None:
            bad |= np.asarray(mask) != 0
        # bad pixels in the 6 x 6 window starting at (r, c): a summed-area table
        sat = np.zeros((H + 1, W + 1), np.int64)
        sat[1:, 1:] = np.cumsum(np.cumsum(bad, 0, dtype=np.int64), 1)
        src = np.where(bad, 0.0, src)
        # regions that share one transform: the frame, or one tile; a region is processed in bands of output rows
        regions = [(j, i) for j in range(ty) for i in range(tx)] if per_tile else [None]
        for reg in regions:
            if reg is None:
                a, y_lo, y_hi, x_lo, x_hi = A[f], 0, h, 0, w
            else:
                a = A[f, reg[0], reg[1]]
                y_lo, y_hi = reg[0] * TILE_H, min(reg[0] * TILE_H + TILE_H, h)
                x_lo, x_hi = reg[1] * TILE_W, min(reg[1] * TILE_W + TILE_W, w)
            if not all(np.isfinite(a)) or max(abs(a)) >= 2.0 ** 30:
                continue
            sane = np.zeros((ty, tx), bool)
            for j in range(y_lo // TILE_H, -(-y_hi // TILE_H)):
                for i in range(x_lo // TILE_W, -(-x_hi // TILE_W)):
                    sane[j, i] = tile_sane(a, i * TILE_W, j * TILE_H, w, h, os)
            if not sane.any():
                continue
            F = [fixed_point(v, ties) for v in a]
            with np.errstate(all='ignore'):
                det = abs(_fma(a[0], a[4], -(a[1] * a[3])))     # the definition's order: the product a1 a3 rounded, then one fma
                fs = float(np.float32(np.float64(fsc[f]) * det)) if conserve_flux else float(fsc[f])
            band = max(1, 65536 // max(1, (x_hi - x_lo) * os * os))
            for yb in range(y_lo, y_hi, band):
                ye = min(yb + band, y_hi)
                ys, xs = np.arange(yb, ye), np.arange(x_lo, x_hi)
                ok_tile = sane[ys // TILE_H][:, xs // TILE_W]
                if not ok_tile.any():
                    continue
                acc = np.zeros((ye - yb, x_hi - x_lo))
                accS = np.zeros_like(acc)
                good = ok_tile.copy()
                for sa in range(os):                            # sub-samples in row-major order
                    for sb in range(os):
                        X, Y = _coords(F, xs * os + sb, ys * os + sa)
                        ix, px = _split(X, sh, perturb)
                        iy, py = _split(Y, sh, perturb)
                        inside = (ix >= 2) & (ix <= W - 4) & (iy >= 2) & (iy <= H - 4)
                        cx, cy = np.where(inside, ix - 2, 0), np.where(inside, iy - 2, 0)
                        nbad = sat[cy + 6, cx + 6] - sat[cy, cx + 6] - sat[cy + 6, cx] + sat[cy, cx]
                        good &= inside & (nbad == 0)
                        wx, wy = lut64[px], lut64[py]           # [rows, cols, 6]
                        if perturb == 'swap_wx_wy':
                            wx, wy = wy, wx
                        win = src[(cy[..., None] + np.arange(6))[..., :, None], (cx[..., None] + np.arange(6))[..., None, :]]
                        acc += fs * np.einsum('rcj,rcji,rci->rc', wy, win, wx)
                        accS += abs(fs) * np.einsum('rcj,rcji,rci->rc', np.abs(wy), np.abs(win), np.abs(wx))
                defined[f, yb:ye, x_lo:x_hi] = good
                value[f, yb:ye, x_lo:x_hi] = np.where(good, acc / (os * os), np.nan)
                S[f, yb:ye, x_lo:x_hi] = np.where(good, accS / (os * os), np.nan)
    return defined, value, S


# ---- the error bound ---------------------------------------------------------------------------------------------------
def rounding_count(conserve_flux):
    """The number of float32 roundings on the longest path of the stated evaluation order, from a tap to the result:
       3  a row's even (or odd) chain: the product wx0 s0, then two fmaf           e = fmaf(wx4, s4, fmaf(wx2, s2, wx0 s0))
       6  the chain over the rows: the product wy0 e0, then five fmaf
       1  the join of the even and the odd half, ve + vo
       1  the multiplication by fs
     = 11, plus 1 under conserve_flux for the float32 rounding of fs itself = 12.
    Every rounding is relative to a partial sum bounded by the sum of the magnitudes, so the error is at most
    gamma_c S with gamma_c = c u / (1 - c u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1)."""
    return 11 + (1 if conserve_flux else 0)


def bound(S, conserve_flux):
    c = rounding_count(conserve_flux)
    return (c * U / (1.0 - c * U)) * S


# ---- the tile rule, restated -------------------------------------------------------------------------------------------
FAST, STAGED_INTERIOR, STAGED_BORDER, GATHER, NOT_SANE = 'fast', 'staged_interior', 'staged_border', 'gather', 'not_sane'


def classify_tiles(affines, in_shape, out_shape, n_phases=1024, oversampling=1, mask=None, th=None):
    """Which path resample_tiles_kernel gives every WORKGROUP tile - a restatement of the tile rule in csrc/resample_core.h, written
    to let tests assert that their cases reach the paths they were built for.  It was NOT confirmed against the device (the tile
    records live in a workspace the library owns), so it is used for coverage assertions only and never decides what is correct.

    affines [N,6] or [N,ty,tx,6] (of the fine grid when oversampling); th: output rows per workgroup (default: the launcher's
    choice - 32 with one transform per frame and more than 16 output rows, else 16; the fused resample + clip kernels use 16).
    -> list of dicts per tile: frame, tx, ty, th, cls, w, h, bx0, by0, steady, inline_mask, sane_top, sane_bot."""
    H, W = in_shape
    h, w = out_shape
    os = int(oversampling)
    A = np.asarray(affines, np.float64)
    per_tile = A.ndim == 4
    if not per_tile:
        A = A.reshape(-1, 6)
    N = A.shape[0]
    if th is None:
        th = 2 * TILE_H if (not per_tile and h > TILE_H) else TILE_H
    assert th == TILE_H or not per_tile
    gx, gy = -(-w // TILE_W), -(-h // th)
    sh = 32 - (int(n_phases).bit_length() - 1)
    has_mask = mask is not None
    scatter = has_mask and not per_tile
    overflow = has_mask and int(np.count_nonzero(mask)) > min(max(H * W // 64, 256), 1 << 20)
    out = []
    for f in range(N):
        for tyi in range(gy):
            for txi in range(gx):
                a = A[f, tyi, txi] if per_tile else A[f]
                x0, y0 = txi * TILE_W, tyi * th
                sane_top = tile_sane(a, x0, y0, w, h, os)
                has_bot = th > TILE_H and y0 + TILE_H < h
                sane_bot = tile_sane(a, x0, y0 + TILE_H, w, h, os) if has_bot else sane_top
                coef_ok = all(np.isfinite(v) and abs(v) < 2.0 ** 30 for v in a)
                rec = dict(frame=f, tx=txi, ty=tyi, th=th, cls=NOT_SANE, w=0, h=0, bx0=0, by0=0, steady=False, sane_top=sane_top,
                           sane_bot=sane_bot, inline_mask=False)
                if has_mask:
                    with np.errstate(all='ignore'):
                        det = abs(a[0] * a[4] - a[1] * a[3])
                        ok = coef_ok and det > 1e-300 and 3 * (abs(a[4]) + abs(a[1])) <= 24 * det and 3 * (abs(a[3]) + abs(a[0])) <= 24 * det
                    rec['inline_mask'] = bool(not (scatter and ok) or overflow)
                if sane_top and sane_bot:
                    F = [fixed_point(v) for v in a]
                    xl = min(x0 + TILE_W - 1, w - 1)
                    yl = min(y0 + th - 1, h - 1) if has_bot else min(y0 + TILE_H - 1, h - 1)
                    ua, ub, va, vb = x0 * os, xl * os + os - 1, y0 * os, yl * os + os - 1
                    jx = [(F[0] * u + F[1] * v + F[2]) >> 32 for u, v in ((ua, va), (ub, va), (ua, vb), (ub, vb))]
                    jy = [(F[3] * u + F[4] * v + F[5]) >> 32 for u, v in ((ua, va), (ub, va), (ua, vb), (ub, vb))]
                    bx0, by0 = min(jx) - 2, min(jy) - 2
                    wl, hl = max(jx) - min(jx) + 6, max(jy) - min(jy) + 6
                    rec.update(w=wl, h=hl, bx0=bx0, by0=by0)
                    if wl * hl <= 4096:
                        interior = bx0 >= 0 and by0 >= 0 and bx0 + wl <= W and by0 + hl <= H and y0 + th <= h
                        if interior and wl <= 80 and hl <= th + 10:
                            rec['cls'] = FAST
                            fr4 = F[4] & 0xffffffff
                            dist = fr4 if fr4 < (1 << 31) else (1 << 32) - fr4
                            rec['steady'] = os == 1 and dist * (th // 4 - 1) < (1 << sh)
                        else:
                            rec['cls'] = STAGED_INTERIOR if interior else STAGED_BORDER
                    else:
                        rec['cls'] = GATHER
                out.append(rec)
    return out


def count_tiles(tiles, **want):
    """number of tile records whose fields equal the given values (a value may be a set / tuple of accepted values)"""
    n = 0
    for t in tiles:
        if all((t[k] in v) if isinstance(v, (set, tuple, list, frozenset)) else (t[k] == v) for k, v in want.items()):
            n += 1
    return n


# ---- comparing a float32 result with the model -------------------------------------------------------------------------
def compare(got, model, conserve_flux=False, what='', mean_rounding=False):
    """Assert that `got` [N,h,w] float32 (NaN = undefined) has exactly the model's defined plane and lies within the derived
    bound of the model's value on EVERY defined pixel; mean_rounding adds the one float32 rounding of an oversampled pixel's
    mean.  Returns the largest |got - value| / (2^-24 S), for the record."""
    defined, value, S = model
    got = np.asarray(got)
    gd = ~np.isnan(got)
    assert np.array_equal(gd, defined), '%s: defined planes differ at %s' % (what, np.argwhere(gd != defined)[:5].tolist())
    if not defined.any():
        return 0.0
    g, v, s = got[defined].astype(np.float64), value[defined], S[defined]
    tol = bound(s, conserve_flux)
    if mean_rounding:
        tol = tol + U * np.abs(v) * (1.0 + 2.0 * U)
    err = np.abs(g - v)
    worst = int(np.argmax(err - tol))
    assert err[worst] <= tol[worst], '%s: |got - model| = %.4g exceeds the bound %.4g (%.2f x 2^-24 S) at defined pixel #%d' % (
        what, err[worst], tol[worst], err[worst] / (U * s[worst]), worst)
    return float((err / (U * s)).max())


# ---- transforms for the test cases -------------------------------------------------------------------------------------
def affine(in_shape, out_shape, deg=0.0, sx=1.0, sy=None, shear=0.0, shift=(0.37, 0.21), flip_x=False, flip_y=False):
    """Rotation by deg after a scale (sx, sy) and an x flip / y flip, plus `shear` input rows per output column; the output's
    centre maps to the input's centre + shift."""
    sy = sx if sy is None else sy
    th = np.deg2rad(deg)
    c, s = np.cos(th), np.sin(th)
    if deg % 90 == 0:
        c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][int(deg // 90) % 4]
    m = np.array([[c, -s], [s, c]]) @ np.diag([-sx if flip_x else sx, -sy if flip_y else sy])
    m[1, 0] += shear
    cin = np.array([(in_shape[1] - 1) / 2.0 + shift[0], (in_shape[0] - 1) / 2.0 + shift[1]])
    cout = np.array([(out_shape[1] - 1) / 2.0, (out_shape[0] - 1) / 2.0])
    t = cin - m @ cout
    return np.array([m[0, 0], m[0, 1], t[0], m[1, 0], m[1, 1], t[1]], np.float64)


def tie_transforms(n_phases=1024):
    """Coefficients whose product with 2^32 is an exact tie: 2^-33 -> 0.5 (to even: 0), 3 * 2^-33 -> 1.5 (to even: 2),
    1 + 5 * 2^-33 -> 2^32 + 2.5 (to even: + 2), 1 - 2^-33; the offsets sit on a phase boundary so that one unit of 2^-32 shows."""
    n = n_phases
    return np.array([[1, -2.0 ** -33, 3 + 0.5 / n, 3 * 2.0 ** -33, 1 + 5 * 2.0 ** -33, 2 + 0.5 / n - 2.5 * 2.0 ** -32],
                     [1 - 2.0 ** -33, 2.0 ** -33, 3 + 1.5 / n - 2.0 ** -32, -2.0 ** -33, 1, 2 + 2.5 / n]], np.float64)


def per_tile_copies(A, out_shape):
    """[N,6] -> [N,ty,tx,6]: every 64 x 16 tile carries its frame's transform (the per-tile form runs 16-row workgroups)"""
    A = np.asarray(A, np.float64).reshape(-1, 6)
    ty, tx = -(-out_shape[0] // TILE_H), -(-out_shape[1] // TILE_W)
    return np.ascontiguousarray(np.broadcast_to(A[:, None, None, :], (A.shape[0], ty, tx, 6)))


def sweep(make, params, in_shape, out_shape, keep, per_tile=False, limit=10, oversampling=1):
    """the transforms make(p) whose tiles (by classify_tiles, of the fine grid when oversampling) satisfy keep(tile) for at least one
    tile; at most `limit`, spread evenly"""
    hits = []
    for p in params:
        a = make(p)
        b = fine_affines(a, oversampling)[0] if oversampling > 1 else a
        tiles = classify_tiles(per_tile_copies(b, out_shape) if per_tile else b[None], in_shape, out_shape, oversampling=oversampling)
        if any(keep(t) for t in tiles):
            hits.append(a)
    if len(hits) > limit:
        hits = [hits[i] for i in np.unique(np.linspace(0, len(hits) - 1, limit).round().astype(int))]
    return np.array(hits, np.float64).reshape(-1, 6)


def footprint_limit_set(in_shape, out_shape, per_tile, oversampling=1, limit=8):
    """Transforms whose tiles sit on the fast path's footprint limits: rotations of both signs and shears with footprints
    th + 9 .. th + 11 rows tall, x scales with footprints 79 .. 81 columns wide.  Chosen by classify_tiles from fine sweeps (of the
    fine grid's footprints when oversampling: the sub-pixel centres reach a little further than the pixel centres)."""
    th = TILE_H if (per_tile or out_shape[0] <= TILE_H) else 2 * TILE_H
    tall = lambda t: t['cls'] in (FAST, STAGED_INTERIOR) and t['h'] in (th + 9, th + 10, th + 11)
    wide = lambda t: t['cls'] in (FAST, STAGED_INTERIOR) and t['w'] in (79, 80, 81) and t['h'] <= th + 10
    kw = dict(per_tile=per_tile, oversampling=oversampling)
    half = max(2, limit // 2)
    sets = []
    for sign in (1, -1):
        sets.append(sweep(lambda d: affine(in_shape, out_shape, deg=sign * d), np.arange(0.5, 9.0, 0.05), in_shape, out_shape, tall, limit=limit, **kw))
    sets.append(sweep(lambda k: affine(in_shape, out_shape, shear=k), np.arange(0.0, 0.25, 0.002), in_shape, out_shape, tall, limit=max(half, 6 * limit // 8), **kw))
    sets.append(sweep(lambda k: affine(in_shape, out_shape, shear=-k), np.arange(0.0, 0.25, 0.002), in_shape, out_shape, tall, limit=half, **kw))
    sets.append(sweep(lambda s: affine(in_shape, out_shape, sx=s, sy=1.0), np.arange(1.10, 1.32, 0.002), in_shape, out_shape, wide, limit=limit, **kw))
    return np.concatenate(sets, 0)


def area_limit_set(in_shape, out_shape, th, oversampling=1, limit=4):
    """Minifying transforms whose footprints sit on both sides of the staged path's 4096 floats: about 32 rows tall, x scales swept
    across 128 columns; `limit` transforms that hold a footprint of 4095 or 4096 floats and `limit` that hold one of 4097 .. 4224."""
    n = oversampling
    make = lambda p: affine(in_shape, out_shape, sx=p[0], sy=p[1] / (th - 1 + (n - 1.0) / n))
    at = lambda t: t['w'] * t['h'] in (4095, 4096)
    above = lambda t: 4097 <= t['w'] * t['h'] <= 4224
    per_tile = th == TILE_H and out_shape[0] > TILE_H
    params = [(sx, q) for q in (26.5, 26.2, 26.8) for sx in np.linspace(119.0 / 63, 125.0 / 63, 61)]
    a = sweep(make, params, in_shape, out_shape, at, per_tile, limit, n)
    b = sweep(make, params, in_shape, out_shape, above, per_tile, limit, n)
    return np.concatenate([a, b], 0)
