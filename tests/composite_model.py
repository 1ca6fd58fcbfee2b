"""NumPy model of the colour composite (F9 ApComposite; DESIGN 4.3f, PARITY UNPINNED: STIFF is absent, the arithmetic is the
project's own definition).  Written from that definition, not from the kernel: float32 arrays, one rounding per operation, the
tone table indexed through view(np.uint32).  tests/test_composite_model_host.py holds it to np.quantile and to a float64
evaluation with pow; tests/test_gpu_composite.py holds the kernels to it, bit for bit."""
import numpy as np

OCTAVES, KNOTS = 40, 256
TABLE_LEN = OCTAVES * KNOTS + 1
F32 = np.float32


# -- levels ---------------------------------------------------------------------------------------------------------
def _keys(v):
    """Order-preserving uint32 keys of float32 values: -0.0 sorts below +0.0."""
    b = np.ascontiguousarray(v, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def _value(key):
    key = np.uint32(key)
    b = (key & np.uint32(0x7fffffff)) if key & np.uint32(0x80000000) else ~key
    return np.array([b], np.uint32).view(F32)[0]


def quantile_levels(planes, q, manual=None):
    """levels float32 [3, 2] and n_finite int64 [3]: the level of q is v[floor(q (n - 1))] of the channel's finite values in
    ascending order (the product in float64; np.quantile method='lower'), NaN when there is none; a manual entry that is not
    NaN replaces the level."""
    planes = np.asarray(planes, F32)
    q = np.broadcast_to(np.asarray(q, np.float64), (3, 2))
    levels = np.full((3, 2), np.nan, F32)
    n_finite = np.zeros(3, np.int64)
    for c in range(3):
        v = planes[c].ravel()
        k = np.sort(_keys(v[np.isfinite(v)]))
        n = n_finite[c] = k.size
        for t in range(2):
            if n:
                levels[c, t] = _value(k[int(np.floor(q[c, t] * np.float64(n - 1)))])
            if manual is not None and not np.isnan(F32(np.asarray(manual, F32).reshape(3, 2)[c, t])):
                levels[c, t] = np.asarray(manual, F32).reshape(3, 2)[c, t]
    return levels, n_finite


# -- tone table -----------------------------------------------------------------------------------------------------
def tone_table(gamma=2.2, gamma_fac=1.0):
    """G(Y) = T(Y) / Y, T(Y) = Y^(1 / (gamma gamma_fac)), in float64 at the knots 2^e (1 + m / 256), e = -40 .. -1, m = 0 .. 255,
    and at Y = 1; rounded once to float32."""
    g = float(gamma) * float(gamma_fac)
    y = np.array([2.0 ** e * (1.0 + m / 256.0) for e in range(-OCTAVES, 0) for m in range(KNOTS)] + [1.0], np.float64)
    return (np.power(y, 1.0 / g) / y).astype(F32)


def table_lookup(table, Y):
    """G by the bits of Y (float32 array): cell = offset exponent and top 8 mantissa bits, t = the low 15 bits 2^-15,
    G[i] + t (G[i + 1] - G[i]); Y > 1 uses Y = 1 (t = 0 there, so the knot after the closing one is never needed);
    Y < 2^-40: 0."""
    Y = np.asarray(Y, F32)
    tiny = ~(Y >= F32(2.0 ** -40))
    yl = np.where(Y > F32(1), F32(1), np.where(tiny, F32(1), Y)).astype(F32)
    b = yl.view(np.uint32)
    i = (b >> np.uint32(15)).astype(np.int64) - ((127 - OCTAVES) << 8)
    t = (b & np.uint32(0x7fff)).astype(F32) * F32(2.0 ** -15)
    g0 = table[i]
    g1 = table[np.minimum(i + 1, TABLE_LEN - 1)]
    d = (g1 - g0).astype(F32)
    G = (g0 + (t * d).astype(F32)).astype(F32)
    return np.where(tiny, F32(0), G).astype(F32)


# -- composite ------------------------------------------------------------------------------------------------------
def _pos(a):
    return np.where(a > 0, a, F32(0)).astype(F32)           # max(a, 0) with NaN -> 0


def composite_rgb(planes, levels, tables, colour_sat, bits=8, flip=True):
    """out [V, H, W, 3] uint8 / uint16 from planes [3, H, W] float32, levels [3, 2], tables [V, TABLE_LEN], colour_sat [V]."""
    planes = np.asarray(planes, F32)
    levels = np.asarray(levels, F32).reshape(3, 2)
    tables = np.asarray(tables, F32).reshape(-1, TABLE_LEN)
    sat = np.asarray(colour_sat, F32).reshape(-1)
    maxv = F32(2 ** bits - 1)
    src = planes[:, ::-1] if flip else planes
    with np.errstate(all='ignore'):
        s = []
        for c in range(3):
            lo, hi = levels[c]
            scale = F32(1) / F32(hi - lo) if hi > lo else F32(0)        # NaN levels compare false
            s.append(_pos(((src[c] - lo).astype(F32) * scale).astype(F32)))
        Y = (((s[0] + s[1]).astype(F32) + s[2]).astype(F32) * F32(1.0 / 3.0)).astype(F32)
        black = ~(np.isfinite(src[0]) & np.isfinite(src[1]) & np.isfinite(src[2]))
        out = np.zeros((len(sat),) + Y.shape + (3,), np.uint8 if bits == 8 else np.uint16)
        for v in range(len(sat)):
            G = table_lookup(tables[v], Y)
            for c in range(3):
                cc = _pos((Y + (sat[v] * (s[c] - Y).astype(F32)).astype(F32)).astype(F32))
                o = (cc * G).astype(F32)
                o = np.where(o < F32(1), o, F32(1)).astype(F32)          # min(o, 1) with NaN -> 1
                pix = ((o * maxv).astype(F32) + F32(0.5)).astype(F32).astype(np.uint32)
                out[v, ..., c] = np.where(black, 0, pix)
    return out


def composite_direct(planes, levels, gamma, gamma_fac, colour_sat, bits=8, flip=True):
    """The same formulas evaluated directly in float64 with pow in place of the table (one variant): what the table and the
    float32 roundings are held against, to within one count."""
    planes = np.asarray(planes, np.float64)
    levels = np.asarray(levels, np.float64).reshape(3, 2)
    src = planes[:, ::-1] if flip else planes
    g = float(gamma) * float(gamma_fac)
    with np.errstate(all='ignore'):
        s = []
        for c in range(3):
            lo, hi = levels[c]
            scale = 1.0 / (hi - lo) if hi > lo else 0.0
            s.append(np.maximum((src[c] - lo) * scale, 0.0))
        Y = (s[0] + s[1] + s[2]) / 3.0
        Yl = np.minimum(Y, 1.0)
        G = np.where(Yl >= 2.0 ** -40, np.power(Yl, 1.0 / g) / np.where(Yl > 0, Yl, 1.0), 0.0)
        black = ~(np.isfinite(src[0]) & np.isfinite(src[1]) & np.isfinite(src[2]))
        out = np.zeros(Y.shape + (3,), np.int64)
        for c in range(3):
            o = np.minimum(np.maximum(Y + colour_sat * (s[c] - Y), 0.0) * G, 1.0)
            out[..., c] = np.where(black, 0, np.floor(np.nan_to_num(o) * (2 ** bits - 1) + 0.5)).astype(np.int64)
    return out


# -- test data ------------------------------------------------------------------------------------------------------
def star_field(shape, seed, n_stars=None, dither=(0.0, 0.0)):
    """Three float32 planes of a seeded star field: sky + noise + Gaussian stars whose colours differ."""
    rng = np.random.default_rng(seed)
    H, W = shape
    n_stars = n_stars if n_stars is not None else max(3, H * W // 400)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    xs, ys = rng.uniform(0, W, n_stars) + dither[0], rng.uniform(0, H, n_stars) + dither[1]
    amp = 10.0 ** rng.uniform(1.5, 3.5, n_stars)
    colour = rng.uniform(0.4, 1.6, (3, n_stars))
    planes = np.empty((3, H, W), F32)
    for c in range(3):
        img = 100.0 + 20.0 * c + rng.normal(0.0, 3.0, (H, W))
        for k in range(n_stars):
            img += colour[c, k] * amp[k] * np.exp(-((xx - xs[k]) ** 2 + (yy - ys[k]) ** 2) / (2 * 1.5 ** 2))
        planes[c] = img
    return planes
