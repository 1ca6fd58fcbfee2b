"""NumPy statement of F10: the scaled sample, the reflected borders, the three demosaic methods in their float32
evaluation order, the four outputs, and the per-colour sums with Python integers.  Written from the definition; the kernels of
csrc/demosaic.hip must equal it bit for bit.

pattern[4]: the colour (R 0, G1 1, B 2, G2 3) of cell position (r & 1) 2 + (c & 1)."""
import math

import numpy as np

F = np.float32
ARRANGEMENTS = {'RGGB': (0, 1, 3, 2), 'BGGR': (2, 1, 3, 0), 'GRBG': (1, 0, 2, 3), 'GBRG': (1, 2, 0, 3)}


def colour_map(shape, pattern):
    r, c = np.indices(shape)
    return np.asarray(pattern)[(r & 1) * 2 + (c & 1)]


def black_subtracted(mosaic, pattern, black=None):
    """max(raw - black[k], 0): integer for uint16 (int64 result), float32 for float32 (d < 0 -> 0, NaN stays)."""
    k = colour_map(mosaic.shape[-2:], pattern)
    b = np.zeros(4) if black is None else np.asarray(black, np.float64)
    if mosaic.dtype == np.uint16:
        d = mosaic.astype(np.int64) - b.astype(np.int64)[k]
        return np.where(d < 0, 0, d)
    assert mosaic.dtype == np.float32
    with np.errstate(invalid='ignore'):
        d = mosaic - b.astype(F)[k]
        return np.where(d < 0, F(0), d).astype(F)


def scaled(mosaic, pattern, black=None, gain=None):
    g = np.ones(4, F) if gain is None else np.asarray(gain, np.float64).astype(F)
    k = colour_map(mosaic.shape[-2:], pattern)
    with np.errstate(invalid='ignore', over='ignore'):
        return (black_subtracted(mosaic, pattern, black).astype(F) * g[k]).astype(F)


def fold(i, n):
    """Reflection about the edge sample without repeating it, period 2 (n - 1)."""
    m = np.mod(i, 2 * (n - 1))
    return np.where(m < n, m, 2 * (n - 1) - m)


def _tap(s, dr, dc):
    H, W = s.shape
    return s[np.ix_(fold(np.arange(H) + dr, H), fold(np.arange(W) + dc, W))]


def _rgb_full(s, pattern, method):
    H, W = s.shape
    assert H >= 2 and W >= 2
    k = colour_map((H, W), pattern)
    rr, cc = np.indices((H, W))
    row_colour = np.asarray(pattern)[(rr & 1) * 2 + ((cc & 1) ^ 1)]          # the colour of the horizontal neighbours
    with np.errstate(invalid='ignore', over='ignore'):
        C = s
        ns = _tap(s, -1, 0) + _tap(s, 1, 0)
        we = _tap(s, 0, -1) + _tap(s, 0, 1)
        d4 = (_tap(s, -1, -1) + _tap(s, -1, 1)) + (_tap(s, 1, -1) + _tap(s, 1, 1))
        if method == 'bilinear':
            g_at_rb = (ns + we) * F(0.25)
            other = d4 * F(0.25)
            hor = we * F(0.5)
            ver = ns * F(0.5)
        elif method == 'mhc':
            ns2 = _tap(s, -2, 0) + _tap(s, 2, 0)
            we2 = _tap(s, 0, -2) + _tap(s, 0, 2)
            a4 = ns2 + we2
            g_at_rb = ((F(8) * C + F(4) * (ns + we)) - F(2) * a4) * F(0.0625)
            other = ((F(12) * C + F(4) * d4) - F(3) * a4) * F(0.0625)
            c10 = F(10) * C
            hor = (((c10 + F(8) * we) + ns2) - F(2) * (d4 + we2)) * F(0.0625)
            ver = (((c10 + F(8) * ns) + we2) - F(2) * (d4 + ns2)) * F(0.0625)
        else:
            raise ValueError(method)
    green = (k & 1) == 1
    R = np.where(green, np.where(row_colour == 0, hor, ver), np.where(k == 0, C, other))
    G = np.where(green, C, g_at_rb)
    B = np.where(green, np.where(row_colour == 2, hor, ver), np.where(k == 2, C, other))
    out = np.stack([R, G, B]).astype(F)
    assert out.dtype == F
    return out


def _rgb_superpixel(s, pattern):
    H, W = s.shape
    assert H % 2 == 0 and W % 2 == 0
    pos = {k: p for p, k in enumerate(pattern)}
    cell = lambda k: s[pos[k] >> 1::2, pos[k] & 1::2]
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([cell(0), (cell(1) + cell(3)) * F(0.5), cell(2)]).astype(F)


def to_u16(v):
    """(uint16) min(max(v, 0), 65535), truncating; NaN -> 0."""
    with np.errstate(invalid='ignore'):
        c = np.where(v > 0, np.where(v < 65535, v, F(65535)), F(0))
    return c.astype(np.uint16)


def luma(rgb):
    with np.errstate(invalid='ignore', over='ignore'):
        return ((F(0.299) * rgb[0] + F(0.587) * rgb[1]) + F(0.114) * rgb[2]).astype(F)


def demosaic(mosaic, pattern=(0, 1, 3, 2), black=None, gain=None, method='mhc', output='rgb'):
    """One frame [H, W] -> [3, h, w] ('rgb' float32, 'rgb_u16') or [h, w] ('grey', 'direct')."""
    s = scaled(mosaic, pattern, black, gain)
    if output == 'direct':
        return s
    rgb = _rgb_superpixel(s, pattern) if method == 'superpixel' else _rgb_full(s, pattern, method)
    if output == 'rgb':
        return rgb
    if output == 'rgb_u16':
        return to_u16(rgb)
    if output == 'grey':
        return luma(rgb)
    raise ValueError(output)


def channel_sums(mosaic, pattern, black=None, region=None):
    """(sums, counts) of the four colours over rowmin, rowmax, colmin, colmax (inclusive, clamped).  uint16: Python integers.
    float32: math.fsum of the finite black-subtracted samples (the exactly rounded sum) and their number; also returns, as a
    third item, the sum of their magnitudes."""
    H, W = mosaic.shape
    r0, r1, c0, c1 = (0, H, 0, W) if region is None else [int(v) for v in region]
    r0, r1, c0, c1 = max(r0, 0), min(r1, H - 1), max(c0, 0), min(c1, W - 1)
    d = black_subtracted(mosaic, pattern, black)
    k = colour_map((H, W), pattern)
    inside = np.zeros((H, W), bool)
    if r1 >= r0 and c1 >= c0:
        inside[r0:r1 + 1, c0:c1 + 1] = True
    sums, counts, mags = [], [], []
    for colour in range(4):
        v = d[inside & (k == colour)]
        if mosaic.dtype == np.uint16:
            sums.append(sum(int(x) for x in v))
            counts.append(int(v.size))
            mags.append(sums[-1])
        else:
            v = v[np.isfinite(v)].astype(np.float64)
            sums.append(math.fsum(v.tolist()))
            counts.append(int(v.size))
            mags.append(math.fsum(np.abs(v).tolist()))
    return sums, counts, mags


def whitebalance(mosaic, pattern, black=None, region=None):
    """avg = sum / count, gain = max(avg) / avg (RawConv.py:315-331), float64."""
    sums, counts, _ = channel_sums(mosaic, pattern, black, region)
    avg = [float(s) / float(n) for s, n in zip(sums, counts)]
    return np.array([max(avg) / a for a in avg], np.float64)
