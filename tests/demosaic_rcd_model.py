"""NumPy statement of F10's RCD method (include/apgpu.h): ratio-corrected, edge-directed demosaic modelled on RCD 2.x
(L. Sanz Rodriguez), in its float32 evaluation order.  Written from the definition; the kernel rcd_kernel of csrc/demosaic.hip must
equal it bit for bit.

The scaled mosaic is extended to all integer positions by the folded reflection of F10 and every intermediate plane is computed on
that extended mosaic (it is not a reflection of the intermediate plane); the image is cut out at the end.  Every operation rounds
once, in the order written.  A shift below wraps around the padded array: the wrapped values travel inwards by less than PAD."""
import numpy as np

from tests.demosaic_model import colour_map, fold, luma, scaled, to_u16

F = np.float32
HALO = 10                           # APGPU_DEMOSAIC_RCD_HALO: an output pixel depends on samples at Chebyshev distance <= HALO
PAD = 12                            # even (a padded index keeps its colour) and >= HALO
EPS, EPSSQ = F(2.0 ** -10), F(2.0 ** -20)
HALF, QUARTER, ONE = F(0.5), F(0.25), F(1)
AXES = {'N': (-1, 0), 'S': (1, 0), 'W': (0, -1), 'E': (0, 1)}
DIAGONALS = {'NW': (-1, -1), 'SE': (1, 1), 'NE': (-1, 1), 'SW': (1, -1)}


def _at(a, dr, dc):
    """The plane whose (r, c) is a(r + dr, c + dc)."""
    return np.roll(a, (-dr, -dc), (0, 1))


def _d4(a):
    return (_at(a, -1, -1) + _at(a, -1, 1)) + (_at(a, 1, -1) + _at(a, 1, 1))


def _stat(s, dr, dc):
    """Step 1 along the direction (dr, dc): the high-pass h, its square q, three of them summed, floored at epssq."""
    t = lambda n: _at(s, n * dr, n * dc)
    h = (((t(-3) + t(3)) - (t(-1) + t(1))) - F(3) * (t(-2) + t(2))) + F(6) * s
    q = h * h
    stat = (_at(q, -dr, -dc) + _at(q, dr, dc)) + q
    return np.where(stat < EPSSQ, EPSSQ, stat)                  # a NaN stays


def _disc(centre):
    """The value itself, or the mean of its four diagonal neighbours where that is farther from 0.5."""
    near = QUARTER * _d4(centre)
    return np.where(np.abs(HALF - centre) < np.abs(HALF - near), near, centre)


def _pair(g1, e1, g2, e2):
    """The estimates e1, e2 of two opposite directions, each weighted by the other's gradient."""
    return (g2 * e1 + g1 * e2) / (g1 + g2)


def rgb_planes(s, pattern):
    """[3, H, W] float32 from the scaled mosaic s [H, W]."""
    H, W = s.shape
    assert H >= 2 and W >= 2 and s.dtype == F
    P = PAD
    s = s[np.ix_(fold(np.arange(-P, H + P), H), fold(np.arange(-P, W + P), W))]
    k = colour_map(s.shape, pattern)
    green = (k & 1) == 1
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        # 1: direction statistics
        V, Hs = _stat(s, 1, 0), _stat(s, 0, 1)
        VH = V / (V + Hs)
        vd = _disc(VH)
        # 2: low pass
        lpf = (s + HALF * ((_at(s, -1, 0) + _at(s, 1, 0)) + (_at(s, 0, -1) + _at(s, 0, 1)))) + QUARTER * _d4(s)
        # 3: green at R/B sites
        grad, est = {}, {}
        for name, (dr, dc) in AXES.items():
            t = lambda n: _at(s, n * dr, n * dc)
            grad[name] = (((EPS + np.abs(t(1) - t(-1))) + np.abs(s - t(2))) + np.abs(t(1) - t(3))) + np.abs(t(2) - t(4))
            lpf2 = _at(lpf, 2 * dr, 2 * dc)
            est[name] = t(1) * (ONE + (lpf - lpf2) / ((EPS + lpf) + lpf2))
        v_est = _pair(grad['N'], est['N'], grad['S'], est['S'])
        h_est = _pair(grad['W'], est['W'], grad['E'], est['E'])
        G = np.where(green, s, vd * h_est + (ONE - vd) * v_est)
        # 4: diagonal statistics.  D = (P - Q) / (P + Q) = 2 PQ - 1 changes its sign, bit for bit, when P and Q change places
        Pst, Qst = _stat(s, 1, 1), _stat(s, -1, 1)
        D = (Pst - Qst) / (Pst + Qst)
        # 5: the other of R/B at R/B sites
        near = QUARTER * _d4(D)
        dd = np.where(np.abs(D) < np.abs(near), near, D)
        grad, est = {}, {}
        for name, (dr, dc) in DIAGONALS.items():
            t = lambda n: _at(s, n * dr, n * dc)
            grad[name] = ((EPS + np.abs(t(1) - t(-1))) + np.abs(t(1) - t(3))) + np.abs(G - _at(G, 2 * dr, 2 * dc))
            est[name] = t(1) - _at(G, dr, dc)
        p_est = _pair(grad['NW'], est['NW'], grad['SE'], est['SE'])
        q_est = _pair(grad['NE'], est['NE'], grad['SW'], est['SW'])
        O = G + ((HALF * (ONE - dd)) * p_est + (HALF * (ONE + dd)) * q_est)
        # 6: R and B at green sites
        out = {}
        for colour in (0, 2):
            X = np.where(k == colour, s, O)
            grad, est = {}, {}
            for name, (dr, dc) in AXES.items():
                x = lambda n: _at(X, n * dr, n * dc)
                grad[name] = ((EPS + np.abs(G - _at(G, 2 * dr, 2 * dc))) + np.abs(x(1) - x(-1))) + np.abs(x(1) - x(3))
                est[name] = x(1) - _at(G, dr, dc)
            v_est = _pair(grad['N'], est['N'], grad['S'], est['S'])
            h_est = _pair(grad['W'], est['W'], grad['E'], est['E'])
            out[colour] = np.where(green, G + ((ONE - vd) * v_est + vd * h_est), X)
    rgb = np.stack([out[0], G, out[2]])[:, P:P + H, P:P + W].astype(F)
    assert rgb.dtype == F
    return np.ascontiguousarray(rgb)


def demosaic(mosaic, pattern=(0, 1, 3, 2), black=None, gain=None, output='rgb'):
    """One frame [H, W] -> [3, H, W] ('rgb' float32, 'rgb_u16') or [H, W] ('grey', 'direct')."""
    s = scaled(mosaic, pattern, black, gain)
    if output == 'direct':
        return s
    rgb = rgb_planes(s, pattern)
    if output == 'rgb':
        return rgb
    if output == 'rgb_u16':
        return to_u16(rgb)
    if output == 'grey':
        return luma(rgb)
    raise ValueError(output)
