"""Polynomial distortion maps (DESIGN 4.3e'): reference pixel -> input pixel beyond a 2x3 affine.  Host-side float64 numpy.

    x_in = Px(u, v),  y_in = Py(u, v),  u = (x - x0) / L,  v = (y - y0) / L        (IEEE division)

of total degree d in 1 .. 5.  The monomials run by total degree t = 0 .. d and within t by j = 0 .. t (the power of v), i = t - j
the power of u: ncoef = (d + 1)(d + 2) / 2 per axis.  The evaluation order is a contract shared with csrc/distortion_core.h (the
kernels) and tests/distortion_model.py (the model), every operation rounding on its own:

    up[0] = 1, up[i] = up[i-1] * u (vp likewise);  s = +0;  s = s + c[k] * (up[i] * vp[j])  in coefficient order.

A first derivative is formed the same way from (i * c[k]) * (up[i-1] * vp[j]) over the terms with i >= 1 (j likewise), then divided
by L.  The resample and drizzle kernels never see the polynomial: they take its linearisation per 16 x 64 output tile
(ops.poly_tile_affines), and `tile_error` bounds what that costs.
"""
import numpy as np

MAX_DEGREE = 5


def ncoef(degree):
    return (degree + 1) * (degree + 2) // 2


def exponents(degree):
    """[(i, j)] in coefficient order: i the power of u, j the power of v."""
    return [(t - j, j) for t in range(degree + 1) for j in range(t + 1)]


def _degree_of(n):
    for d in range(1, MAX_DEGREE + 1):
        if ncoef(d) == n:
            return d
    raise ValueError('%d coefficients per axis are no polynomial of total degree 1 .. %d (3, 6, 10, 15 or 21)' % (n, MAX_DEGREE))


def _powers(u, d):
    up = [np.ones_like(u)]
    for _ in range(d):
        up.append(up[-1] * u)
    return up


def _sum(c, up, vp, d, du=0, dv=0):
    """The (du, dv)-th derivative with respect to (u, v), in the contract's order (du + dv <= 2 here)."""
    s = np.zeros_like(up[0])
    for k, (i, j) in enumerate(exponents(d)):
        if i < du or j < dv:
            continue
        m = 1.0
        for q in range(du):
            m *= i - q
        for q in range(dv):
            m *= j - q
        s = s + (m * c[k] if du or dv else c[k]) * (up[i - du] * vp[j - dv])
    return s


class PolyMap:
    """One frame's map.  cx, cy: [ncoef] float64; origin (x0, y0) and scale L as above."""

    def __init__(self, cx, cy, origin=(0.0, 0.0), scale=1.0):
        self.cx, self.cy = np.array(cx, np.float64).reshape(-1), np.array(cy, np.float64).reshape(-1)
        if self.cx.size != self.cy.size:
            raise ValueError('the two axes hold %d and %d coefficients' % (self.cx.size, self.cy.size))
        self.degree = _degree_of(self.cx.size)
        if not (np.all(np.isfinite(self.cx)) and np.all(np.isfinite(self.cy))):
            raise ValueError('the coefficients must be finite')
        self.x0, self.y0, self.L = float(origin[0]), float(origin[1]), float(scale)
        if not (np.isfinite(self.x0) and np.isfinite(self.y0) and np.isfinite(self.L) and self.L > 0.0):
            raise ValueError('origin must be finite and scale finite and positive, got %r, %r' % (origin, scale))

    @property
    def origin(self):
        return (self.x0, self.y0)

    def _uv(self, x, y):
        x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
        return _powers((x - self.x0) / self.L, self.degree), _powers((y - self.y0) / self.L, self.degree)

    def eval(self, x, y):
        up, vp = self._uv(x, y)
        return _sum(self.cx, up, vp, self.degree), _sum(self.cy, up, vp, self.degree)

    def jacobian(self, x, y):
        """(dX/dx, dX/dy, dY/dx, dY/dy)."""
        up, vp = self._uv(x, y)
        d, L = self.degree, self.L
        return (_sum(self.cx, up, vp, d, 1, 0) / L, _sum(self.cx, up, vp, d, 0, 1) / L,
                _sum(self.cy, up, vp, d, 1, 0) / L, _sum(self.cy, up, vp, d, 0, 1) / L)

    def hessian(self, x, y):
        """(Xxx, Xxy, Xyy, Yxx, Yxy, Yyy) per pixel^2."""
        up, vp = self._uv(x, y)
        d, L2 = self.degree, self.L * self.L
        return tuple(_sum(c, up, vp, d, a, b) / L2 for c in (self.cx, self.cy) for a, b in ((2, 0), (1, 1), (0, 2)))

    @classmethod
    def from_affine(cls, A, degree=1, origin=(0.0, 0.0), scale=1.0):
        """The affine x_in = a0 x + a1 y + a2, y_in = a3 x + a4 y + a5 as a map of `degree` (the higher terms zero)."""
        if isinstance(degree, bool) or int(degree) != degree or not 1 <= int(degree) <= MAX_DEGREE:
            raise ValueError('degree must be 1 .. %d, got %r' % (MAX_DEGREE, degree))
        A = np.asarray(A, np.float64).reshape(6)
        x0, y0, L = float(origin[0]), float(origin[1]), float(scale)
        cx, cy = np.zeros(ncoef(int(degree))), np.zeros(ncoef(int(degree)))
        cx[:3] = (A[0] * x0 + A[1] * y0) + A[2], A[0] * L, A[1] * L
        cy[:3] = (A[3] * x0 + A[4] * y0) + A[5], A[3] * L, A[4] * L
        return cls(cx, cy, origin, scale)

    def affine_part(self):
        """The terms of degree <= 1 as a 2x3 affine in pixels."""
        L = self.L
        a0, a1, a3, a4 = self.cx[1] / L, self.cx[2] / L, self.cy[1] / L, self.cy[2] / L
        return np.array([a0, a1, self.cx[0] - (a0 * self.x0 + a1 * self.y0), a3, a4, self.cy[0] - (a3 * self.x0 + a4 * self.y0)])

    def compose_affine(self, B):
        """The map p -> B(self(p)) for a 2x3 affine B acting on the input frame's pixels (a crop, a binning, a flip of the frame):
        a linear combination of the coefficients, same degree, origin and scale."""
        B = np.asarray(B, np.float64).reshape(6)
        e0 = np.zeros_like(self.cx)
        e0[0] = 1.0
        return PolyMap(B[0] * self.cx + B[1] * self.cy + B[2] * e0, B[3] * self.cx + B[4] * self.cy + B[5] * e0, self.origin, self.L)

    def inverse(self, x_in, y_in, tol=1e-12, max_steps=20):
        """The reference pixel that maps to (x_in, y_in): Newton from the inverse of the affine part.  Stops at a step below tol
        pixels - or below 8 ulp of the coordinate where that is larger: beyond 2048 px a float64 coordinate moves in steps of
        4.5e-13 px and the residual's own rounding is a few of those - or after max_steps; NaN where it has not converged by then."""
        xi, yi = np.broadcast_arrays(np.asarray(x_in, np.float64), np.asarray(y_in, np.float64))
        A = self.affine_part()
        det = A[0] * A[4] - A[1] * A[3]
        x = (A[4] * (xi - A[2]) - A[1] * (yi - A[5])) / det
        y = (A[0] * (yi - A[5]) - A[3] * (xi - A[2])) / det
        done = np.zeros(x.shape, bool)
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            for _ in range(max_steps):
                X, Y = self.eval(x, y)
                xx, xy, yx, yy = self.jacobian(x, y)
                rx, ry = X - xi, Y - yi
                d = xx * yy - xy * yx
                dx, dy = (yy * rx - xy * ry) / d, (xx * ry - yx * rx) / d
                x, y = np.where(done, x, x - dx), np.where(done, y, y - dy)
                lim = np.maximum(tol, 8.0 * np.spacing(np.maximum(np.abs(x), np.abs(y))))
                done = done | (np.hypot(dx, dy) < lim)
                if done.all():
                    break
        return np.where(done, x, np.nan), np.where(done, y, np.nan)

    @staticmethod
    def design(r, degree, origin, scale):
        """[n, ncoef]: the monomials at the reference positions r [n, 2]."""
        r = np.asarray(r, np.float64)
        up, vp = _powers((r[:, 0] - float(origin[0])) / float(scale), degree), _powers((r[:, 1] - float(origin[1])) / float(scale), degree)
        return np.stack([up[i] * vp[j] for i, j in exponents(degree)], axis=1)

    @classmethod
    def fit(cls, r, s, degree, origin, scale):
        """Least squares s ~ map(r) (r, s [n, 2]), each axis on the design matrix in (u, v).  -> (map, rank, 2-D rms); the map is
        None when the design is rank-deficient or holds fewer rows than columns."""
        r, s = np.asarray(r, np.float64), np.asarray(s, np.float64)
        D = cls.design(r, degree, origin, scale)
        if D.shape[0] < D.shape[1]:
            return None, int(np.linalg.matrix_rank(D)) if D.size else 0, float('nan')
        cx, _, rank, _ = np.linalg.lstsq(D, s[:, 0], rcond=None)
        cy = np.linalg.lstsq(D, s[:, 1], rcond=None)[0]
        if rank < D.shape[1]:
            return None, int(rank), float('nan')
        m = cls(cx, cy, origin, scale)
        X, Y = m.eval(r[:, 0], r[:, 1])
        return m, int(rank), float(np.sqrt(np.mean((X - s[:, 0]) ** 2 + (Y - s[:, 1]) ** 2)))

    def tile_error(self, out_shape, tile_scale=1, scale=1.0):
        """An upper estimate (input pixels) of what the per-tile linearisation of ops.poly_tile_affines leaves over a tile of
        64 tile_scale x 16 tile_scale output pixels: 0.5 (|fxx| hx^2 + 2 |fxy| hx hy + |fyy| hy^2) with hx = 32 tile_scale, hy =
        8 tile_scale, the second derivatives (per output pixel: the grid holds `scale` pixels per reference pixel) taken at the
        tile centres, the larger of the two axes, over at most 64 x 64 evenly spaced tiles with the corner tiles among them."""
        ts, s = int(tile_scale), float(scale)
        th, tw = 16 * ts, 64 * ts
        ty, tx = -(-int(out_shape[0]) // th), -(-int(out_shape[1]) // tw)
        iy = np.unique(np.round(np.linspace(0, ty - 1, min(ty, 64)))).astype(np.float64)
        ix = np.unique(np.round(np.linspace(0, tx - 1, min(tx, 64)))).astype(np.float64)
        yc = ((iy * th + (th - 1) / 2.0) + 0.5) / s - 0.5
        xc = ((ix * tw + (tw - 1) / 2.0) + 0.5) / s - 0.5
        H = self.hessian(xc[None, :], yc[:, None])
        hx, hy = 32.0 * ts / s, 8.0 * ts / s
        e = [0.5 * (np.abs(H[o]) * hx * hx + 2.0 * np.abs(H[o + 1]) * hx * hy + np.abs(H[o + 2]) * hy * hy) for o in (0, 3)]
        return float(max(e[0].max(), e[1].max()))


def stack_coefficients(maps):
    """maps (a list of PolyMap sharing degree, origin and scale) -> (coef float64 [N, 2, ncoef], degree, x0, y0, L)."""
    maps = list(maps)
    if not maps:
        raise ValueError('no maps')
    m0 = maps[0]
    for m in maps[1:]:
        if (m.degree, m.x0, m.y0, m.L) != (m0.degree, m0.x0, m0.y0, m0.L):
            raise ValueError('the maps of one call share their degree, origin and scale')
    return np.stack([np.stack([m.cx, m.cy]) for m in maps]), m0.degree, m0.x0, m0.y0, m0.L


# -- the `distortion:` entry of a transforms file (ApRegister.write_transforms writes it, ap_coadd and ap_drizzle read it) --------
def to_document(maps, orders, names):
    """{origin, scale, frames: {name: {order, x: [...], y: [...]}}}: every frame at its own order (a frame that kept its affine holds
    three coefficients per axis); maps share origin and scale, None entries are left out."""
    kept = [(m, int(o), n) for m, o, n in zip(maps, orders, names) if m is not None]
    if not kept:
        return None
    m0 = kept[0][0]
    frames = {}
    for m, o, n in kept:
        if (m.x0, m.y0, m.L) != (m0.x0, m0.y0, m0.L):
            raise ValueError('the maps of one file share their origin and scale')
        k = ncoef(min(o, m.degree))
        frames[n] = {'order': min(o, m.degree), 'x': [float(v) for v in m.cx[:k]], 'y': [float(v) for v in m.cy[:k]]}
    return {'origin': [m0.x0, m0.y0], 'scale': m0.L, 'frames': frames}


def from_document(entry, names):
    """The maps of `names` (a frame is looked up by its name as given, then by its base name) from a file's `distortion:` entry,
    brought to one degree - the largest order among them, the others padded with zeros.  ValueError for a frame without an entry
    or an entry that is no map."""
    import os
    if not isinstance(entry, dict) or 'frames' not in entry or 'origin' not in entry or 'scale' not in entry:
        raise ValueError('the distortion entry must hold origin, scale and frames')
    origin, L, table = [float(v) for v in entry['origin']], float(entry['scale']), entry['frames'] or {}
    recs = []
    for n in names:
        key = n if n in table else os.path.basename(str(n))
        if key not in table:
            raise ValueError('no distortion map for %s' % n)
        r = table[key]
        order, x, y = int(r['order']), [float(v) for v in r['x']], [float(v) for v in r['y']]
        if not 1 <= order <= MAX_DEGREE or len(x) != ncoef(order) or len(y) != ncoef(order):
            raise ValueError('the map of %s: order %d needs %d coefficients per axis, found %d and %d'
                             % (key, order, ncoef(order) if 1 <= order <= MAX_DEGREE else 0, len(x), len(y)))
        recs.append((order, x, y))
    top = max(o for o, _, _ in recs)
    pad = lambda c: c + [0.0] * (ncoef(top) - len(c))
    return [PolyMap(pad(x), pad(y), origin, L) for _, x, y in recs]
