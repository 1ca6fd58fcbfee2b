"""Minimal FITS celestial WCS (gnomonic / TAN projection) for the registration step.

The reference registers its frames with astrometry.net and hands the navigated files to SWarp with
``PROJECTION_TYPE TAN`` (scripts/resample_all.sh:123-131, 330-342): every file carries CTYPE = RA---TAN /
DEC--TAN, CRPIX, CRVAL and a CD (or CDELT + PC / CROTA2) matrix.  This module turns such headers into
pixel <-> sky maps (FITS WCS paper II, zenithal gnomonic projection; pinned against astropy.wcs by golden
vectors G10) and into the per-tile affine transforms the resample kernel consumes.  Host-side float64 numpy.
SIP distortion polynomials (RA---TAN-SIP / DEC--TAN-SIP, Shupe et al. 2005; pinned by golden vectors G20) are read by SipWcs -
`from_header` picks the class -; TanWcs itself refuses a distorted header, and TPV (PVi_j) terms are refused by both.
"""
import numpy as np

D2R = np.pi / 180.0


class TanWcs:
    """0-based pixel (x = column, y = row) <-> (ra, dec) in degrees for a RA---TAN / DEC--TAN header."""

    def __init__(self, crpix, crval, cd):
        self.crpix = np.asarray(crpix, np.float64)          # FITS 1-based reference pixel (CRPIX1, CRPIX2)
        self.crval = np.asarray(crval, np.float64)          # (ra0, dec0) degrees
        self.cd = np.asarray(cd, np.float64).reshape(2, 2)  # degrees per pixel
        self.cdinv = np.linalg.inv(self.cd)

    @classmethod
    def from_header(cls, hdr):
        get = hdr.get if hasattr(hdr, 'get') else (lambda k, d=None: hdr[k] if k in hdr else d)
        c1, c2 = str(get('CTYPE1', '')).strip(), str(get('CTYPE2', '')).strip()
        if not (c1.startswith('RA--') and c1.endswith('TAN') and c2.startswith('DEC-') and c2.endswith('TAN')):
            raise ValueError(f'Error, only RA---TAN / DEC--TAN headers are supported (found {c1!r}, {c2!r}).')
        if get('A_ORDER') is not None or get('B_ORDER') is not None or get('PV1_1') is not None:
            raise ValueError('Error, distortion terms (SIP / PV) are not supported.')
        crpix = (float(get('CRPIX1')), float(get('CRPIX2')))
        crval = (float(get('CRVAL1')), float(get('CRVAL2')))
        if get('CD1_1') is not None:
            cd = [[float(get('CD1_1')), float(get('CD1_2', 0.0))], [float(get('CD2_1', 0.0)), float(get('CD2_2'))]]
        else:
            cdelt = (float(get('CDELT1')), float(get('CDELT2')))
            if get('PC1_1') is not None:
                pc = [[float(get('PC1_1')), float(get('PC1_2', 0.0))], [float(get('PC2_1', 0.0)), float(get('PC2_2', 1.0))]]
            else:
                rot = float(get('CROTA2', 0.0)) * D2R       # the AIPS convention
                pc = [[np.cos(rot), -np.sin(rot) * cdelt[1] / cdelt[0]], [np.sin(rot) * cdelt[0] / cdelt[1], np.cos(rot)]]
            cd = [[cdelt[0] * pc[0][0], cdelt[0] * pc[0][1]], [cdelt[1] * pc[1][0], cdelt[1] * pc[1][1]]]
        return cls(crpix, crval, cd)

    @classmethod
    def from_center(cls, ra, dec, pixscale_arcsec, shape):
        """North up, east left, `pixscale_arcsec` per pixel, (ra, dec) at the centre of a [ny, nx] image: the grid
        SWarp builds from -CENTER / -PIXEL_SCALE / -IMAGE_SIZE (resample_all.sh:334-338)."""
        ny, nx = shape
        s = pixscale_arcsec / 3600.0
        return cls(((nx + 1) / 2.0, (ny + 1) / 2.0), (ra, dec), [[-s, 0.0], [0.0, s]])

    def tan(self):
        """The pure TAN part (an output grid is never distorted)."""
        return self

    def oversampled(self, n):
        """The same projection on a grid n times finer whose n x n blocks are this grid's pixels (FITS pixel centres are
        integers: CRPIX' = (CRPIX - 0.5) * n + 0.5)."""
        n = int(n)
        return type(self)(((self.crpix[0] - 0.5) * n + 0.5, (self.crpix[1] - 0.5) * n + 0.5), (self.crval[0], self.crval[1]),
                          [[self.cd[0, 0] / n, self.cd[0, 1] / n], [self.cd[1, 0] / n, self.cd[1, 1] / n]])

    def header_cards(self):
        return {'CTYPE1': 'RA---TAN', 'CTYPE2': 'DEC--TAN', 'CRPIX1': float(self.crpix[0]), 'CRPIX2': float(self.crpix[1]),
                'CRVAL1': float(self.crval[0]), 'CRVAL2': float(self.crval[1]), 'CD1_1': float(self.cd[0, 0]),
                'CD1_2': float(self.cd[0, 1]), 'CD2_1': float(self.cd[1, 0]), 'CD2_2': float(self.cd[1, 1])}

    def pix2sky(self, x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        u, v = x + 1.0 - self.crpix[0], y + 1.0 - self.crpix[1]
        xi = (self.cd[0, 0] * u + self.cd[0, 1] * v) * D2R   # standard coordinates (radians), xi towards east
        eta = (self.cd[1, 0] * u + self.cd[1, 1] * v) * D2R
        a0, d0 = self.crval[0] * D2R, self.crval[1] * D2R
        den = np.cos(d0) - eta * np.sin(d0)
        ra = a0 + np.arctan2(xi, den)
        dec = np.arctan2((eta * np.cos(d0) + np.sin(d0)) * np.cos(ra - a0), den)
        return np.mod(ra / D2R, 360.0), dec / D2R

    def sky2pix(self, ra, dec):
        a, d = np.asarray(ra, np.float64) * D2R, np.asarray(dec, np.float64) * D2R
        a0, d0 = self.crval[0] * D2R, self.crval[1] * D2R
        cosc = np.sin(d0) * np.sin(d) + np.cos(d0) * np.cos(d) * np.cos(a - a0)
        with np.errstate(divide='ignore', invalid='ignore'):
            xi = np.where(cosc > 0, np.cos(d) * np.sin(a - a0) / cosc, np.nan) / D2R       # behind the tangent plane -> NaN
            eta = np.where(cosc > 0, (np.cos(d0) * np.sin(d) - np.sin(d0) * np.cos(d) * np.cos(a - a0)) / cosc, np.nan) / D2R
        u = self.cdinv[0, 0] * xi + self.cdinv[0, 1] * eta
        v = self.cdinv[1, 0] * xi + self.cdinv[1, 1] * eta
        return u + self.crpix[0] - 1.0, v + self.crpix[1] - 1.0


SIP_MAX_ORDER = 5
SIP_CARDS = ('A_ORDER', 'B_ORDER', 'AP_ORDER', 'BP_ORDER', 'A_DMAX', 'B_DMAX')


def is_sip_card(key):
    """A header keyword of the SIP convention: the orders, A_p_q, B_p_q, AP_p_q, BP_p_q."""
    import re
    return key in SIP_CARDS or re.fullmatch(r'(A|B|AP|BP)_\d_\d', key) is not None


class SipWcs:
    """0-based pixel <-> (ra, dec) for a RA---TAN-SIP / DEC--TAN-SIP header: with (u, v) the pixel's offset from CRPIX, the TAN
    projection is applied to (u + A(u, v), v + B(u, v)), A = sum A_p_q u^p v^q over 2 <= p + q <= A_ORDER <= 5, B likewise.  The way
    back solves that by Newton (the rule of distortion.PolyMap.inverse); the header's AP / BP polynomials are only its starting
    point when present."""

    def __init__(self, crpix, crval, cd, a, b, ap=None, bp=None):
        self._tan = TanWcs(crpix, crval, cd)
        self.crpix, self.crval, self.cd = self._tan.crpix, self._tan.crval, self._tan.cd
        self.a, self.b = self._terms(a), self._terms(b)
        self.ap, self.bp = (None if ap is None else self._terms(ap)), (None if bp is None else self._terms(bp))

    @staticmethod
    def _terms(t):
        t = {(int(p), int(q)): float(c) for (p, q), c in dict(t).items() if float(c) != 0.0}
        if any(p < 0 or q < 0 or p + q > SIP_MAX_ORDER for p, q in t):
            raise ValueError('Error, SIP terms up to order %d are supported.' % SIP_MAX_ORDER)
        return t

    @classmethod
    def from_header(cls, hdr):
        get = hdr.get if hasattr(hdr, 'get') else (lambda k, d=None: hdr[k] if k in hdr else d)
        c1, c2 = str(get('CTYPE1', '')).strip(), str(get('CTYPE2', '')).strip()
        if not (c1.startswith('RA--') and c2.startswith('DEC-') and c1.endswith('TAN-SIP') and c2.endswith('TAN-SIP')):
            raise ValueError(f'Error, only RA---TAN-SIP / DEC--TAN-SIP headers are supported (found {c1!r}, {c2!r}).')
        if get('A_ORDER') is None or get('B_ORDER') is None:
            raise ValueError('Error, a -SIP header needs A_ORDER and B_ORDER.')
        plain = {k: get(k) for k in ('CRPIX1', 'CRPIX2', 'CRVAL1', 'CRVAL2', 'CD1_1', 'CD1_2', 'CD2_1', 'CD2_2', 'CDELT1', 'CDELT2',
                                      'PC1_1', 'PC1_2', 'PC2_1', 'PC2_2', 'CROTA2', 'PV1_1') if get(k) is not None}
        tan = TanWcs.from_header(dict(plain, CTYPE1='RA---TAN', CTYPE2='DEC--TAN'))

        def terms(prefix, lowest):
            order = get(prefix + '_ORDER')
            if order is None:
                return None
            order = int(order)
            if not 0 <= order <= SIP_MAX_ORDER:
                raise ValueError(f'Error, {prefix}_ORDER = {order}: SIP orders up to {SIP_MAX_ORDER} are supported.')
            return {(p, q): float(get('%s_%d_%d' % (prefix, p, q), 0.0)) for p in range(order + 1) for q in range(order + 1 - p)
                    if p + q >= lowest}
        return cls(tan.crpix, tan.crval, tan.cd, terms('A', 2), terms('B', 2), terms('AP', 0), terms('BP', 0))

    def tan(self):
        return self._tan

    def header_cards(self):
        """The cards `from_header` reads back: the TAN cards with CTYPE = ...-SIP, the orders and every non-zero coefficient."""
        cards = dict(self._tan.header_cards(), CTYPE1='RA---TAN-SIP', CTYPE2='DEC--TAN-SIP')
        for prefix, t, lowest in (('A', self.a, 2), ('B', self.b, 2), ('AP', self.ap, 0), ('BP', self.bp, 0)):
            if t is None:
                continue
            cards[prefix + '_ORDER'] = max([p + q for p, q in t] + [lowest])
            for (p, q), c in sorted(t.items()):
                cards['%s_%d_%d' % (prefix, p, q)] = float(c)
        return cards

    @staticmethod
    def _poly(t, u, v, du=0, dv=0):
        s = np.zeros(np.broadcast(u, v).shape)
        for (p, q), c in sorted(t.items()):
            if p < du or q < dv:
                continue
            s = s + (c * (p if du else 1) * (q if dv else 1)) * u ** (p - du) * v ** (q - dv)
        return s

    def pix2sky(self, x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        u, v = x + 1.0 - self.crpix[0], y + 1.0 - self.crpix[1]
        return self._tan.pix2sky(x + self._poly(self.a, u, v), y + self._poly(self.b, u, v))

    def sky2pix(self, ra, dec, tol=1e-12, max_steps=20):
        X, Y = self._tan.sky2pix(ra, dec)
        U, V = np.asarray(X + 1.0 - self.crpix[0]), np.asarray(Y + 1.0 - self.crpix[1])
        u, v = U.copy(), V.copy()
        if self.ap is not None and self.bp is not None:
            u, v = U + self._poly(self.ap, U, V), V + self._poly(self.bp, U, V)
        done = ~(np.isfinite(U) & np.isfinite(V))                           # behind the tangent plane: stays NaN
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            for _ in range(max_steps):
                rx, ry = u + self._poly(self.a, u, v) - U, v + self._poly(self.b, u, v) - V
                xx, xy = 1.0 + self._poly(self.a, u, v, 1, 0), self._poly(self.a, u, v, 0, 1)
                yx, yy = self._poly(self.b, u, v, 1, 0), 1.0 + self._poly(self.b, u, v, 0, 1)
                d = xx * yy - xy * yx
                du, dv = (yy * rx - xy * ry) / d, (xx * ry - yx * rx) / d
                u, v = np.where(done, u, u - du), np.where(done, v, v - dv)
                lim = np.maximum(tol, 8.0 * np.spacing(np.maximum(np.abs(u), np.abs(v))))
                done = done | (np.hypot(du, dv) < lim)
                if done.all():
                    break
        ok = done & np.isfinite(U) & np.isfinite(V)
        return np.where(ok, u, np.nan) + self.crpix[0] - 1.0, np.where(ok, v, np.nan) + self.crpix[1] - 1.0


def from_header(hdr):
    """TanWcs or SipWcs, whichever the header's CTYPE asks for."""
    get = hdr.get if hasattr(hdr, 'get') else (lambda k, d=None: hdr[k] if k in hdr else d)
    if str(get('CTYPE1', '')).strip().endswith('-SIP') or str(get('CTYPE2', '')).strip().endswith('-SIP'):
        return SipWcs.from_header(hdr)
    return TanWcs.from_header(hdr)


TILE_H, TILE_W = 16, 64          # the resample kernel's output tile (csrc/resample.hip)


def tile_affines(out_wcs, in_wcs, out_shape, tile_scale=1):
    """Per-tile affine approximation of the map output pixel -> input pixel (through the sky; either may be a TanWcs or a SipWcs):
    the exact map at
    the tile centre plus its central-difference Jacobian over the tile.  Over a 64 x 16 pixel tile of an
    arcsecond-scale image the second-order terms of TAN -> TAN are < 1e-3 pixel (the kernel's phase table
    resolves 1/1024 pixel).  Returns float64 [tiles_y, tiles_x, 6]: xin = A0*x + A1*y + A2, yin = A3*x + A4*y + A5
    with ABSOLUTE output pixel coordinates x, y.  tile_scale = n: `out_wcs` / `out_shape` describe the n-times finer grid of
    an OVERSAMPLING n resample and a tile is the 64 n x 16 n fine pixels of one output tile (apgpu_resample_oversampled_f32)."""
    ny, nx = out_shape
    TILE_H, TILE_W = 16 * int(tile_scale), 64 * int(tile_scale)
    ty, tx = (ny + TILE_H - 1) // TILE_H, (nx + TILE_W - 1) // TILE_W
    yc = np.arange(ty, dtype=np.float64)[:, None] * TILE_H + (TILE_H - 1) / 2.0 + np.zeros((1, tx))
    xc = np.arange(tx, dtype=np.float64)[None, :] * TILE_W + (TILE_W - 1) / 2.0 + np.zeros((ty, 1))

    def fwd(x, y):
        ra, dec = out_wcs.pix2sky(x, y)
        return in_wcs.sky2pix(ra, dec)

    hx, hy = TILE_W / 2.0, TILE_H / 2.0
    x0, y0 = fwd(xc, yc)
    xpx, ypx = fwd(xc + hx, yc)
    xmx, ymx = fwd(xc - hx, yc)
    xpy, ypy = fwd(xc, yc + hy)
    xmy, ymy = fwd(xc, yc - hy)
    a0, a3 = (xpx - xmx) / (2 * hx), (ypx - ymx) / (2 * hx)
    a1, a4 = (xpy - xmy) / (2 * hy), (ypy - ymy) / (2 * hy)
    a2 = x0 - a0 * xc - a1 * yc
    a5 = y0 - a3 * xc - a4 * yc
    return np.ascontiguousarray(np.stack([a0, a1, a2, a3, a4, a5], axis=-1))
