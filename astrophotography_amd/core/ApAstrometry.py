"""ApAstrometry - an astrometric solution (a FITS WCS) for an image from its star list: the reference's step between ap_find_stars and
the SWarp resample (core/ApAstrometry.py).

The reference sends the star positions to the astrometry.net web service.  Here the field is solved offline against a catalogue file
the user provides, from the same hints the reference derives (an approximate centre, plate scale and field of view in the source
list's primary header): ops.solve_field, DESIGN 4.3m (PARITY UNPINNED: the rule is this project's own, the truth of its tests a planted
WCS).  The constructor's arguments, statuses and file behaviour are the reference's: a copy of the image with the WCS cards, and the
source list's photometry table (AP_L1MAG) with ra / dec columns.

  device  the catalogue's projection about the hint and its search cells (csrc/astrometry.hip), the triangle votes and the neighbour
          searches (csrc/register.hip)
  host    the hints, the TAN (and SIP order 2) least-squares fits, the files

Out of scope: blind solving without a centre, index files, proper motion and epoch, SIP above order 2, TPV, multi-GPU.
"""
import math
import os

import numpy as np

from .. import fitsio
from . import _common

BAD_KEYS = ('SIMPLE', 'BITPIX', 'NAXIS', 'EXTEND', 'HISTORY', 'DATE', 'COMMENT')       # never copied from a WCS into the output
PHOT_EXTNAME = 'AP_L1MAG'


def generate_hints(srclist_hdr, user_scale=None, scale_err_ratio=None):
    """The reference's _generate_hints on the source list's primary header: the centre from RA-OBJ / DEC-OBJ, else APRX_RA / APRX_DEC;
    the field of view from APRX_FOV, or with user_scale from the image size (IMG_COLS, IMG_ROWS, 4096 where absent); the pixel size
    sqrt((APRX_XPS^2 + APRX_YPS^2) / 2), or user_scale; radius = ceil(fov 1.5 ratio) with fov 4 degrees when unknown.
    -> dict(ra, dec, scale: None where unknown; ratio; radius: None without a centre; scale_lower, scale_upper)."""
    ratio = 1.3 if scale_err_ratio is None else float(scale_err_ratio)
    has = lambda k: k in srclist_hdr
    ra = float(srclist_hdr['RA-OBJ']) if has('RA-OBJ') else (float(srclist_hdr['APRX_RA']) if has('APRX_RA') else None)
    dec = float(srclist_hdr['DEC-OBJ']) if has('DEC-OBJ') else (float(srclist_hdr['APRX_DEC']) if has('APRX_DEC') else None)
    fov = xps = yps = None
    if user_scale is None:
        fov = float(srclist_hdr['APRX_FOV']) if has('APRX_FOV') else None
        xps = float(srclist_hdr['APRX_XPS']) if has('APRX_XPS') else None
        yps = float(srclist_hdr['APRX_YPS']) if has('APRX_YPS') else None
    else:
        cols = int(srclist_hdr['IMG_COLS']) if has('IMG_COLS') else 4096
        rows = int(srclist_hdr['IMG_ROWS']) if has('IMG_ROWS') else 4096
        xsiz, ysiz = cols * user_scale / 3600.0, rows * user_scale / 3600.0
        fov = math.sqrt(xsiz * xsiz + ysiz * ysiz)
        xps = yps = float(user_scale)
    out = dict(ra=ra, dec=dec, scale=None, ratio=ratio, radius=None, scale_lower=None, scale_upper=None)
    if ra is not None and dec is not None:
        out['radius'] = math.ceil((4.0 if fov is None else fov) * 1.5 * ratio)
    if xps is not None and yps is not None:
        mean = math.sqrt((xps * xps + yps * yps) / 2)
        out.update(scale=mean, scale_lower=mean / ratio, scale_upper=mean * ratio)
    return out


def _catalogue_column(cols, name, path):
    for k, v in cols.items():
        if k.strip().lower() == name.strip().lower():
            return np.asarray(v, np.float64)
    raise KeyError(f'{path}: the catalogue has no column {name!r} (columns: {sorted(cols)})')


def _hdus(raw):
    """(Header, first byte, one-past-last byte) of every HDU in the bytes that follow a primary HDU."""
    pos = 0
    while pos < len(raw):
        start, text = pos, ''
        while True:
            block = raw[pos:pos + fitsio.BLOCK].decode('ascii', 'replace')
            if len(block) < fitsio.BLOCK:
                raise OSError('extension header is truncated.')
            pos += fitsio.BLOCK
            text += block
            if any(block[i:i + 8] == 'END     ' for i in range(0, fitsio.BLOCK, 80)):
                break
        eh = fitsio.Header.fromstring(text)
        naxis = int(eh.get('NAXIS', 0))
        count = int(np.prod([int(eh['NAXIS%d' % i]) for i in range(1, naxis + 1)])) if naxis > 0 else 0
        nbytes = count * abs(int(eh['BITPIX'])) // 8 + int(eh.get('PCOUNT', 0))
        pos += ((nbytes + fitsio.BLOCK - 1) // fitsio.BLOCK) * fitsio.BLOCK
        yield eh, start, pos


class ApAstrometry:
    """Solves the image's astrometry from its source list against a catalogue and writes a copy of the image with valid WCS keywords.
    With a solution the photometry table of the source list also gets the sources' ra and dec.

    The arguments up to loglevel are the reference's, in its order (astnet_key is accepted and ignored: nothing is sent anywhere).
    catalog: a FITS file with a binary table (extension catalog_ext, default the first one named CATALOG) of columns ra_col, dec_col
    (degrees) and mag_col, names case-insensitive.  centre = (ra, dec) and radius (degrees) override the list's hints."""

    NOMINAL = 0       #: a WCS solution was obtained
    INPUT_ERROR = 1   #: non-nominal input, missing file, etc
    NO_SOLUTION = 2   #: no solution was found

    def __init__(self, inp_img_fname, inp_img_extnum, srclist_fname, srclist_extname, out_img_fname, astnet_key, use_sip, user_scale=None,
                 scale_err_ratio=None, loglevel='INFO', catalog=None, catalog_ext='CATALOG', ra_col='ra', dec_col='dec', mag_col='mag',
                 centre=None, radius=None, K=40, match_radius=3.0, min_matched=10):
        self._logger = _common.make_logger('ApAstrometry', loglevel)
        self._loglevel = loglevel
        self._status = ApAstrometry.NOMINAL
        self._use_sip = bool(use_sip)
        self._user_scale = user_scale
        self._scale_err_ratio = 1.3 if scale_err_ratio is None else float(scale_err_ratio)
        self._solution = None
        self._inp_fname, self._inp_extnum, self._src_fname, self._out_fname = inp_img_fname, inp_img_extnum, srclist_fname, out_img_fname
        if inp_img_fname == out_img_fname:
            self._logger.error('Output image cannot be the same as the input image. Choose a different name or path.')
            self._status = ApAstrometry.INPUT_ERROR
            return
        try:
            self._read_inputs(srclist_extname or 'AP_XYPOS', catalog, catalog_ext, ra_col, dec_col, mag_col)
            hints = generate_hints(self._src_meta, self._user_scale, scale_err_ratio)
            if centre is not None:
                hints['ra'], hints['dec'] = float(centre[0]), float(centre[1])
                if hints['radius'] is None:
                    hints['radius'] = math.ceil(4.0 * 1.5 * hints['ratio'])
            if radius is not None:
                hints['radius'] = float(radius)
            if hints['ra'] is None or hints['dec'] is None:
                raise ValueError('Could not estimate center_ra, center_dec: the source list has no RA-OBJ / APRX_RA cards; give centre=.')
            if hints['scale'] is None:
                raise ValueError('Could not generate scale hints: the source list has no APRX_XPS / APRX_YPS cards; give user_scale=.')
        except (OSError, KeyError, ValueError, TypeError) as exc:
            self._logger.error(str(exc))
            self._status = ApAstrometry.INPUT_ERROR
            return
        self._hints = hints
        self._logger.debug(f'Hints: {hints}')
        self._sanity_check(self._inp_fname, self._src_meta)
        from .. import ops
        sol = ops.solve_field(self._xy, (self._rows, self._cols), self._catalogue, (hints['ra'], hints['dec']), hints['scale'],
                              hints['ratio'], hints['radius'], K=K, match_radius=match_radius, min_matched=min_matched, use_sip=self._use_sip)
        self._solution = sol
        if sol['status'] != ops.SOLVE_NOMINAL:
            self._logger.warning(f'No output as no WCS found. Output image {out_img_fname} NOT created.')
            self._status = ApAstrometry.NO_SOLUTION
            return
        self._wcs = sol['wcs']
        self._logger.info('Obtained a WCS: %d stars matched, rms %.3f pix, %.4f arcsec/pix' % (sol['n_matched'], sol['rms'], sol['scale']))
        self._write_fits_image(self._wcs_cards(catalog))
        self._update_sourcelist(self._src_fname)

    # -- inputs ----------------------------------------------------------------------------------------------------------------
    def _read_inputs(self, srclist_extname, catalog, catalog_ext, ra_col, dec_col, mag_col):
        if self._inp_extnum not in (0, None):
            raise ValueError('Only the primary HDU (image extension 0) can be read.')
        for path in (self._inp_fname, self._src_fname):
            if not os.path.isfile(os.path.expanduser(str(path))):
                raise OSError(f'Cannot find {path}. Not a valid path or file.')
        if catalog is None or not os.path.isfile(os.path.expanduser(str(catalog))):
            raise OSError(f'Cannot find the catalogue {catalog}. Not a valid path or file.')
        self._ihdr = fitsio.getheader(str(self._inp_fname))
        if int(self._ihdr.get('NAXIS', 0)) != 2:
            raise ValueError('Error, only 2-D images are handled.')
        self._cols, self._rows = int(self._ihdr['NAXIS1']), int(self._ihdr['NAXIS2'])
        cols, _, self._src_meta = fitsio.read_table(str(self._src_fname), srclist_extname)
        x, y = _catalogue_column(cols, 'X', self._src_fname), _catalogue_column(cols, 'Y', self._src_fname)
        self._xy = np.stack([x - 1.0, y - 1.0], axis=1)                      # FITS 1-based -> 0-based, in file order (brightest first)
        self._logger.info(f'Read {len(x)} source positions from {self._src_fname}')
        ccols, _, _ = fitsio.read_table(str(catalog), catalog_ext)
        self._catalogue = {k: _catalogue_column(ccols, n, catalog) for k, n in (('ra', ra_col), ('dec', dec_col), ('mag', mag_col))}
        self._logger.info(f'Read {len(self._catalogue["ra"])} catalogue stars from {catalog}')

    def _sanity_check(self, image_filename, srclist_metadata):
        """Warns when the source list was not produced from the input image."""
        key = 'IMG_FILE'
        if key in srclist_metadata:
            if str(image_filename) in str(srclist_metadata[key]):
                self._logger.debug('The source list was generated from this input image. Proceding.')
                return
            msg = f'Source list NOT generated from the input image, but instead from {srclist_metadata[key]}'
        else:
            msg = f'Source list file lacks {key} keyword. Cannot assess if it was produced from {image_filename}'
        self._logger.warning(msg)
        self._logger.warning('Proceding, but WCS may be incorrect.')

    # -- outputs ---------------------------------------------------------------------------------------------------------------
    def _wcs_cards(self, catalog):
        sol, w = self._solution, self._wcs
        cards = {k: (v, 'astrometric solution') for k, v in w.header_cards().items()}
        rot = math.degrees(math.atan2(w.cd[0, 1], w.cd[1, 1]))      # the sky direction of the y axis is (CD1_2, CD2_2), whatever the parity
        cards.update(ASTNMAT=(int(sol['n_matched']), 'stars matched with the catalogue'), ASTRMS=(float(sol['rms']), '[pix] rms of the matched stars'),
                     ASTSCALE=(float(sol['scale']), '[arcsec/pix] fitted plate scale'), ASTROT=(float(rot), '[deg] position angle of the y axis, east of north'),
                     ASTPARIT=(int(sol['parity']), '+1: as on the sky (east left of north), -1: mirrored'),
                     ASTCAT=(os.path.basename(str(catalog))[:60], 'catalogue file'))
        return cards

    def _write_fits_image(self, cards):
        """A copy of the input file with the WCS solution in its header."""
        data, hdr = fitsio.read(str(self._inp_fname))
        for key, val in cards.items():
            if key not in BAD_KEYS and not key.startswith('NAXIS'):
                hdr[key] = val
        fitsio.write(str(self._out_fname), data, hdr, overwrite=True)
        self._logger.info(f'Wrote updated file with WCS to {self._out_fname}')

    def _update_sourcelist(self, srclist):
        """The photometry table (AP_L1MAG) gets ra and dec of its xcenter / ycenter (0-based) under the solution; the primary header and
        every other extension are kept byte for byte."""
        self._logger.info(f'Updating photometry in {srclist} with WCS soluton.')
        _, prim = fitsio.read(str(srclist), want_data=False)
        raw, parts, found = prim._tail, [], False
        for eh, lo, hi in _hdus(raw):
            if found or str(eh.get('EXTNAME', '')).strip().upper() != PHOT_EXTNAME or str(eh.get('XTENSION', '')).strip() != 'BINTABLE':
                parts.append(raw[lo:hi])
                continue
            found = True
            cols, _, _ = fitsio.read_table(str(srclist), PHOT_EXTNAME)
            cols = {k: v for k, v in cols.items() if k not in ('ra', 'dec')}
            ra, dec = self._wcs.pix2sky(cols['xcenter'], cols['ycenter'])
            cols['ra'], cols['dec'] = np.asarray(ra, np.float64), np.asarray(dec, np.float64)
            units = {str(eh['TTYPE%d' % i]).strip(): str(eh['TUNIT%d' % i]).strip() for i in range(1, int(eh['TFIELDS']) + 1) if 'TUNIT%d' % i in eh}
            units.update(ra='deg', dec='deg')
            extra = [(c.key, c.value) for c in eh.cards if c.key == 'COMMENT']
            parts.append(fitsio._bintable_hdu(PHOT_EXTNAME, cols, units, extra))
        if not found:
            raise RuntimeError(f'{srclist} does not contain the expected {PHOT_EXTNAME} extension.')
        with open(str(srclist), 'rb') as fh:
            whole = fh.read()
        tmp = str(srclist) + '.tmp%d' % os.getpid()
        with open(tmp, 'wb') as fh:
            fh.write(whole[:len(whole) - len(raw)])
            fh.write(b''.join(parts))
        os.replace(tmp, str(srclist))

    # -- public ----------------------------------------------------------------------------------------------------------------
    def status(self):
        return self._status

    def solution(self):
        """ops.solve_field's result (None when the inputs were refused)."""
        return self._solution
