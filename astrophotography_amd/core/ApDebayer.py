"""ApDebayer - colour planes from the Bayer mosaic of a one-shot-colour camera: the arithmetic of core/RawConv.py on the GPU (white
balance from the image :291-366, rgb() :401-486, grey() :488-587, split() :111-128).

The reference leaves the interpolation to LibRaw (rawpy.postprocess), which is not in its tree; this stage defines its own
(restated in tests/demosaic_model.py and tests/demosaic_rcd_model.py): bilinear, Malvar-He-Cutler 2004, one pixel per
2 x 2 cell, or the edge-directed RCD (modelled on RCD 2.x), every sample black-subtracted and scaled by its colour's white-balance
gain once, in one kernel launch (csrc/demosaic.hip).

  device  the per-colour sums of the white balance, the demosaic, FITS decode and encode
  host    the four gains from the eight numbers, headers

Out of scope: decoding camera RAW files and their EXIF data, the camera's own and the daylight white balance (LibRaw metadata),
--renormalize (ApComposite's levels cover the stretch), other adaptive demosaics such as AHD, RCD's refinement passes.
"""
import ast
import os

import numpy as np

from .. import fitsio
from . import _common

ARRANGEMENTS = {'RGGB': (0, 1, 3, 2), 'BGGR': (2, 1, 3, 0), 'GRBG': (1, 0, 2, 3), 'GBRG': (1, 2, 0, 3)}
WB_METHODS = ['daylight', 'camera', 'auto', 'region', 'user']          # RawConv.py:375
METHODS = ('bilinear', 'mhc', 'superpixel', 'rcd')
LUMINANCE_METHODS = ('linear', 'direct')
WB_KEYWORDS = ('WBRED', 'WBGREEN1', 'WBBLUE', 'WBGREEN2')


def pattern_of(name, xoff=0, yoff=0):
    """The pattern of a BAYERPAT name (the colours of the first two pixels of the first two rows), shifted by the offsets of
    XBAYROFF / YBAYROFF: the array's pixel (r, c) has the colour of the named cell's pixel (r + yoff, c + xoff)."""
    key = str(name).strip().upper()
    if key not in ARRANGEMENTS:
        raise ValueError(f'Bayer pattern {name!r} is not one of {sorted(ARRANGEMENTS)}.')
    base = ARRANGEMENTS[key]
    return tuple(base[(((p >> 1) + int(yoff)) & 1) * 2 + (((p & 1) + int(xoff)) & 1)] for p in range(4))


def parse_whitebalance(wb_method):
    """('auto' | 'region' | 'user', numbers or None) from the reference's white-balance strings, or from four numbers.  Raises
    before anything touches the device: RuntimeError with the reference's text for an unknown method (RawConv.py:379-382),
    NotImplementedError for 'camera' and 'daylight'."""
    if not isinstance(wb_method, str):
        vals = [float(v) for v in wb_method]
        if len(vals) != 4:
            raise ValueError(f'A user white balance takes four numbers (R, G1, B, G2), got {wb_method!r}.')
        return 'user', vals
    method = wb_method.split('[')[0]
    if method not in WB_METHODS:
        raise RuntimeError(f'Unexpected white balance method "{method}" not one of the allowed method: {WB_METHODS}')
    if method in ('camera', 'daylight'):
        raise NotImplementedError(f'White balance "{method}" needs the camera_whitebalance / daylight_whitebalance metadata that '
                                  'LibRaw reads from a RAW file; a FITS mosaic does not carry it. Use auto, region[...] or user[...].')
    if method == 'auto':
        return 'auto', None
    try:
        vals = list(ast.literal_eval(wb_method[len(method):]))
        vals = [float(v) for v in vals] if method == 'user' else [int(v) for v in vals]
    except (ValueError, SyntaxError, TypeError):
        vals = []
    if len(vals) != 4:
        raise ValueError(f'White balance {wb_method!r}: expected {method}[a, b, c, d] with four numbers.')
    return method, vals


class ApDebayer:
    """Bayer mosaics (device tensors or FITS files) -> red, green, blue planes or a luminance."""

    def __init__(self, loglevel='INFO'):
        self._loglevel = loglevel
        self._logger = _common.make_logger('ApDebayer', loglevel)
        self.gains = None               # the four gains (R, G1, B, G2) of the last rgb() / grey() call

    def whitebalance(self, mosaic, pattern, wb_method='auto', black=None):
        """Four float64 gains (R, G1, B, G2).  wb_method: 'auto' (the whole image), 'region[rowmin, rowmax, colmin, colmax]'
        (inclusive, zero based), 'user[r, g1, b, g2]' or four numbers.  auto and region: the mean of each colour's black-subtracted
        samples, gain = largest mean / mean (RawConv.py:291-331)."""
        from .. import ops
        pattern = ops.bayer_pattern(pattern)
        kind, vals = parse_whitebalance(wb_method)
        if kind == 'user':
            gains = np.asarray(vals, np.float64)
            if not np.all(np.isfinite(gains)):
                raise ValueError(f'A user white balance must be finite, got {vals}.')
            return gains
        frame = mosaic if mosaic.dim() == 2 else mosaic[0]
        return ops.bayer_whitebalance(frame, pattern, black, None if kind == 'auto' else vals)

    def _prepare(self, mosaic, pattern, method, wb_method, subtract_black, black):
        from .. import ops
        pattern = ops.bayer_pattern(pattern)
        if method not in METHODS:
            raise ValueError(f'Unexpected demosaic method {method!r}. Allowed methods are: {list(METHODS)}')
        parse_whitebalance(wb_method)
        black = black if subtract_black else None
        self.gains = self.whitebalance(mosaic, pattern, wb_method, black)
        self._logger.debug(f'White balance values adopted: {self.gains.tolist()}')
        return pattern, black

    def rgb(self, mosaic, pattern, method='mhc', wb_method='auto', subtract_black=True, black=None, as_uint16=False):
        """[3, h, w] (or [N, 3, h, w]) float32 planes of mosaic [H, W] / [N, H, W]; as_uint16: clipped to 0 .. 65535 and truncated
        (RawConv.rgb's np.clip + astype).  method: 'bilinear', 'mhc', 'superpixel' (h = H / 2) or 'rcd' (edge-directed: no zippers
        along edges, no coloured rims on stars; nothing is clamped, so a colour may undershoot below 0 beside a bright edge).  A slab
        takes the white balance of its first frame.  subtract_black False: the black levels stay in the data (--keepblack)."""
        from .. import ops
        pattern, black = self._prepare(mosaic, pattern, method, wb_method, subtract_black, black)
        return ops.bayer_demosaic(mosaic, pattern, black, self.gains, method, 'rgb_u16' if as_uint16 else 'rgb')

    def grey(self, mosaic, pattern, method='mhc', wb_method='auto', subtract_black=True, black=None, luminance_method='linear'):
        """The luminance [h, w] float32: 'linear' the CCIR 601 weights on the demosaiced colours (RawConv.py:549-556), 'direct' every
        sample times its white-balance gain, no interpolation (:533-547; method is ignored).  method: as in rgb()."""
        from .. import ops
        if luminance_method not in LUMINANCE_METHODS:
            raise ValueError(f'Unexpected luminance calculate method supplied to ApDebayer.grey: {luminance_method}. '
                             f'Allowed methods are: {list(LUMINANCE_METHODS)}')
        pattern, black = self._prepare(mosaic, pattern, method, wb_method, subtract_black, black)
        return ops.bayer_demosaic(mosaic, pattern, black, self.gains, method, 'grey' if luminance_method == 'linear' else 'direct')

    def split(self, mosaic, pattern, subtract_black=True, black=None):
        """RawConv.split: four full-size uint16 planes [4, H, W] (R, G1, B, G2), zero off their own sites."""
        from .. import ops
        return ops.bayer_split(mosaic, pattern, black if subtract_black else None)

    # -- files ------------------------------------------------------------------------------------------
    def _pattern_from(self, hdr, pattern):
        if pattern is not None:
            return pattern_of(pattern) if isinstance(pattern, str) else tuple(pattern)
        name = hdr.get('BAYERPAT')
        if name is None:
            raise RuntimeError('No Bayer pattern: the file has no BAYERPAT keyword and none was given (RGGB, BGGR, GRBG or GBRG).')
        return pattern_of(name, hdr.get('XBAYROFF', 0) or 0, hdr.get('YBAYROFF', 0) or 0)

    def debayer_files(self, infile, out_root, method='mhc', wb_method='auto', subtract_black=True, black=None, pattern=None,
                      grey=None, luminance_method='linear', overwrite=True):
        """Reads one FITS mosaic and writes out_root_r.fits, out_root_g.fits and out_root_b.fits (float32), or, with grey = a file
        name, the luminance alone.  pattern: RGGB, BGGR, GRBG or GBRG (or four colour indices), else the BAYERPAT keyword shifted
        by XBAYROFF / YBAYROFF; it applies to the array rows in file order.  The input header is passed through with HISTORY lines
        and DEBAYER (BILINEAR, MHC, SUPERPIXEL, RCD or DIRECT), WBRED, WBGREEN1, WBBLUE, WBGREEN2.  Returns the list of files
        written."""
        import torch
        _common.check_file_exists(self._logger, infile)
        data, hdr = fitsio.read_device(str(infile))
        if data is None or data.dim() != 2:
            raise RuntimeError(f'{infile}: expected a 2-D primary image.')
        if data.dtype not in (torch.uint16, torch.float32):
            data = data.to(torch.float32)
        pat = self._pattern_from(hdr, pattern)
        black = [0, 0, 0, 0] if black is None else list(black)
        if grey is not None:
            planes = [self.grey(data, pat, method, wb_method, subtract_black, black, luminance_method)]
            names = [str(grey)]
            what = f'{luminance_method} luminance'
        else:
            planes = list(self.rgb(data, pat, method, wb_method, subtract_black, black))
            names = [f'{out_root}_{c}.fits' for c in 'rgb']
            what = 'red, green, blue'
        out_hdr = hdr.copy()
        for key in ('BAYERPAT', 'XBAYROFF', 'YBAYROFF'):
            if key in out_hdr:
                del out_hdr[key]
        out_hdr['DEBAYER'] = (method.upper() if not (grey is not None and luminance_method == 'direct') else 'DIRECT', 'demosaic method')
        for key, g, name in zip(WB_KEYWORDS, self.gains, ('red', 'green 1', 'blue', 'green 2')):
            out_hdr[key] = (float(g), f'white balance gain of {name}')
        order = ''.join('RGBG'[k] for k in pat)
        out_hdr['HISTORY'] = f'ApDebayer: {os.path.basename(str(infile))} debayered ({order} in array order, {what})'
        out_hdr['HISTORY'] = ('ApDebayer: black levels ' + (' '.join('%g' % b for b in black) if subtract_black else 'kept')
                              + f', white balance {wb_method if isinstance(wb_method, str) else list(wb_method)}')
        _common.write_images(self._logger, list(zip(names, planes)), out_hdr, overwrite)
        return names
