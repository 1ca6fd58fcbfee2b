"""ApMultiscale - noise reduction and detail enhancement by scale with the B3-spline a trous ("starlet") transform.

The reference has no such stage, so it is defined by this project (restated in tests/multiscale_model.py).  It sits
between ap_coadd / ap_deconvolve and ap_composite: the input is a float32 image, NaN meaning "no data"; the output has the same
footprint.

  device  the transform, the thresholds, the gains and the sum, one launch per scale (csrc/multiscale.hip); plane 1 and its clipped
          standard deviation behind a measured noise; FITS decode and encode
  host    the noise constants of the planes, the thresholds, headers

Header cards, one line per group:
  MSCALES           number of scales J
  MSMODE            HARD or SOFT
  MSSIGMA           [adu] image noise the thresholds are scaled by (given or measured)
  MSK1 .. MSKJ      threshold of plane j in units of its noise
  MSG1 .. MSGJ      gain of plane j
  MSGRES            gain of the smooth residual

Out of scope: star protection or deringing masks, per-pixel noise maps and Poisson (Anscombe) noise, other wavelets, iterated
(multiresolution support) reconstruction, colour beyond one image at a time.
"""
import math

import numpy as np

from . import _common

MODES = ('hard', 'soft')
MAX_SCALES = 6
DEFAULT_K = (3.0, 3.0, 2.0, 1.0, 1.0, 1.0)
CARDS = ('MSCALES', 'MSMODE', 'MSSIGMA', 'MSK1', 'MSG1', 'MSGRES')


def _per_scale(v, J, name):
    try:
        v = np.asarray(v, np.float64).reshape(-1)
    except (TypeError, ValueError) as exc:
        raise ValueError(f'{name} must be a number or {J} numbers, got {v!r}') from exc
    if v.size == 1:
        v = np.repeat(v, J)
    if v.size != J:
        raise ValueError(f'{name} needs one value or {J} (one per scale), got {v.size}')
    return v


class ApMultiscale:
    """Starlet denoise and sharpen of an image (a device tensor or a FITS file)."""

    CARDS = CARDS

    def __init__(self, loglevel='INFO', scales=4, k=None, gains=1.0, residual_gain=1.0, mode='hard', sigma=None):
        """scales: J, 1 .. 6.  k: the threshold of each plane in units of its noise (one value per scale or one for all; 0 leaves a
        plane alone; None: DEFAULT_K cut to the number of scales).  gains: the weight of each plane in the sum (above 1 sharpens that
        scale, 0 drops it).  residual_gain: the weight of the smooth residual.  mode: 'hard' or 'soft'.  sigma: the image noise in ADU; None: measured from plane 1."""
        self._loglevel = loglevel
        self._logger = _common.make_logger('ApMultiscale', loglevel)
        if isinstance(scales, bool) or int(scales) != scales or not 1 <= int(scales) <= MAX_SCALES:
            raise ValueError(f'scales must be 1 .. {MAX_SCALES}, got {scales!r}')
        self.scales = int(scales)
        if mode not in MODES:
            raise ValueError(f'Unexpected mode {mode!r}. Allowed values are: {list(MODES)}')
        self.mode = mode
        self.k = _per_scale(DEFAULT_K[:self.scales] if k is None else k, self.scales, 'k')
        if not np.all(np.isfinite(self.k)) or not np.all(self.k >= 0.0):
            raise ValueError(f'the thresholds k must be finite and >= 0, got {self.k.tolist()}')
        self.gains = _per_scale(gains, self.scales, 'gains')
        self.residual_gain = float(residual_gain)
        if not np.all(np.isfinite(self.gains.astype(np.float32))) or not math.isfinite(float(np.float32(self.residual_gain))):
            raise ValueError(f'the gains must be finite, got {self.gains.tolist()} and {residual_gain!r}')
        self.sigma = None if sigma is None else float(sigma)
        if self.sigma is not None and not (self.sigma >= 0.0 and math.isfinite(self.sigma)):
            raise ValueError(f'sigma must be finite and >= 0, got {sigma!r}')

    # -- tensors -----------------------------------------------------------------------------------------
    def process(self, image, sigma=None):
        """image: a float32 device tensor [H, W].  sigma: the image noise; None takes the constructor's, and when that is None too
        it is measured (RuntimeError when the image has no measurable noise: pass sigma).

        Returns dict(image, report); report has sigma, t, J, mode, k, gains, g_res, measured."""
        from .. import ops
        _common.need_image_f32(image)
        sigma = self.sigma if sigma is None else float(sigma)
        out, rep = ops.multiscale(image, self.scales, self.k, self.gains, self.residual_gain, self.mode, sigma=sigma)
        rep['measured'] = sigma is None
        self._logger.info('Starlet %s thresholding, %d scales, noise %.6g ADU (%s): thresholds %s, gains %s, residual gain %g' % (
            self.mode, self.scales, rep['sigma'], 'measured' if sigma is None else 'given', ' '.join('%.4g' % t for t in rep['t']),
            ' '.join('%g' % g for g in rep['gains']), rep['g_res']))
        return dict(image=out, report=rep)

    # -- files ---------------------------------------------------------------------------------------------
    def process_file(self, input_file, output_file, sigma=None, overwrite=True):
        """FITS in, FITS out (float32).  The output header is the input's plus the MS* cards and HISTORY.  Returns the report."""
        image, hdr = _common.read_image_f32(self._logger, input_file)
        rep = self.process(image, sigma=sigma)
        out, rep = rep['image'], rep['report']
        out_hdr = hdr.copy()
        out_hdr['MSCALES'] = (int(rep['J']), 'starlet scales')
        out_hdr['MSMODE'] = (rep['mode'].upper(), 'thresholding of the starlet planes')
        out_hdr['MSSIGMA'] = (float(rep['sigma']), '[adu] image noise (%s)' % ('measured' if rep['measured'] else 'given'))
        for j in range(rep['J']):
            out_hdr['MSK%d' % (j + 1)] = (float(rep['k'][j]), 'threshold of plane %d in units of its noise' % (j + 1))
        for j in range(rep['J']):
            out_hdr['MSG%d' % (j + 1)] = (float(rep['gains'][j]), 'gain of plane %d' % (j + 1))
        out_hdr['MSGRES'] = (float(rep['g_res']), 'gain of the smooth residual')
        out_hdr['HISTORY'] = (f'ApMultiscale: {rep["J"]} starlet scales, {rep["mode"]} thresholds at '
                              f'{",".join("%g" % v for v in rep["k"])} sigma, noise {rep["sigma"]:.6g}')
        _common.write_image(self._logger, output_file, out, out_hdr, overwrite)
        return rep
