"""ApDeconvolve - damped Richardson-Lucy deconvolution of a finished co-add with its own PSF.

The reference has no such stage, so it is defined by this project (restated in tests/deconvolve_model.py).  It sits
between ap_coadd and ap_composite: the input is a float32 image, NaN meaning "no data"; the output has the same footprint.

  device  the norm plane, the forward convolution with the (damped) ratio and the back-projection with the update, two launches per
          iteration (csrc/deconvolve.hip); the star search and the Gaussian fits behind a measured FWHM; the clipped sky level;
          FITS decode and encode
  host    the PSF stamp (a pixel-integrated Gaussian or Moffat of the measured FWHM, or a stamp from a file), headers

Out of scope (the empirical PSF of the stars is ApEmpiricalPsf; its file is a stamp file for `psf`): spatially varying PSFs, deringing or star protection, TV or wavelet
regularisation, PSFs of radius above 12 (bin the image).
"""
import math
import os

import numpy as np

from .. import fitsio
from . import _common

PSF_KINDS = ('gaussian', 'moffat')
CARDS = ('DCONPSF', 'DCONFWHM', 'DCONRAD', 'DCONITER', 'DCONDAMP', 'DCONSKY', 'DCONSTRT')


class ApDeconvolve:
    """Richardson-Lucy deconvolution of an image (a device tensor or a FITS file) with a Gaussian, Moffat or given PSF."""

    def __init__(self, loglevel='INFO', psf='gaussian', beta=2.5, radius=None, niter=30, damp=0.0, readnoise=0.0, gain_keyword='EGAIN',
                 min_weight=0.1, search_fwhm=3.0, search_nsigma=7.0):
        """psf: 'gaussian', 'moffat' or the name of a FITS file with an odd, square stamp (normalised here).  beta: the Moffat
        exponent.  radius: of the stamp (None: ceil(1.7 FWHM) for the Gaussian, ceil(2.5 FWHM) for the Moffat).  damp: White's
        threshold in sigma, 0 for plain Richardson-Lucy.  readnoise: ADU.  search_fwhm, search_nsigma: the star search behind a
        measured FWHM."""
        self._loglevel = loglevel
        self._logger = _common.make_logger('ApDeconvolve', loglevel)
        self.psf_file = None
        if psf not in PSF_KINDS:
            if not isinstance(psf, (str, os.PathLike)) or not str(psf).lower().endswith(('.fits', '.fit', '.fts')):
                raise ValueError(f'Unexpected psf {psf!r}. Allowed values are: {list(PSF_KINDS)} or a FITS file name')
            self.psf_file = str(psf)
            psf = 'file'
        self.psf_kind = psf
        self.beta = float(beta)
        self.radius = None if radius is None else int(radius)
        self.niter, self.damp, self.readnoise = int(niter), float(damp), float(readnoise)
        if self.niter < 0 or not self.damp >= 0.0 or not self.readnoise >= 0.0:
            raise ValueError(f'niter ({niter}), damp ({damp}) and readnoise ({readnoise}) must be >= 0')
        self.gain_keyword = gain_keyword
        self.min_weight = float(min_weight)
        self.search_fwhm, self.search_nsigma = float(search_fwhm), float(search_nsigma)

    # -- pieces -----------------------------------------------------------------------------------------
    @staticmethod
    def normalise_stamp(stamp):
        """A PSF stamp from a file or the caller: odd and square, finite, >= 0; normalised to sum 1 in float64, cast to float32."""
        p = np.asarray(stamp, np.float64)
        if p.ndim != 2 or p.shape[0] != p.shape[1] or p.shape[0] % 2 != 1:
            raise ValueError('the PSF stamp must be square with an odd side, got shape %s' % (p.shape,))
        if not np.all(np.isfinite(p)) or np.any(p < 0) or not p.sum() > 0:
            raise ValueError('the PSF weights must be finite and >= 0 with a sum > 0')
        return (p / p.sum()).astype(np.float32)

    def measure_fwhm(self, image):
        """The median FWHM (pixels) of Gaussian fits to the image's stars, as ap_find_stars measures it."""
        from .ApFindStars import ApFindStars
        fs = ApFindStars.from_device(image, search_fwhm=self.search_fwhm, search_nsigma=self.search_nsigma, loglevel=self._loglevel)
        fwhm = fs.measure_fwhm(None)
        if not (np.isfinite(fwhm[0]) and fwhm[0] > 0):
            raise RuntimeError(f'Could not measure the FWHM of the image ({fwhm[2]} stars fitted): give fwhm or a PSF stamp.')
        self._logger.info(f'Measured FWHM: {fwhm[0]:.3f} +/- {fwhm[1]:.3f} pixels from {fwhm[2]} values')
        return float(fwhm[0])

    def make_psf(self, fwhm):
        """The float32 stamp of the constructor's PSF for this FWHM (a file's stamp needs none)."""
        from .. import ops
        if self.psf_kind == 'file':
            stamp, _ = fitsio.read(self.psf_file)
            return self.normalise_stamp(stamp)
        try:
            if self.psf_kind == 'moffat':
                return ops.psf_moffat(fwhm, self.beta, self.radius)
            return ops.psf_gaussian(fwhm, self.radius)
        except ValueError as exc:
            raise RuntimeError(f'No PSF stamp for FWHM = {fwhm} pixels: {exc}') from exc

    # -- tensors -----------------------------------------------------------------------------------------
    def deconvolve(self, image, fwhm=None, psf=None, sky=None, gain=1.0, niter=None, damp=None, readnoise=None, start=None):
        """image: a float32 device tensor [H, W].  psf: a stamp (array; normalised here) that overrides the constructor's choice.
        fwhm: pixels; measured from the image's stars when neither it nor a stamp is given.  sky: the level that is not
        deconvolved; None: the median of ops.sigclip_global.  gain: e-/ADU.  niter, damp, readnoise: None takes the constructor's.
        start: see ops.richardson_lucy.

        Returns dict(image, report)."""
        from .. import ops
        _common.need_image_f32(image)
        niter = self.niter if niter is None else int(niter)
        damp = self.damp if damp is None else float(damp)
        readnoise = self.readnoise if readnoise is None else float(readnoise)
        kind = self.psf_kind
        if psf is not None:
            stamp, kind = self.normalise_stamp(psf.cpu().numpy() if hasattr(psf, 'cpu') else psf), 'stamp'
        else:
            if fwhm is None and kind != 'file':
                fwhm = self.measure_fwhm(image)
            stamp = self.make_psf(fwhm)
        if sky is None:
            sky = float(ops.sigclip_global(image).cpu().numpy()[1])
            if not math.isfinite(sky):
                raise RuntimeError('Could not measure the sky level of the image: give sky.')
            sky = max(sky, 0.0)
            self._logger.info(f'Sky level (clipped median): {sky:.6g}')
        out, rep = ops.richardson_lucy(image, stamp, sky, niter=niter, damp=damp, gain=gain, readnoise=readnoise, start=start,
                                       min_weight=self.min_weight)
        rep.update(psf=kind, fwhm=None if fwhm is None else float(fwhm), beta=self.beta if kind == 'moffat' else None)
        self._logger.info('Richardson-Lucy: %s PSF of radius %d%s, %d iterations, damping %g, sky %.6g, start %s' % (
            kind, rep['radius'], '' if fwhm is None else f' (FWHM {float(fwhm):.3f})', niter, damp, rep['sky'],
            'plane' if rep['start'] is None else '%.6g' % rep['start']))
        return dict(image=out, report=rep, psf=stamp)

    # -- files ---------------------------------------------------------------------------------------------
    def deconvolve_files(self, input_file, output_file, fwhm=None, sky=None, overwrite=True):
        """FITS in, FITS out (float32).  The gain is the header's gain_keyword (1 when it is missing or not positive).  The output
        header is the input's plus the DCON* cards and HISTORY.  Returns the report."""
        image, hdr = _common.read_image_f32(self._logger, input_file)
        gain = 1.0
        if self.gain_keyword and self.gain_keyword in hdr:
            try:
                g = float(hdr[self.gain_keyword])
                gain = g if math.isfinite(g) and g > 0 else 1.0
            except (TypeError, ValueError):
                pass
        rep = self.deconvolve(image, fwhm=fwhm, sky=sky, gain=gain)
        out, rep = rep['image'], rep['report']
        out_hdr = hdr.copy()
        name = os.path.basename(self.psf_file) if rep['psf'] == 'file' else rep['psf'].upper()
        out_hdr['DCONPSF'] = (name, 'PSF of the deconvolution')
        out_hdr['DCONFWHM'] = (-999.0 if rep['fwhm'] is None else float(rep['fwhm']), '[pix] FWHM of the PSF')
        out_hdr['DCONRAD'] = (int(rep['radius']), '[pix] radius of the PSF stamp')
        out_hdr['DCONITER'] = (int(rep['niter']), 'Richardson-Lucy iterations')
        out_hdr['DCONDAMP'] = (float(rep['damp']), '[sigma] damping threshold (0: none)')
        out_hdr['DCONSKY'] = (float(rep['sky']), '[adu] sky level held out')
        out_hdr['DCONSTRT'] = (-999.0 if rep['start'] is None else float(rep['start']), '[adu] start level of the estimate')
        out_hdr['HISTORY'] = (f'ApDeconvolve: {rep["niter"]} Richardson-Lucy iterations, {name} PSF of radius {rep["radius"]}, '
                              f'damping {rep["damp"]:g}, gain {rep["gain"]:g}')
        _common.write_image(self._logger, output_file, out, out_hdr, overwrite)
        return rep
