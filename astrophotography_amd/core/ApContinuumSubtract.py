"""ApContinuumSubtract - the line emission of a narrow-band image: L = N' - s C' - b, the primes the two images brought to one PSF.

The reference's stage table lists "Image Combination - Continuum Subtract - Continuum scaling/subtraction" as not yet built
(doc/iTelescope_processing.md:8-29), so the stage is defined by this project (restated in tests/continuum_model.py).
It sits between ap_coadd and ap_composite: both inputs are float32 images on one pixel grid, NaN meaning "no data".

  device  the normalised Gaussian blur that matches the sharper image to the broader one, the six moments of every round of the
          clipped straight-line fit, aperture photometry of the stars, the fused subtraction (csrc/continuum.hip), FITS decode
          and encode
  host    the taps, the 2 x 2 solve per round, the medians over a few hundred stars, headers

Out of scope: correcting C for the line's own share of the broad band (filter-width algebra), non-Gaussian or spatially varying
PSF matching, per-pixel variance planes.
"""
import math
import os

import numpy as np

from .. import fitsio
from . import _common

METHODS = ('stars', 'pixels')
CARDS = ('CSUBSCAL', 'CSUBOFF', 'CSUBMETH', 'CSUBFILE', 'CSUBFWN', 'CSUBFWC', 'CSUBKSIG', 'CSUBNPIX', 'CSUBITER')


class ApContinuumSubtract:
    """Scaled, PSF-matched subtraction of a continuum image from a narrow-band image (device tensors or FITS files)."""

    def __init__(self, loglevel='INFO', method=None, psf_match=True, fwhm_threshold=0.05, min_weight=0.5, sigma_lower=3.0,
                 sigma_upper=2.0, maxiters=10, min_stars=5, satlevel=None, search_fwhm=3.0, search_nsigma=7.0, keep_matched=False):
        """method: 'stars', 'pixels' or None (stars when a star list is given, pixels otherwise).  satlevel: stars whose list peak
        reaches it are not used for the scale.  search_fwhm, search_nsigma: the star search behind a measured FWHM."""
        if method is not None and method not in METHODS:
            raise ValueError(f'Unexpected method {method!r}. Allowed methods are: {list(METHODS)}')
        self._loglevel = loglevel
        self._logger = _common.make_logger('ApContinuumSubtract', loglevel)
        self.method = method
        self.psf_match = bool(psf_match)
        self.fwhm_threshold = float(fwhm_threshold)
        self.min_weight = float(min_weight)
        self.sigma_lower, self.sigma_upper, self.maxiters = float(sigma_lower), float(sigma_upper), int(maxiters)
        self.min_stars = int(min_stars)
        self.satlevel = satlevel
        self.search_fwhm, self.search_nsigma = float(search_fwhm), float(search_nsigma)
        self.keep_matched = bool(keep_matched)

    # -- pieces -----------------------------------------------------------------------------------------
    def measure_fwhm(self, image, name='image'):
        """The median FWHM (pixels) of Gaussian fits to the image's stars, as ap_find_stars measures it; also returns the star
        positions [k, 2] (x, y) and their peaks."""
        from .ApFindStars import ApFindStars
        fs = ApFindStars.from_device(image, search_fwhm=self.search_fwhm, search_nsigma=self.search_nsigma, loglevel=self._loglevel,
                                     fitsimg=name)
        fwhm = fs.measure_fwhm(None)
        if not (np.isfinite(fwhm[0]) and fwhm[0] > 0):
            raise RuntimeError(f'Could not measure the FWHM of the {name} image ({fwhm[2]} stars fitted): give fwhm=(narrow, continuum).')
        self._logger.info(f'Measured FWHM of the {name} image: {fwhm[0]:.3f} +/- {fwhm[1]:.3f} pixels from {fwhm[2]} values')
        t = fs._phot_table
        return float(fwhm[0]), np.stack([t['xcenter'], t['ycenter']], 1), np.asarray(t['peak_adu'], np.float64)

    @staticmethod
    def _star_arrays(stars):
        """(xy [k, 2], peak [k] or None) from an array [k, 2] / [k, 3] (x, y[, peak]) or a dict with xcenter, ycenter[, peak_adu]."""
        if stars is None:
            return None, None
        if isinstance(stars, dict):
            xy = np.stack([np.asarray(stars['xcenter'], np.float64), np.asarray(stars['ycenter'], np.float64)], 1)
            peak = np.asarray(stars['peak_adu'], np.float64) if 'peak_adu' in stars else None
            return xy, peak
        a = np.asarray(stars.cpu() if hasattr(stars, 'cpu') else stars, np.float64)
        if a.ndim != 2 or a.shape[1] not in (2, 3):
            raise ValueError('stars must be [k, 2] (x, y) or [k, 3] (x, y, peak), got shape %s' % (a.shape,))
        return a[:, :2].copy(), (a[:, 2].copy() if a.shape[1] == 3 else None)

    # -- tensors -----------------------------------------------------------------------------------------
    def subtract(self, narrow, continuum, fwhm=None, stars=None, mask=None, scale=None, offset=None, keep_matched=None):
        """narrow, continuum: float32 device tensors [H, W] on one grid.  fwhm: (narrow, continuum) in pixels, measured from the
        images when None and PSF matching is on.  stars: positions (see _star_arrays; x = column) in the common grid.  mask: non-zero
        pixels take no part in the fit.  scale, offset: given values are used as they are; a given scale alone is held while the
        offset is fitted over the pixels.  keep_matched: also return the PSF-matched images (None: the constructor's setting).

        The method is the constructor's; None means 'stars' when the caller gives a star list and 'pixels' otherwise.  Stars that
        were found while the FWHM was measured only serve star_residual_frac: they never choose the method.  'stars' without a
        list searches C' with ops.find_stars.

        Returns dict(image, report[, narrow_matched, continuum_matched])."""
        if tuple(narrow.shape) != tuple(continuum.shape):
            raise RuntimeError(f'The narrow-band image is {tuple(narrow.shape)} and the continuum image {tuple(continuum.shape)}: '
                               'continuum subtraction needs both on one pixel grid (ap_coadd --center/--pixelscale/--image_size).')
        from .. import ops
        for name, t in (('narrow', narrow), ('continuum', continuum)):
            _common.need_image_f32(t, name)
        keep_matched = self.keep_matched if keep_matched is None else bool(keep_matched)
        xy, peak = self._star_arrays(stars)
        method = self.method or ('stars' if xy is not None else 'pixels')
        xy_res = xy                                                  # the stars behind star_residual_frac
        fw_n = fw_c = None
        if fwhm is not None:
            fw_n, fw_c = float(fwhm[0]), float(fwhm[1])
        elif self.psf_match:
            fw_n, _, _ = self.measure_fwhm(narrow, 'narrow')
            fw_c, xy_c, _ = self.measure_fwhm(continuum, 'continuum')
            if xy_res is None:
                xy_res = xy_c
        info = dict(blurred=None, sigma_k=0.0, taps=None)
        n_m, c_m = narrow.contiguous(), continuum.contiguous()
        if self.psf_match:
            try:
                n_m, c_m, info = ops.psf_match(n_m, c_m, fw_n, fw_c, self.fwhm_threshold, self.min_weight)
            except ValueError as exc:
                raise RuntimeError(f'PSF matching failed for FWHM narrow = {fw_n}, continuum = {fw_c} pixels: {exc}') from exc
            self._logger.info('PSF matching: %s (sigma_k = %.4f pixels, %d taps)' % (
                'nothing blurred' if info['blurred'] is None else f"the {info['blurred']} image blurred", info['sigma_k'],
                0 if info['taps'] is None else len(info['taps'])))
        fw_broad = max(fw_n, fw_c) if fw_n is not None else self.search_fwhm

        if method == 'stars' and xy is None and scale is None:
            st = ops.sigclip_global(c_m).cpu().numpy()                # mean, median, std of the background
            f = ops.find_stars(c_m, fw_broad, self.search_nsigma * float(st[2]), bg_median=float(st[1]))
            xy = np.stack([f['xcentroid'].cpu().numpy(), f['ycentroid'].cpu().numpy()], 1)
            peak = f['peak'].cpu().numpy()
            xy_res = xy
        fit = None
        if scale is not None and offset is not None:
            s, b, method = float(scale), float(offset), 'user'
        elif method == 'stars' and scale is None:
            fit = ops.continuum_scale_stars(n_m, c_m, xy, fw_broad, peak, self.satlevel, self.min_stars, mask, self.sigma_lower,
                                            self.sigma_upper, self.maxiters)
            s, b = fit['s'], fit['b']
        else:                                                         # a given scale is held: only the offset is fitted
            method = 'pixels'
            fit = ops.continuum_scale_pixels(n_m, c_m, mask, self.sigma_lower, self.sigma_upper, self.maxiters, fixed_scale=scale)
            s, b = fit['s'], fit['b']
        if scale is not None:
            s = float(scale)
        if offset is not None:
            b = float(offset)
        image = ops.linear_combine(n_m, c_m, 1.0, -s, -b)

        report = dict(scale=s, offset=b, method=method, fwhm_narrow=fw_n, fwhm_continuum=fw_c, sigma_k=info['sigma_k'],
                      blurred=info['blurred'], taps=0 if info['taps'] is None else len(info['taps']), iterations=0, n_pixels=0, n_stars=0,
                      sigma=float('nan'), sigma0=float('nan'), se_scale=float('nan'), se_offset=float('nan'), offset_uncorrected=b,
                      sigma_lower=self.sigma_lower, sigma_upper=self.sigma_upper, star_residual_frac=float('nan'))
        if fit is not None:
            report.update(iterations=fit['iterations'], n_pixels=fit['n'], sigma=fit['sigma'], sigma0=fit['sigma0'], se_scale=fit['se_s'],
                          se_offset=fit['se_b'], offset_uncorrected=fit['b_uncorrected'], n_stars=fit.get('n_stars_used', 0))
        if xy_res is not None and len(xy_res):
            fl = ops.aperture_photometry(image, xy_res[:, 0], xy_res[:, 1], fwhm=fw_broad)['aperture_sum'].cpu().numpy()
            fn = fit['flux_n'] if fit is not None and 'flux_n' in fit else \
                ops.aperture_photometry(n_m, xy_res[:, 0], xy_res[:, 1], fwhm=fw_broad)['aperture_sum'].cpu().numpy()
            ok = np.isfinite(fl) & np.isfinite(fn) & (fn > 0)
            if ok.any():
                report['star_residual_frac'] = float(np.median(np.abs(fl[ok]) / fn[ok]))
        self._logger.info('Continuum subtraction (%s): scale = %.6g, offset = %.6g, %d pixels, %d stars, %d clipping rounds, '
                          'star residual fraction = %.4g' % (method, s, b, report['n_pixels'], report['n_stars'], report['iterations'],
                                                             report['star_residual_frac']))
        out = dict(image=image, report=report)
        if keep_matched:
            out.update(narrow_matched=n_m, continuum_matched=c_m)
        return out

    # -- files ---------------------------------------------------------------------------------------------
    @staticmethod
    def read_star_list(path):
        """The stars of a source list written by ap_find_stars (extension AP_L1MAG): dict(xcenter, ycenter, peak_adu)."""
        cols, _, _ = fitsio.read_table(str(path), 'AP_L1MAG')
        return {k: np.asarray(cols[k], np.float64) for k in ('xcenter', 'ycenter', 'peak_adu') if k in cols}

    def subtract_files(self, narrow_file, continuum_file, output_file, fwhm=None, stars=None, mask_file=None, scale=None, offset=None,
                       matched_out=None, overwrite=True):
        """FITS in, FITS out (float32).  stars: a source list of ap_find_stars (a file name) or what subtract() takes.  mask_file: a
        FITS image, non-zero = take no part in the fit.  matched_out: a prefix; PREFIX_narrow.fits and PREFIX_continuum.fits get the
        PSF-matched images.  The output header is the narrow-band file's, plus the CSUB* cards and HISTORY.  Returns the report."""
        import torch
        narrow, hdr = _common.read_image_f32(self._logger, narrow_file)
        continuum, _ = _common.read_image_f32(self._logger, continuum_file)
        if tuple(narrow.shape) != tuple(continuum.shape):
            raise RuntimeError(f'{narrow_file} is {tuple(narrow.shape)} and {continuum_file} is {tuple(continuum.shape)}: continuum '
                               'subtraction needs both on one pixel grid (ap_coadd --center/--pixelscale/--image_size).')
        if isinstance(stars, (str, os.PathLike)):
            stars = self.read_star_list(stars)
        mask = None
        if mask_file is not None:
            m, _ = _common.read_image_f32(self._logger, mask_file)
            if tuple(m.shape) != tuple(narrow.shape):
                raise RuntimeError(f'{mask_file} is {tuple(m.shape)}, the images are {tuple(narrow.shape)}.')
            mask = (m != 0).to(torch.uint8)
        r = self.subtract(narrow, continuum, fwhm=fwhm, stars=stars, mask=mask, scale=scale, offset=offset,
                          keep_matched=self.keep_matched or matched_out is not None)
        rep = r['report']
        out_hdr = hdr.copy()

        def num(v):
            return float(v) if v is not None and math.isfinite(v) else -999.0
        out_hdr['CSUBSCAL'] = (float(rep['scale']), 'continuum scale s of L = N - s C - b')
        out_hdr['CSUBOFF'] = (float(rep['offset']), 'offset b of L = N - s C - b')
        out_hdr['CSUBMETH'] = (str(rep['method']).upper(), 'how s and b were set')
        out_hdr['CSUBFILE'] = (os.path.basename(str(continuum_file)), 'continuum image')
        out_hdr['CSUBFWN'] = (num(rep['fwhm_narrow']), '[pix] FWHM of the narrow-band image')
        out_hdr['CSUBFWC'] = (num(rep['fwhm_continuum']), '[pix] FWHM of the continuum image')
        out_hdr['CSUBKSIG'] = (float(rep['sigma_k']), '[pix] sigma of the PSF-matching Gaussian')
        out_hdr['CSUBNPIX'] = (int(rep['n_pixels']), 'pixel pairs kept by the fit')
        out_hdr['CSUBITER'] = (int(rep['iterations']), 'clipping rounds of the fit')
        out_hdr['HISTORY'] = f'ApContinuumSubtract: L = N - s C - b, s = {rep["scale"]:.6g}, b = {rep["offset"]:.6g}'
        out_hdr['HISTORY'] = ('ApContinuumSubtract: ' + ('no image blurred' if rep['blurred'] is None else f'{rep["blurred"]} image blurred')
                              + f', star residual {rep["star_residual_frac"]:.4g}')
        names = [(str(output_file), r['image'])]
        if matched_out is not None:
            names += [(f'{matched_out}_narrow.fits', r['narrow_matched']), (f'{matched_out}_continuum.fits', r['continuum_matched'])]
        _common.write_images(self._logger, names, out_hdr, overwrite)
        return rep
