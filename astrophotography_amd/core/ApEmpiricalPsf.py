"""ApEmpiricalPsf - the effective PSF of an image from its own stars, PSF-fitting photometry with it, and the image with the stars
removed.

The reference has no such stage (it would need photutils), so it is defined by this project (restated in
tests/epsf_model.py) after Anderson & King (2000).  The input is a float32 image (NaN meaning "no data") and the star list
ap_find_stars wrote; the ePSF's stamp is what ap_deconvolve --psf takes.

  device  the accumulation of the stars' residuals on the oversampled grid, the update (add, smooth), the shift, the fits of every
          star and the model / residual image (csrc/epsf.hip); FITS decode and encode
  host    the choice of the stars, the smoothing taps, the grid's centre of mass and sum (a copy of at most 257 x 257 values), the
          tiles' star lists, headers and tables

Out of scope: a spatially varying ePSF, simultaneous fits of groups of stars, saturated stars' wings, several GPUs.
"""
import math

import numpy as np

from .. import fitsio
from . import _common

PHOT_COLUMNS = ('flux_fit', 'x_fit', 'y_fit', 'sky_fit', 'chi2', 'fit_ok')
NOMINAL, BAD_INPUT, TOO_FEW_STARS = 0, 1, 2
MIN_STARS = 3


class TooFewStars(RuntimeError):
    """Fewer than three stars of the list can be used to build the ePSF."""


class ApEmpiricalPsf:
    """The empirical PSF of an image (a device tensor or a FITS file) and what follows from it."""

    def __init__(self, loglevel='INFO', oversampling=4, radius=12, fit_radius=None, max_stars=500, niter=8, tol=1e-4, smoothing='quartic',
                 sigma=2.5, maxiters=5, min_count=1, fit_sky=False, gain_keyword=None, readnoise=0.0, max_iter=50):
        """oversampling: grid nodes per pixel (1 .. 4).  radius: of the stamp, pixels (2 .. 32).  fit_radius: of the fits, pixels
        (None: max(2, the list's FWHM)).  max_stars, niter, tol, smoothing, sigma, maxiters, min_count: see ops.epsf_build.
        fit_sky: the fits free the sky as well.  gain_keyword: header card of the gain (e-/ADU) of the *_files forms; with a gain
        the fits weigh by 1 / (readnoise^2 + max(model, 0) / gain), readnoise in ADU.  Give a read noise (or the sky's noise) with a
        gain: with readnoise = 0 a pixel whose model is <= 0 has an infinite weight and its star gets fit_ok = False."""
        from .. import ops
        self._logger = _common.make_logger('ApEmpiricalPsf', loglevel)
        ops.epsf_grid_size(oversampling, radius)
        ops.epsf_smoothing_taps(smoothing)
        self.oversampling, self.radius = int(oversampling), int(radius)
        self.fit_radius = None if fit_radius is None else float(fit_radius)
        if self.fit_radius is not None and not 1.0 <= self.fit_radius <= 32.0:
            raise ValueError(f'fit_radius ({fit_radius}) must lie in 1 .. 32')
        self.max_stars, self.niter, self.tol, self.smoothing = int(max_stars), int(niter), float(tol), smoothing
        self.sigma, self.maxiters, self.min_count = float(sigma), int(maxiters), int(min_count)
        self.fit_sky, self.gain_keyword, self.readnoise, self.max_iter = bool(fit_sky), gain_keyword, float(readnoise), int(max_iter)
        if self.max_stars < 1 or self.niter < 1 or not self.readnoise >= 0.0:
            raise ValueError(f'max_stars ({max_stars}) and niter ({niter}) must be >= 1 and readnoise ({readnoise}) >= 0')
        self.epsf = None                                       # the grid of the last build() or load_psf(): a float32 device tensor

    # -- pieces -----------------------------------------------------------------------------------------
    @staticmethod
    def star_columns(stars):
        """(x, y, flux, sky, psbl_sat) float64 / bool arrays of a star list: a dict or table with the columns xcenter, ycenter,
        aperture_sum, bgmed_per_pix (optional: 0) and psbl_sat (optional: False) of ap_find_stars' AP_L1MAG."""
        try:
            x, y, f = (np.asarray(stars[k], np.float64).reshape(-1) for k in ('xcenter', 'ycenter', 'aperture_sum'))
        except (KeyError, TypeError, IndexError) as exc:
            raise ValueError(f'the star list needs the columns xcenter, ycenter and aperture_sum ({exc!r})') from exc
        keys = stars.keys() if hasattr(stars, 'keys') else ()
        sky = np.broadcast_to(np.asarray(stars['bgmed_per_pix'], np.float64).reshape(-1), x.shape) if 'bgmed_per_pix' in keys else np.zeros(x.size)
        sat = np.asarray(stars['psbl_sat']).astype(bool).reshape(-1) if 'psbl_sat' in keys else np.zeros(x.size, bool)
        if not (x.size == y.size == f.size == sky.size == sat.size):
            raise ValueError('the star list\'s columns differ in length')
        return x, y, f, np.array(sky), sat

    def _r_fit(self, fwhm):
        if self.fit_radius is not None:
            return self.fit_radius
        fwhm = float(fwhm) if fwhm is not None and math.isfinite(float(fwhm)) and float(fwhm) > 0 else 0.0
        return min(max(2.0, fwhm), 32.0)

    # -- tensors -----------------------------------------------------------------------------------------
    def build(self, image, stars, fwhm=None, gain=0.0):
        """The ePSF of a float32 device image from a star list (see star_columns).  fwhm: of the list's header, for the default
        fit radius.  Returns ops.epsf_build's dict plus stamp (ops.epsf_stamp) and keeps the grid for photometry() and subtract();
        TooFewStars if fewer than 3 stars qualify."""
        from .. import ops
        _common.need_image_f32(image)
        x, y, f, sky, sat = self.star_columns(stars)
        r_fit = self._r_fit(fwhm)
        out = ops.epsf_build(image, x, y, f, sky, self.oversampling, self.radius, r_fit, sat, self.max_stars, self.niter, self.tol, self.sigma,
                             self.maxiters, self.smoothing, self.min_count, self.fit_sky, gain, self.readnoise, self.max_iter, min_stars=MIN_STARS)
        index = out['index']
        if index.size < MIN_STARS:
            raise TooFewStars(f'{index.size} of the {x.size} stars are isolated, unsaturated and inside the image: {MIN_STARS} are needed.')
        out['stamp'] = ops.epsf_stamp(out['epsf'], self.oversampling)
        self.epsf = out['epsf']
        self._logger.info('ePSF: %d stars, oversampling %d, radius %d, fit radius %.2f, %d rounds, last change %.3g of the peak' % (
            index.size, self.oversampling, self.radius, r_fit, out['niter'], out['change'][-1]))
        return out

    def _grid(self, epsf):
        epsf = self.epsf if epsf is None else epsf
        if epsf is None:
            raise ValueError('no ePSF yet: call build() or load_psf() first, or give epsf')
        return epsf

    def load_psf(self, psf_file):
        """Takes the grid of a PSF.FITS (write_psf) for photometry() and subtract(); its oversampling and radius become this object's."""
        import torch
        grid, o, r = self.read_psf(psf_file)
        self.oversampling, self.radius = o, r
        self.epsf = torch.from_numpy(grid).cuda()
        return self.epsf

    def photometry(self, image, stars, passes=1, epsf=None, fwhm=None, gain=0.0):
        """PSF-fitting photometry of every star of the list with the ePSF of the last build() or load_psf() (or the grid `epsf`, a
        float32 device tensor of this oversampling).  passes = 2: every star is fitted again on the image minus the other stars'
        models of the first pass.
        Returns dict(records: float64 NumPy [n, 8], ops.EPSF_REC_COLUMNS; columns: the PHOT_COLUMNS as arrays; r_fit)."""
        from .. import ops
        _common.need_image_f32(image)
        if passes not in (1, 2):
            raise ValueError(f'passes = {passes!r}; allowed: 1, 2')
        epsf = self._grid(epsf)
        x, y, f, sky, _ = self.star_columns(stars)
        r_fit = self._r_fit(fwhm)
        init = np.stack([f, x, y, sky], axis=1)
        rec = ops.epsf_fit(image, init, epsf, self.oversampling, r_fit, self.fit_sky, gain, self.readnoise, self.max_iter).cpu().numpy()
        if passes == 2:
            ok = rec[:, 7] > 0
            first = np.where(ok[:, None], rec[:, :3], np.array([0.0, 0.0, 0.0]))        # a failed star has no model: nothing to add back
            _, resid = ops.epsf_render(image, first, epsf, self.oversampling, model=False)
            start = np.where(ok[:, None], rec[:, :4], init)
            rec = ops.epsf_fit(resid, start, epsf, self.oversampling, r_fit, self.fit_sky, gain, self.readnoise, self.max_iter,
                               prev=first).cpu().numpy()
        cols = dict(flux_fit=rec[:, 0].copy(), x_fit=rec[:, 1].copy(), y_fit=rec[:, 2].copy(), sky_fit=rec[:, 3].copy(), chi2=rec[:, 4].copy(),
                    fit_ok=rec[:, 7] > 0)
        self._logger.info('PSF photometry: %d of %d stars fitted (%d pass%s, fit radius %.2f)' % (
            int(cols['fit_ok'].sum()), len(rec), passes, 'es' if passes == 2 else '', r_fit))
        return dict(records=rec, columns=cols, r_fit=r_fit)

    def subtract(self, image, records, model=False, epsf=None):
        """The image minus the models of the fitted stars (records: photometry()'s; failed fits are left in) under the ePSF of the
        last build() or load_psf() (or `epsf`).  Returns the residual, or (residual, model) with model=True: float32 device planes."""
        from .. import ops
        _common.need_image_f32(image)
        epsf = self._grid(epsf)
        rec = np.asarray(records, np.float64).reshape(-1, 8)
        m, r = ops.epsf_render(image, rec[rec[:, 7] > 0, :3], epsf, self.oversampling, model=bool(model))
        return (r, m) if model else r

    # -- files ---------------------------------------------------------------------------------------------
    def _gain(self, hdr):
        if self.gain_keyword and self.gain_keyword in hdr:
            try:
                g = float(hdr[self.gain_keyword])
                return g if math.isfinite(g) and g > 0 else 0.0
            except (TypeError, ValueError):
                pass
        return 0.0

    def _read_inputs(self, image_file, stars_file):
        image, hdr = _common.read_image_f32(self._logger, image_file)
        _common.check_file_exists(self._logger, stars_file)
        cols, _, prim = fitsio.read_table(str(stars_file), 'AP_L1MAG')
        return image, hdr, cols, prim, prim.get('AP_FWHM', None), self._gain(hdr)

    def build_files(self, image_file, stars_file, psf_file, overwrite=True):
        """IMAGE.FITS and the star list of ap_find_stars in, PSF.FITS out (write_psf).  Returns build()'s dict; TooFewStars as build()."""
        image, _, cols, _, fwhm, gain = self._read_inputs(image_file, stars_file)
        built = self.build(image, cols, fwhm=fwhm, gain=gain)
        self.write_psf(psf_file, built, overwrite)
        return built

    def photometry_files(self, image_file, stars_file, psf_file, phot_file, passes=1, overwrite=True):
        """Photometry with the ePSF of an existing PSF.FITS: PHOT.FITS is the list's AP_L1MAG table plus the PHOT_COLUMNS.  Returns
        photometry()'s dict."""
        image, _, cols, prim, fwhm, gain = self._read_inputs(image_file, stars_file)
        self.load_psf(psf_file)
        phot = self.photometry(image, cols, passes=passes, fwhm=fwhm, gain=gain)
        self._write_phot(phot_file, cols, prim, phot, psf_file, passes, overwrite)
        return phot

    def subtract_files(self, image_file, stars_file, psf_file, residual_file=None, model_file=None, passes=1, overwrite=True):
        """The residual and / or the model image from an existing PSF.FITS (the stars are fitted first).  Returns photometry()'s dict."""
        image, hdr, cols, _, fwhm, gain = self._read_inputs(image_file, stars_file)
        self.load_psf(psf_file)
        phot = self.photometry(image, cols, passes=passes, fwhm=fwhm, gain=gain)
        self._write_planes(image, hdr, phot, residual_file, model_file, overwrite)
        return phot

    def _write_phot(self, phot_file, cols, prim, phot, psf_file, passes, overwrite):
        table = dict(cols)
        table.update(phot['columns'])
        fitsio.write_table(str(phot_file), [('AP_L1MAG', table, {'xcenter': 'pix', 'ycenter': 'pix', 'x_fit': 'pix', 'y_fit': 'pix'},
                                             [('PSFFILE', str(psf_file)), ('PSFRFIT', float(phot['r_fit'])), ('PSFPASS', int(passes))])],
                           header=prim, overwrite=overwrite)
        self._logger.info(f'Wrote {phot_file}')

    def _write_planes(self, image, hdr, phot, residual_file, model_file, overwrite):
        resid, model = self.subtract(image, phot['records'], model=True)
        out_hdr = hdr.copy()
        out_hdr['HISTORY'] = f'ApEmpiricalPsf: {int(phot["columns"]["fit_ok"].sum())} stars modelled with the ePSF'
        named = ([(residual_file, resid)] if residual_file else []) + ([(model_file, model)] if model_file else [])
        _common.write_images(self._logger, named, out_hdr, overwrite)

    def run_files(self, image_file, stars_file, psf_file, phot_file=None, residual_file=None, model_file=None, passes=1, overwrite=True):
        """ap_epsf: build, and what is named of photometry, residual and model, reading the inputs once.  Returns dict(status, build,
        photometry)."""
        image, hdr, cols, prim, fwhm, gain = self._read_inputs(image_file, stars_file)
        try:
            built = self.build(image, cols, fwhm=fwhm, gain=gain)
        except TooFewStars as exc:
            self._logger.error(str(exc))
            return dict(status=TOO_FEW_STARS, build=None, photometry=None)
        self.write_psf(psf_file, built, overwrite)
        phot = None
        if phot_file or residual_file or model_file:
            phot = self.photometry(image, cols, passes=passes, fwhm=fwhm, gain=gain)
        if phot_file:
            self._write_phot(phot_file, cols, prim, phot, psf_file, passes, overwrite)
        if residual_file or model_file:
            self._write_planes(image, hdr, phot, residual_file, model_file, overwrite)
        return dict(status=NOMINAL, build=built, photometry=phot)

    def write_psf(self, psf_file, built, overwrite=True):
        """PSF.FITS: the primary HDU is the stamp (odd, square, sum 1: what ap_deconvolve --psf reads), the extension EPSF the grid."""
        hdr = fitsio.Header()
        cards = {'OVERSAMP': (int(built['o']), 'grid nodes per pixel'), 'RADIUS': (int(built['R']), '[pix] radius of the stamp'),
                 'NSTARS': (int(built['index'].size), 'stars the ePSF was built from'), 'NITER': (int(built['niter']), 'rounds of the build'),
                 'RFIT': (float(built['r_fit']), '[pix] radius of the fits')}
        for k, v in cards.items():
            hdr[k] = v
        grid = built['epsf'].cpu().numpy() if hasattr(built['epsf'], 'cpu') else np.asarray(built['epsf'], np.float32)
        fitsio.write(str(psf_file), built['stamp'], header=hdr, overwrite=overwrite, extensions=[('EPSF', grid, cards)])
        self._logger.info(f'Wrote {psf_file}')

    @staticmethod
    def read_psf(psf_file):
        """(grid float32 NumPy, oversampling, radius) of a PSF.FITS."""
        grid, eh = fitsio.read_extension(str(psf_file), 'EPSF')
        return np.ascontiguousarray(grid, np.float32), int(eh['OVERSAMP']), int(eh['RADIUS'])
