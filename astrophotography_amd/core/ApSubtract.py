"""ApSubtract - optimal image subtraction: D = I - (T (x) K + B) with a convolution kernel K(u, v; x, y) that varies over the field and
a background B(x, y), fitted by least squares on stamps around stars (Alard & Lupton 1998; Alard 2000 - the method of ISIS and
HOTPANTS).

The reference has no such stage, so it is defined by this project (restated in tests/subtract_model.py).  Two uses: the
difference of two epochs (novae, supernovae, variable stars, asteroids), and, with a narrow-band image as I and the continuum image
as T, the continuum subtraction whose PSF match may be elongated, skewed and different in every corner - the spatially varying
alternative to ApContinuumSubtract.  Both inputs are float32 images on one pixel grid, NaN meaning "no data".

  device  the normal equations of every stamp and the application of the fitted kernel (csrc/subtract.hip), the star search and the
          FWHM fits behind a missing star list, FITS decode and encode
  host    the basis, the choice of the stamps, the solve with its stamp rejection (float64), the composite kernels, headers

Out of scope: a delta-function basis, Gaussian widths chosen from the FWHMs, a photometric scale that varies over the field,
variance planes and a noise image, rejection of pixels inside stamps, several GPUs.
"""
import math
import os

import numpy as np

from .. import fitsio
from . import _common

DONE, BAD_INPUT, NO_FIT = 0, 1, 2
CARDS = ('SUBSCALE', 'SUBKDEG', 'SUBBDEG', 'SUBRAD', 'SUBNBAS', 'SUBSTAMP', 'SUBNUSED', 'SUBNREJ', 'SUBCHI2', 'SUBCONV', 'SUBIMG', 'SUBTMPL')


class ApSubtract:
    """Optimal image subtraction of a template from an image (device tensors or FITS files)."""

    def __init__(self, loglevel='INFO', sigmas=(0.7, 1.5, 3.0), degrees=(6, 4, 2), radius=10, kernel_degree=2, bg_degree=1, stamp=15,
                 regions=(4, 4), per_region=5, convolve='template', satlevel=None, gain_keyword=None, readnoise=0.0, k=3.0, rounds=3,
                 search_fwhm=3.0, search_nsigma=7.0):
        """sigmas, degrees, radius: the kernel basis (ops.kernel_basis).  kernel_degree, bg_degree: of the spatial polynomials, 0 .. 3.
        stamp: half-size of the stamps, 1 .. 15.  regions = (nx, ny), per_region: the brightest per_region stars of every cell become
        stamps.  convolve: 'template', 'image' or 'auto' (the one with the smaller measured FWHM).  satlevel: stars whose list peak
        reaches it are not used.  gain_keyword (the *_files forms), readnoise (ADU): weights 1 / (readnoise^2 / gain^2 + max(O, 0) / gain),
        O the image that is not convolved (the image, or with convolve='image' the template).
        k, rounds: the stamp rejection."""
        from .. import ops
        self._loglevel = loglevel
        self._logger = _common.make_logger('ApSubtract', loglevel)
        self.basis = ops.kernel_basis(sigmas, degrees, radius)
        self.kernel_degree, self.bg_degree = ops._sub_degree(kernel_degree, 'kernel_degree'), ops._sub_degree(bg_degree, 'bg_degree')
        if convolve not in ('template', 'image', 'auto'):
            raise ValueError(f"Unexpected convolve {convolve!r}. Allowed: 'template', 'image', 'auto'")
        self.stamp, self.regions, self.per_region = int(stamp), (int(regions[0]), int(regions[1])), int(per_region)
        if not 1 <= self.stamp <= 15 or min(self.regions) < 1 or self.per_region < 1 or not float(readnoise) >= 0 or not float(k) > 0 or int(rounds) < 0:
            raise ValueError('stamp must be 1 .. 15, regions and per_region >= 1, readnoise >= 0, k > 0 and rounds >= 0')
        self.convolve, self.satlevel, self.gain_keyword, self.readnoise = convolve, satlevel, gain_keyword, float(readnoise)
        self.k, self.rounds = float(k), int(rounds)
        self.search_fwhm, self.search_nsigma = float(search_fwhm), float(search_nsigma)

    # -- pieces -----------------------------------------------------------------------------------------
    def find_stars(self, image, name='image'):
        """(FWHM, stars [k, 4] = x, y, flux, peak) of the image's own stars, as ApContinuumSubtract.measure_fwhm finds them."""
        from .ApFindStars import ApFindStars
        fs = ApFindStars.from_device(image, search_fwhm=self.search_fwhm, search_nsigma=self.search_nsigma, loglevel=self._loglevel,
                                     fitsimg=name)
        fwhm = fs.measure_fwhm(None)
        if not (np.isfinite(fwhm[0]) and fwhm[0] > 0):
            raise RuntimeError(f'Could not measure the FWHM of the {name} ({fwhm[2]} stars fitted): give fwhm=(image, template) or a star list.')
        t = fs._phot_table
        peak = np.asarray(t['peak_adu'], np.float64)
        flux = np.asarray(t['aperture_sum'], np.float64) if 'aperture_sum' in t else peak
        self._logger.info(f'Measured FWHM of the {name}: {fwhm[0]:.3f} pixels; {len(peak)} stars')
        return float(fwhm[0]), np.stack([np.asarray(t['xcenter'], np.float64), np.asarray(t['ycenter'], np.float64), flux, peak], 1)

    @staticmethod
    def star_array(stars):
        """[k, 3] or [k, 4] = x, y, flux[, peak] from such an array, or from a dict with xcenter, ycenter, peak_adu[, aperture_sum]."""
        if isinstance(stars, dict):
            peak = np.asarray(stars['peak_adu'], np.float64)
            flux = np.asarray(stars['aperture_sum'], np.float64) if 'aperture_sum' in stars else peak
            return np.stack([np.asarray(stars['xcenter'], np.float64), np.asarray(stars['ycenter'], np.float64), flux, peak], 1)
        a = np.asarray(stars.cpu() if hasattr(stars, 'cpu') else stars, np.float64)
        if a.ndim != 2 or a.shape[1] not in (3, 4):
            raise ValueError('stars must be [k, 3] (x, y, flux) or [k, 4] (x, y, flux, peak), got shape %s' % (a.shape,))
        return a

    # -- tensors -----------------------------------------------------------------------------------------
    def subtract(self, image, template, stars=None, mask=None, fwhm=None, gain=0.0, matched=False):
        """image, template: float32 device tensors [H, W] on one grid.  stars: see star_array (x = column); None: the template's own
        stars (ApFindStars.from_device).  mask: non-zero pixels refuse the stamps they fall in.  fwhm = (image, template) for
        convolve='auto' (measured when None).  Raises ops.SubtractNoFit when too few stamps are usable.
        Returns dict(image = D, report[, matched]); the report holds the fit (ops.subtract_fit) and the counts."""
        from .. import ops
        if tuple(image.shape) != tuple(template.shape):
            raise RuntimeError(f'The image is {tuple(image.shape)} and the template {tuple(template.shape)}: image subtraction needs both '
                               'on one pixel grid (ap_register / ap_coadd --center/--pixelscale/--image_size).')
        for name, t in (('image', image), ('template', template)):
            _common.need_image_f32(t, name)
        convolve = self.convolve
        if convolve == 'auto' and fwhm is None:
            fw_t, st_t = self.find_stars(template, 'template')
            fw_i, _ = self.find_stars(image, 'image')
            fwhm = (fw_i, fw_t)
            if stars is None:
                stars = st_t
        if stars is None:
            _, stars = self.find_stars(template, 'template')
        st = self.star_array(stars)
        r = ops.optimal_subtract(image, template, stars=st, mask=mask, sigmas=self.basis['sigmas'], degrees=self.basis['degrees'],
                                 radius=self.basis['radius'], kernel_degree=self.kernel_degree, bg_degree=self.bg_degree, half=self.stamp,
                                 regions=self.regions, per_region=self.per_region, satlevel=self.satlevel, gain=gain,
                                 readnoise=self.readnoise, k=self.k, rounds=self.rounds, convolve=convolve, fwhm=fwhm, matched=matched)
        usable = r['status'] == 0
        chi2 = float(np.median(r['chi2'][r['kept']]))
        report = dict(scale=r['a0'], kernel_degree=self.kernel_degree, bg_degree=self.bg_degree, radius=self.basis['radius'],
                      n_basis=self.basis['nb'], stamps=len(r['centers']), used=int(r['kept'].sum()), rejected=int((usable & ~r['kept']).sum()),
                      refused=int((~usable).sum()), chi2=chi2, convolve=r['convolve'], cond=r['cond'], rounds=r['rounds'], fit=r)
        self._logger.info('Image subtraction (%s convolved): scale a0 = %.6g, %d stamps used, %d rejected, %d refused, median chi2 = %.4g, '
                          'condition number %.3g' % (r['convolve'], r['a0'], report['used'], report['rejected'], report['refused'], chi2, r['cond']))
        out = dict(image=r['diff'], report=report)
        if matched:
            out['matched'] = r['matched']
        return out

    def kernel_cube(self, report, shape, lattice=3):
        """The fitted kernel at a lattice x lattice grid of positions: float32 [lattice^2, 2 r + 1, 2 r + 1], row-major positions."""
        from .. import ops
        H, W = shape
        pos = [(int(round((i + 0.5) * W / lattice - 0.5)), int(round((j + 0.5) * H / lattice - 0.5))) for j in range(lattice) for i in range(lattice)]
        return np.stack([ops.subtract_kernel_at(report['fit'], x, y, shape) for x, y in pos]).astype(np.float32), pos

    # -- files ---------------------------------------------------------------------------------------------
    @staticmethod
    def read_star_list(path):
        """The stars of a source list written by ap_find_stars (extension AP_L1MAG): dict(xcenter, ycenter, peak_adu[, aperture_sum])."""
        cols, _, _ = fitsio.read_table(str(path), 'AP_L1MAG')
        return {k: np.asarray(cols[k], np.float64) for k in ('xcenter', 'ycenter', 'peak_adu', 'aperture_sum') if k in cols}

    def _gain(self, hdr):
        if self.gain_keyword and self.gain_keyword in hdr:
            try:
                g = float(hdr[self.gain_keyword])
                return g if math.isfinite(g) and g > 0 else 0.0
            except (TypeError, ValueError):
                pass
        return 0.0

    def subtract_files(self, image_file, template_file, output_file, stars=None, mask_file=None, matched_out=None, kernel_out=None,
                       overwrite=True):
        """FITS in, FITS out (float32).  stars: a source list of ap_find_stars (a file name; its positions are in the common grid) or
        what subtract() takes.  mask_file: a FITS image, non-zero = refuse the stamps there.  matched_out: the matched image
        T (x) K + B.  kernel_out: the kernel at a 3 x 3 lattice of positions as a FITS cube.  The output header is the image file's
        plus the SUB* cards and HISTORY.  Returns the report."""
        import torch
        image, hdr = _common.read_image_f32(self._logger, image_file)
        template, _ = _common.read_image_f32(self._logger, template_file)
        if tuple(image.shape) != tuple(template.shape):
            raise ValueError(f'{image_file} is {tuple(image.shape)} and {template_file} is {tuple(template.shape)}: image subtraction needs '
                             'both on one pixel grid.')
        if isinstance(stars, (str, os.PathLike)):
            stars = self.read_star_list(stars)
        mask = None
        if mask_file is not None:
            m, _ = _common.read_image_f32(self._logger, mask_file)
            if tuple(m.shape) != tuple(image.shape):
                raise ValueError(f'{mask_file} is {tuple(m.shape)}, the images are {tuple(image.shape)}.')
            mask = (m != 0).to(torch.uint8)
        r = self.subtract(image, template, stars=stars, mask=mask, gain=self._gain(hdr), matched=matched_out is not None)
        rep = r['report']
        out_hdr = hdr.copy()
        out_hdr['SUBSCALE'] = (float(rep['scale']), 'photometric scale a0 = sum of the kernel')
        out_hdr['SUBKDEG'] = (int(rep['kernel_degree']), 'degree of the kernel variation')
        out_hdr['SUBBDEG'] = (int(rep['bg_degree']), 'degree of the background')
        out_hdr['SUBRAD'] = (int(rep['radius']), '[pix] kernel radius')
        out_hdr['SUBNBAS'] = (int(rep['n_basis']), 'basis functions')
        out_hdr['SUBSTAMP'] = (int(self.stamp), '[pix] half-size of the stamps')
        out_hdr['SUBNUSED'] = (int(rep['used']), 'stamps used')
        out_hdr['SUBNREJ'] = (int(rep['rejected'] + rep['refused']), 'stamps rejected or refused')
        out_hdr['SUBCHI2'] = (float(rep['chi2']), 'median chi2 per pixel of the stamps used')
        out_hdr['SUBCONV'] = (str(rep['convolve']).upper(), 'the image that was convolved')
        out_hdr['SUBIMG'] = (os.path.basename(str(image_file)), 'image')
        out_hdr['SUBTMPL'] = (os.path.basename(str(template_file)), 'template')
        out_hdr['HISTORY'] = f'ApSubtract: D = I - (T x K + B), a0 = {rep["scale"]:.6g}, {rep["used"]} stamps, {rep["convolve"]} convolved'
        names = [(str(output_file), r['image'])]
        if matched_out is not None:
            names.append((str(matched_out), r['matched']))
        _common.write_images(self._logger, names, out_hdr, overwrite)
        if kernel_out is not None:
            cube, pos = self.kernel_cube(rep, tuple(image.shape))
            kh = fitsio.Header()
            kh['SUBSCALE'] = (float(rep['scale']), 'photometric scale a0')
            for n, (x, y) in enumerate(pos):
                kh['KPOS%d' % n] = ('%d,%d' % (x, y), 'x,y of plane %d' % n)
            fitsio.write(str(kernel_out), cube, header=kh, overwrite=overwrite)
            self._logger.info(f'Wrote {kernel_out}')
        return rep
