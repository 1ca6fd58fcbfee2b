"""ApFindStars - star detection and aperture photometry of one frame (reference: core/ApFindStars.py).

Keeps the reference's API - the constructor ``ApFindStars(fitsimg, extnum, search_fwhm, search_nsigma, detector_bitdepth,
max_sources, nosatmask, sat_frac, loglevel, plotfile, quiet)`` (:87-201), ``source_search`` (:299-340),
``aperture_photometry(notrim=None)`` (:363-446), ``trim`` (:203-222), ``write_source_list`` (:342-361, 627-678) and
``write_ds9_region_file`` (:878-916) - over HIP kernels (csrc/findstars.hip), and adds ``from_device`` for a frame that is
already in HBM.

The reference hands the numerics to photutils (DAOStarFinder, find_peaks, aperture_photometry); photutils is not available
in the build container, so its published algorithms are restated (tests/findstars_model.py: PARITY UNPINNED) and run as:

  device  global sigma-clipped statistics (A3 kernels) -> detection threshold -> threshold mask (A4 kernel) -> 8-connected
          components >= 5 pixels dilated 11 x 11 (apgpu_source_mask_u8) -> the masked statistics (A3 on a copy with NaN)
          -> saturated peaks (apgpu_local_peaks_f32, square footprint) -> mask boxes (apgpu_mask_add_rects_u8)
          -> DAOFIND: convolution, peaks, measurement (apgpu_daofind_*) -> aperture sums and annulus medians
             (apgpu_aperture_phot_f32)
  host    the source tables (a few thousand rows): exposure scaling, magnitudes, sort, trim, files

``_sources`` and ``_phot_table`` are plain dicts of NumPy columns with the reference's column names.  ``measure_fwhm(None)``
fits Gaussians to a sample of the stars (core/ApMeasureStars.py, csrc/measurestars.hip) and ``quality_report`` /
``write_quality_report`` summarise the frame; ``plot_image`` and the plot of the fits are not provided (matplotlib).
"""
import math
from datetime import datetime

import numpy as np

from .. import fitsio
from . import _common

_KW_COMMENTS = {'EXPOSURE': '[seconds] Image exposure time',
                'DATE-OBS': 'Observation date and time',
                'OBJECT': 'Target object',
                'OBJNAME': 'Target object',
                'TELESCOP': 'Telescope used',
                'INSTRUME': 'Detector used',
                'CCD-TEMP': 'CCD temperature at start of exposure in C',
                'APTDIA': '[mm] Diameter of telescope aperture',
                'RA': 'Target right ascension',
                'DEC': 'Target declination',
                'RA-OBJ': 'Target right ascension',
                'DEC-OBJ': 'Target declination',
                'XPIXSZ': '[micrometers] X-axis pixel scale after binning',
                'YPIXSZ': '[micrometers] Y-axis pixel scale after binning',
                'FOCALLEN': '[mm] Stated telescope focal length',
                'FILTER': 'Filter used',
                'EGAIN': '[e/ADU] Gain in electrons per ADU',
                'LAT-OBS': '[deg +N WGS84] Observatory Geodetic latitude',
                'LONG-OBS': '[deg +E WGS84] Observatory Geodetic longitude',
                'ALT-OBS': '[metres] Observatort altitude above mean sea level',
                'AIRMASS': 'Airmass (multiple of zenithal airmass)'}


def _sexagesimal(value):
    """'hh mm ss.s' / 'dd:mm:ss' / a number -> float in the string's own unit, or None."""
    if isinstance(value, (int, float)):
        return float(value)
    parts = str(value).replace(':', ' ').split()
    try:
        nums = [float(p) for p in parts]
    except ValueError:
        return None
    if not 1 <= len(nums) <= 3:
        return None
    sign = -1.0 if parts[0].lstrip().startswith('-') else 1.0
    return sign * sum(abs(n) / 60.0 ** i for i, n in enumerate(nums))


class ApFindStars:
    """Find and characterize stars within a FITS image."""

    GOOD = 0
    INPUT_ERROR = 1

    def __init__(self, fitsimg, extnum, search_fwhm, search_nsigma, detector_bitdepth, max_sources, nosatmask, sat_frac,
                 loglevel, plotfile, quiet):
        self._configure(fitsimg, extnum, search_fwhm, search_nsigma, detector_bitdepth, max_sources, nosatmask, sat_frac,
                        loglevel, plotfile, quiet)
        if extnum not in (0, None):
            self._status = ApFindStars.INPUT_ERROR
            raise RuntimeError(f'Only the primary HDU (extension 0) can be read, got extension {extnum}.')
        try:
            data, hdr, _ = _common.read_fits(self._logger, fitsimg)
        except RuntimeError:
            self._status = ApFindStars.INPUT_ERROR
            raise
        self._run(self._to_device(data), hdr)

    @classmethod
    def from_device(cls, data_t, hdr=None, search_fwhm=3.0, search_nsigma=7.0, detector_bitdepth=16, max_sources=None,
                    nosatmask=False, sat_frac=0.80, loglevel='INFO', quiet=True, fitsimg='device'):
        """The same for a frame that is already on the GPU: a 2-D CUDA tensor (float32, or uint16 / float64 / integer as a
        FITS file would hold) and its header (a fitsio.Header or a dict; EXPOSURE / EXPTIME is read from it)."""
        self = cls.__new__(cls)
        self._configure(fitsimg, 0, search_fwhm, search_nsigma, detector_bitdepth, max_sources, nosatmask, sat_frac, loglevel,
                        None, quiet)
        if not getattr(data_t, 'is_cuda', False) or data_t.dim() != 2:
            raise ValueError('from_device takes a 2-D CUDA tensor')
        if hdr is None:
            hdr = {}
        if 'NAXIS1' not in hdr:
            hdr = dict(hdr.items()) if not isinstance(hdr, dict) else dict(hdr)
            hdr['NAXIS1'], hdr['NAXIS2'] = int(data_t.shape[1]), int(data_t.shape[0])
        self._run(data_t, hdr)
        return self

    # -------------------------------------------------------------------------------------------
    def _configure(self, fitsimg, extnum, search_fwhm, search_nsigma, detector_bitdepth, max_sources, nosatmask, sat_frac,
                   loglevel, plotfile, quiet):
        self._status = ApFindStars.GOOD
        self._loglevel = loglevel
        self._fitsimg = fitsimg
        self._extnum = extnum
        self._search_fwhm = search_fwhm
        self._search_nsigma = search_nsigma
        self._bitdepth = detector_bitdepth
        self._max_sources = max_sources
        self._nosatmask = nosatmask
        self._sat_frac = sat_frac
        self._plotfile = plotfile
        self._max_adu = math.pow(2, detector_bitdepth) - 1
        self._sat_thresh = math.floor(sat_frac * self._max_adu)
        self._quiet = quiet
        self._psf_table = None
        self._fwhm_both = None
        self._fwhm_x = None
        self._fwhm_y = None
        self._nsrcs_detected = 0
        self._nsrcs_photom = 0
        self._nsrcs_fitted = 0
        self._nsrcs_saturated = 0
        self._ap_fwhm_mult = 2.0          # Aperture radius is this times search_fhwm
        self._logger = _common.make_logger('ApFindStars', loglevel)

    @staticmethod
    def _to_device(data):
        import torch
        from .. import ops
        a = np.asarray(data)
        if a.dtype == np.uint16:
            return ops.to_device_u16(a)
        if a.dtype in (np.uint32, np.uint64):
            a = a.astype(np.int64)
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def _run(self, data_t, hdr):
        import torch
        from .. import ops
        self._hdr = hdr
        self._data_raw = data_t
        # the kernels work on float32 pixels (uint16 and other integers below 2^24 convert exactly)
        if data_t.dtype == torch.float32:
            d32 = data_t.contiguous()
        elif data_t.dtype == torch.uint16:
            d32 = _common.widen_u16(data_t, torch.float32)
        else:
            d32 = data_t.to(torch.float32).contiguous()
        self._data = d32
        H, W = d32.shape

        # 1. initial background estimate (:142): numpy's statistics in the file's own type
        st = ops.sigclip_global(data_t, sigma=3.0).cpu().numpy()
        self._bg_mean, self._bg_median, self._bg_stddev = float(st[0]), float(st[1]), float(st[2])
        self._logger.debug('Sigma clipped image stats: mean={:.3f}, median={:.3f}, stddev={:.3f}'.format(
            self._bg_mean, self._bg_median, self._bg_stddev))

        # 2. source mask (:146-149): detect_threshold(nsigma=2, SigmaClip(3, maxiters=10)), detect_sources(npixels=5), size 11
        s10 = ops.sigclip_global(d32, sigma=3.0, maxiters=10)
        thr = (s10[0].float() + s10[2].float() * 2.0).double()
        th = torch.stack([torch.full_like(thr, -float('inf')), thr]).contiguous()
        above, _ = ops.threshold_mask(d32, thresholds=th)
        self._source_mask, _ = ops.source_mask(above, min_pixels=5, dilate_size=11)

        # 3. the masked statistics (:151-153): astropy drops masked and non-finite values alike
        if data_t.dtype == torch.float32:
            x = d32.clone()
        elif data_t.dtype == torch.uint16:
            x = _common.widen_u16(data_t, torch.float64)
        else:
            x = data_t.to(torch.float64)
        x[self._source_mask != 0] = float('nan')
        st = ops.sigclip_global(x, sigma=3.0).cpu().numpy()
        self._bg_mean, self._bg_median, self._bg_stddev = float(st[0]), float(st[1]), float(st[2])
        self._logger.debug('Source-masked image stats: mean={:.3f}, median={:.3f}, stddev={:.3f}'.format(
            self._bg_mean, self._bg_median, self._bg_stddev))

        # 4. possibly saturated stars (:159-161, 866-876) and 5. their mask boxes (:165-185)
        self._mask = torch.zeros((H, W), dtype=torch.uint8, device=d32.device)
        self._logger.debug('Checking for possibly saturated stars or regions.')
        self._saturated_idx = self._find_saturated(d32, self._sat_thresh, self._search_fwhm)
        num_sat_candidates = len(self._saturated_idx)
        if not self._nosatmask:
            box_width = int(4 * self._search_fwhm)
            self._logger.debug(f'Excluding {num_sat_candidates} possibly saturated stars using mask boxes of half-width {box_width} pixels.')
            rects = []
            for q in self._saturated_idx:
                srow, scol = divmod(int(q), W)
                rects.append([max(0, srow - box_width + 1), min(H, srow + box_width), max(0, scol - box_width + 1),
                              min(W, scol + box_width)])
            self._sat_rects = np.asarray(rects, np.int32).reshape(-1, 4)
            if len(rects):
                ops.mask_add_rects(self._mask, self._sat_rects, value=1)
                self._mask = (self._mask != 0).to(torch.uint8)        # overlapping boxes add up: back to 0 / 1
        else:
            self._sat_rects = np.zeros((0, 4), np.int32)
            self._logger.debug(f'Retaining {num_sat_candidates} possibly saturated stars in source searching and photometry.')
        self._nsrcs_saturated = num_sat_candidates

        # 6. search and photometry
        self.source_search(self._search_fwhm, self._search_nsigma)
        self.aperture_photometry()

    def _find_saturated(self, d32, sat_thresh, search_fwhm):
        """find_peaks(data, threshold=sat_thresh, box_size=int(4 fwhm)): flat indices of the peaks, ascending (numpy int64)."""
        from .. import ops
        boxsize = int(4 * search_fwhm)
        self._logger.debug(f'Looking for possibly saturated regions above {sat_thresh} ADU separated by {boxsize} pixels.')
        if boxsize < 1:
            return np.zeros(0, np.int64)
        idx, n = ops.local_peaks(d32, boxsize, float(sat_thresh), border=0, capacity=1024)
        if n > 1024:
            idx, n = ops.local_peaks(d32, boxsize, float(sat_thresh), border=0, capacity=n)
        return idx.cpu().numpy().astype(np.int64)

    # -------------------------------------------------------------------------------------------
    def source_search(self, search_fwhm, search_nsigma):
        """Search for star-like objects with the given FWHM that have a statistical significance nsigma above the
        established background noise level."""
        from .. import ops
        self._logger.debug(f'Running DAOStarFinder with FWHM={search_fwhm:.2f} pixels, threshold={search_nsigma} BG sigma.')
        r = ops.find_stars(self._data, search_fwhm, search_nsigma * self._bg_stddev, bg_median=self._bg_median, mask=self._mask)
        cols = ('xcentroid', 'ycentroid', 'sharpness', 'roundness1', 'roundness2', 'npix', 'peak', 'flux', 'mag')
        host = {k: r[k].cpu().numpy() for k in cols}
        n = len(host['peak'])
        sources = {'id': np.arange(1, n + 1, dtype=np.int64)}
        for k in ('xcentroid', 'ycentroid', 'sharpness', 'roundness1', 'roundness2'):
            sources[k] = host[k]
        sources['npix'] = host['npix'].astype(np.int64)
        sources['sky'] = np.zeros(n)
        sources['peak'], sources['flux'], sources['mag'] = host['peak'], host['flux'], host['mag']
        self._logger.info(f'Initial source list using FHWM={search_fwhm} pixels, threshold={search_nsigma} x BG stddev, found {n} sources.')
        self._logger.debug(f'Sources with pixels exceding {self._sat_thresh} ADU will be flagged as possibly saturated.')
        sources['psbl_sat'] = sources['peak'] > self._sat_thresh
        self._logger.debug(f'There are {int(np.sum(sources["psbl_sat"]))} possibly saturated stars in the output source list.')
        if not self._quiet:
            print(self._format_table(sources))
        self._sources = sources
        self._nsrcs_detected = n

    def aperture_photometry(self, notrim=None):
        """Aperture photometry of the current sources; with notrim=True the table is not trimmed to max_sources."""
        from .. import ops
        dont_trim = bool(notrim) if notrim is not None else False
        ap_radius = math.ceil(self._ap_fwhm_mult * self._search_fwhm)
        outer_radius = math.ceil(1.5 * ap_radius)
        self._logger.debug(f'Radius of circular aperture photometry is {ap_radius} pixels.')
        self._logger.debug(f'Local BG estimation in annulus outer radius {outer_radius} pixels, inner radius {ap_radius} pixels.')
        src = self._sources
        r = ops.aperture_photometry(self._data, src['xcentroid'], src['ycentroid'],
                                    radii=(float(ap_radius), float(ap_radius), float(outer_radius)))
        bkg_median = r['bkg_median'].cpu().numpy().astype(np.float64)
        raw = r['aperture_sum_raw'].cpu().numpy()
        n = len(raw)
        phot = {'id': np.arange(1, n + 1, dtype=np.int64), 'xcenter': np.asarray(src['xcentroid'], np.float64),
                'ycenter': np.asarray(src['ycentroid'], np.float64)}
        phot['aperture_sum'] = raw - bkg_median * (math.pi * ap_radius ** 2)
        phot['peak_adu'] = src['peak']
        phot['psbl_sat'] = src['psbl_sat']
        phot['bgmed_per_pix'] = bkg_median
        exposure = None
        for kw in ('EXPOSURE', 'EXPTIME'):
            if exposure is None and kw in self._hdr:
                exposure = float(self._hdr[kw])
                self._logger.debug(f'Image exposure time [seconds]: {exposure:.2f}')
        if exposure is None:
            self._logger.warning('EXPOSURE not found in FITS header. Assuming 1 second.')
            exposure = 1
        with np.errstate(all='ignore'):
            phot['adu_per_sec'] = phot['aperture_sum'] / exposure
            phot['magnitude'] = -2.5 * np.log10(phot['adu_per_sec'])
        # Table.sort(['adu_per_sec', 'xcenter', 'ycenter'], reverse=True): the ascending lexical order, reversed
        order = np.lexsort((phot['ycenter'], phot['xcenter'], phot['adu_per_sec']))[::-1]
        phot = {k: v[order] for k, v in phot.items()}
        if not self._quiet:
            print(self._format_table(phot))
        self._phot_table = phot
        self._full_srclist = {k: v.copy() for k, v in phot.items()}
        self._create_photometry_statistics()
        if not dont_trim:
            self.trim(self._max_sources)
        self._nsrcs_photom = len(self._phot_table['id'])
        return phot

    def trim(self, max_srcs):
        """Reduce the photometry table to at most max_srcs of the brightest sources (None keeps all)."""
        nsrc = len(self._phot_table['id'])
        nuse = nsrc if max_srcs is None else min(nsrc, max_srcs)
        self._logger.debug('Selecting {} sources out of {} to write to the output source list.'.format(nuse, nsrc))
        self._phot_table = {k: v[0:nuse] for k, v in self._phot_table.items()}

    def _create_photometry_statistics(self):
        num_srcs = len(self._full_srclist['id'])
        if num_srcs == 0:
            self._phot_stats = None
            return
        a = self._full_srclist['adu_per_sec']
        idx = (0, int(num_srcs / 2), num_srcs - 1)
        self._phot_stats = tuple((float(a[i]), i) for i in idx)

    @staticmethod
    def _format_table(table):
        names = list(table)
        lines = [' '.join('%12s' % n for n in names)]
        for i in range(len(table[names[0]])):
            lines.append(' '.join(('%12d' % table[n][i]) if table[n].dtype.kind in 'iub' else ('%12.4f' % table[n][i]) for n in names))
        return '\n'.join(lines)

    # -- output ---------------------------------------------------------------------------------------
    def _build_keyword_dictionary(self, img_name, hdr, bg_median, bg_stddev):
        """key -> (value, comment) for the source list's primary header (:761-849, less the FWHM entries)."""
        kw_dict = {'IMG_FILE': (str(img_name), 'Name of image file searched for stars')}
        cols, rows = int(hdr['NAXIS1']), int(hdr['NAXIS2'])
        kw_dict['IMG_COLS'] = (cols, 'Number of columns in input image')
        kw_dict['IMG_ROWS'] = (rows, 'Number of rows in input image')
        self._logger.info('Image is {} cols x {} rows'.format(cols, rows))
        kw_dict['AP_NDET'] = (self._nsrcs_detected, 'Number of sources detected in the image.')
        kw_dict['AP_NPHOT'] = (self._nsrcs_photom, 'Number of sources final photometry.')
        kw_dict['AP_NFIT'] = (self._nsrcs_fitted, 'Number of sources used in FWHM fitting.')
        kw_dict['AP_NSIGM'] = (self._search_nsigma, 'Source searching threshold (sigma above background)')
        for kw, comment in _KW_COMMENTS.items():
            if kw in hdr:
                kw_dict[kw] = (hdr[kw], comment)
        ra = _sexagesimal(kw_dict['RA'][0]) if 'RA' in kw_dict else None
        dec = _sexagesimal(kw_dict['DEC'][0]) if 'DEC' in kw_dict else None
        if ra is not None and dec is not None:
            self._logger.info('Approximate coordinates: ra={:.6f} hours, dec={:.6f} deg'.format(ra, dec))
            kw_dict['APRX_RA'] = (ra * 15.0, '[deg] Approximate image center RA')
            kw_dict['APRX_DEC'] = (dec, '[deg] Approximate image center Dec')
        if 'FOCALLEN' in kw_dict and 'XPIXSZ' in kw_dict and 'YPIXSZ' in kw_dict:
            focal_len_mm = float(kw_dict['FOCALLEN'][0])
            pixsiz_x_deg = math.degrees((float(kw_dict['XPIXSZ'][0]) * 1.0e-6) / (focal_len_mm * 1.0e-3))
            pixsiz_y_deg = math.degrees((float(kw_dict['YPIXSZ'][0]) * 1.0e-6) / (focal_len_mm * 1.0e-3))
            imgsiz_x_deg, imgsiz_y_deg = cols * pixsiz_x_deg, rows * pixsiz_y_deg
            imgsiz_deg = math.sqrt(imgsiz_x_deg * imgsiz_x_deg + imgsiz_y_deg * imgsiz_y_deg)
            self._logger.info('Approximate image field of view is {:.3f} degrees across.'.format(imgsiz_deg))
            kw_dict['APRX_FOV'] = (imgsiz_deg, '[deg] Approximate diagonal size of image')
            kw_dict['APRX_XWD'] = (imgsiz_x_deg, '[deg] Approximate X-axis width of image')
            kw_dict['APRX_YHG'] = (imgsiz_y_deg, '[deg] Approximate Y-axis height of image')
            kw_dict['APRX_XPS'] = (3600.0 * pixsiz_x_deg, '[arcseconds] Approximate X-axis plate scale')
            kw_dict['APRX_YPS'] = (3600.0 * pixsiz_y_deg, '[arcseconds] Approximate Y-axis plate scale')
        if getattr(self, '_fwhm_both', None) is not None:
            kw_dict['AP_FWHM'] = (self._fwhm_both[0], '[pix] Median FWHM of fitted stars in image')
            kw_dict['AP_EFWHM'] = (self._fwhm_both[1], '[pix] MAD standard deviation of fitted FWHM')
        kw_dict['AP_BGMED'] = (float(bg_median), '[ADU] Median source-masked background level')
        kw_dict['AP_BGSTD'] = (float(bg_stddev), '[ADU] Std dev of source-masked background level')
        return kw_dict

    def write_source_list(self, output_fits_table):
        """Write the current source positions (AP_XYPOS, FITS 1-based) and photometry (AP_L1MAG, 0-based) to a FITS table,
        overwriting any existing file."""
        self._kw_dict = self._build_keyword_dictionary(self._fitsimg, self._hdr, self._bg_median, self._bg_stddev)
        self._logger.debug('Converting python 0-based coordinates to FITS 1-based pixel coordinates for XY table.')
        t = self._phot_table
        self._logger.info('Writing source list to FITS binary table {}'.format(output_fits_table))
        pri = fitsio.Header()
        for k, v in self._kw_dict.items():
            pri[k] = v
        pri['HISTORY'] = 'Created by ApFindStars at {}'.format(datetime.now().isoformat(timespec='milliseconds'))
        hdus = [('AP_XYPOS', {'X': t['xcenter'] + 1.0, 'Y': t['ycenter'] + 1.0}, {'X': 'pix', 'Y': 'pix'},
                 [('COMMENT', 'Uses FITS 1-based pixel coordinate system.')]),
                ('AP_L1MAG', t, {'xcenter': 'pix', 'ycenter': 'pix'},
                 [('COMMENT', 'Aperature photometry using the DAOFIND kernels of ApFindStars.'),
                  ('COMMENT', 'Uses python 0-based pixel coordinate system.')])]
        if getattr(self, '_psf_table', None) is not None:
            regions = ('CN', 'TL', 'TR', 'BR', 'BL')               # the table writer holds numbers only: region as an index
            psf = {k: (np.array([regions.index(r) for r in v], np.int32) if k == 'region' else v) for k, v in self._psf_table.items()}
            hdus.append(('AP_L1PSF', psf, {'xcenter': 'pix', 'ycenter': 'pix'},
                         [('COMMENT', 'PSF characterization using ApMeasureStars.'),
                          ('COMMENT', 'Uses python 0-based pixel coordinate system.'),
                          ('COMMENT', 'region: 0 CN, 1 TL, 2 TR, 3 BR, 4 BL.')]))
        fitsio.write_table(str(output_fits_table), hdus, header=pri)

    def write_ds9_region_file(self, region_file):
        """Write a ds9-format region file (image coordinates, 1-based) with one circle per star of the photometry table."""
        ap_radius = math.ceil(self._ap_fwhm_mult * self._search_fwhm)
        lines = ['# Region file format: DS9', 'image']
        t = self._phot_table
        for x, y, sid in zip(t['xcenter'], t['ycenter'], t['id']):
            lines.append('circle({:.4f},{:.4f},{:.4f}) # color=red text={{{}}}'.format(x + 1.0, y + 1.0, float(ap_radius), int(sid)))
        with open(region_file, 'w', encoding='utf-8') as f_out:
            f_out.write('\n'.join(lines) + '\n')
        self._logger.debug(f'Wrote ds9-format region file to {region_file}')

    # -- PSF measurement (ApMeasureStars) and the quality report ------------------------------------------
    def measure_fwhm(self, fwhm_plot_file, direction=None):
        """Fits 2-D Gaussians to a sample of the stars (ApMeasureStars) and returns (median FWHM, MAD standard deviation,
        values used) over 'both' axes (default), 'x' or 'y'.  A plot file cannot be written."""
        if fwhm_plot_file is not None:
            raise NotImplementedError('measure_fwhm cannot plot the fits (matplotlib is not provided): pass None.')
        from .ApMeasureStars import ApMeasureStars
        measure_stars = ApMeasureStars(self._data, self._phot_table, self._search_fwhm, self._bg_median, self._full_srclist, None,
                                       None, self._loglevel, self._quiet)
        self._psf_table = measure_stars.results_table()
        self._nsrcs_fitted = len(self._psf_table['id'])
        self._fwhm_both = measure_stars.median_fwhm('both')
        self._fwhm_x = measure_stars.median_fwhm('x')
        self._fwhm_y = measure_stars.median_fwhm('y')
        self._logger.info(f'Median FWHM (over x and y) is {self._fwhm_both[0]:.2f} +/- {self._fwhm_both[1]:.2f} pixels '
                          f'using {self._fwhm_both[2]} data points')
        if direction is None or direction == 'both':
            return self._fwhm_both
        if direction == 'x':
            return self._fwhm_x
        if direction == 'y':
            return self._fwhm_y
        raise ValueError(f'Unexpected direction={direction} passed to measure_fwhm. Expecting one of None, "both", "x" or "y".')

    def plot_image(self, plotfile):
        raise NotImplementedError('plot_image needs matplotlib, which is out of scope here.')

    def quality_report(self):
        """The reference's quality report (:947-1074) as a dict of dicts: image, background, source, saturation and PSF
        information.  Null value -999 where there is no plate scale (the reference multiplies by it all the same)."""
        null_val = -999
        self._kw_dict = self._build_keyword_dictionary(self._fitsimg, self._hdr, self._bg_median, self._bg_stddev)
        kw = self._kw_dict
        im_info = {}
        for okey, fkw in (('file', 'IMG_FILE'), ('ncols', 'IMG_COLS'), ('nrows', 'IMG_ROWS'), ('object', 'OBJECT'),
                          ('telescope', 'TELESCOP'), ('filter', 'FILTER'), ('date-obs', 'DATE-OBS'), ('exposure', 'EXPOSURE'),
                          ('ccd_temperature', 'CCD-TEMP'), ('electronic_gain', 'EGAIN'), ('airmass', 'AIRMASS'),
                          ('approx_width_deg', 'APRX_XWD'), ('approx_height_deg', 'APRX_YHG'), ('approx_xpixsiz_arcs', 'APRX_XPS'),
                          ('approx_ypixsiz_arcs', 'APRX_YPS')):
            if fkw in kw:
                v = kw[fkw][0]
                im_info[okey] = v.item() if isinstance(v, np.generic) else v
            else:
                self._logger.warning(f'Keyword {fkw} not found, not written to quality report.')
        bg_info = {'median': kw['AP_BGMED'][0], 'stddev': kw['AP_BGSTD'][0]}
        stats = self._phot_stats if getattr(self, '_phot_stats', None) else ((null_val, 0),) * 3
        src_info = {'num_detected': int(kw['AP_NDET'][0]), 'num_with_photometry': int(kw['AP_NPHOT'][0]),
                    'search_nsigma': kw['AP_NSIGM'][0], 'adups_brightest': stats[0][0], 'adups_median': stats[1][0],
                    'adups_faintest': stats[2][0]}
        sat_info = {'num_saturated_in_image': int(self._nsrcs_saturated),
                    'num_saturated_in_photometry': int(np.sum(np.asarray(self._phot_table['psbl_sat']) == True))}   # noqa: E712
        psf_info = {'num_fit': int(kw['AP_NFIT'][0])}
        have_platescale = 'APRX_XPS' in kw and 'APRX_YPS' in kw
        if not have_platescale:
            self._logger.warning('Skipping some quality reporting that requires an estimate platescale.')
        if self._psf_table is not None:
            if have_platescale:
                xps, yps = kw['APRX_XPS'][0], kw['APRX_YPS'][0]
                avg = math.sqrt(0.5 * (xps ** 2 + yps ** 2))
            else:
                xps = yps = avg = null_val
            from .ApMeasureStars import ApMeasureStars
            psf_info['circular_psf'] = ApMeasureStars.is_circular(self._fwhm_x[0], self._fwhm_y[0], self._fwhm_x[1], self._fwhm_y[1])
            for name, result, pix in (('fwhm_xandy', self._fwhm_both, avg), ('fwhm_x', self._fwhm_x, xps), ('fwhm_y', self._fwhm_y, yps)):
                psf_info[name] = {'fwhm_val_pix': float(result[0]), 'fwhm_err_pix': float(result[1]),
                                  'fwhm_val_arcs': float(result[0] * pix), 'fwhm_err_arcs': float(result[1] * pix),
                                  'num_data_pts': int(result[2])}
        return {'image_info': im_info, 'background_info': bg_info, 'source_info': src_info, 'saturation_info': sat_info,
                'psf_info': psf_info}

    def write_quality_report(self, quality_report_name):
        """Writes quality_report() as YAML (floats with six decimals, as the reference's representer)."""
        if getattr(self, '_psf_table', None) is None:
            raise NotImplementedError('write_quality_report summarises the FWHM fits: call measure_fwhm(None) first.')
        try:
            import yaml
        except ImportError as exc:                                               # pragma: no cover
            raise RuntimeError('write_quality_report needs PyYAML') from exc

        class _Dumper(yaml.SafeDumper):
            pass

        _Dumper.add_representer(float, lambda dumper, value: dumper.represent_scalar('tag:yaml.org,2002:float', '{0:.6f}'.format(value)))
        with open(quality_report_name, 'w') as write_file:
            yaml.dump(self.quality_report(), write_file, Dumper=_Dumper, indent=4, sort_keys=False)
        self._logger.info(f'Wrote image quality report to {quality_report_name}')
