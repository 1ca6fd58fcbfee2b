"""ApMeasureStars - stellar PSF size and symmetry from 2-D Gaussian fits (reference: core/ApMeasureStars.py).

Keeps the reference's constructor ``ApMeasureStars(img_data, srclist, init_fwhm, init_bglevel, full_srclist, fwhm_plot_file,
fwhm_plot_title, loglevel, quiet)``, ``median_fwhm(direction)``, ``results_table()`` and ``is_circular``.  The candidate
selection (nearest-neighbour trimming, regions, edge limits, boxes) is plain NumPy on the source tables; the fits run on the GPU,
one wavefront per star (ops.gauss2d_fit, csrc/measurestars.hip).

``img_data`` is a device tensor or an array; the tables are dicts of NumPy columns (as in ApFindStars) and are not modified:
the reference removes three columns from the caller's tables.  When no candidate survives the result is an empty table (the
reference raises a TypeError there).  A plot file is refused: matplotlib is not provided.
"""
import math

import numpy as np

from . import _common

_REGIONS = ('CN', 'TL', 'TR', 'BR', 'BL')
_DROPPED = ('aperture_sum', 'psbl_sat', 'adu_per_sec')
_FIT_DEFAULTS = {'xc_fit': 0.0, 'xc_err': 0.0, 'yc_fit': 0.0, 'yc_err': 0.0, 'ampl': 0.0, 'ampl_err': 0.0, 'fwhm_x': 0.0,
                 'fwhm_x_err': 0.0, 'fwhm_y': 0.0, 'fwhm_y_err': 0.0, 'theta': 0.0, 'theta_err': 0.0, 'axrat': 0.0, 'axrat_err': 0.0,
                 'circular': True, 'fit_ok': True, 'rchisq': 0.0}


def sigma_clipped(values, sigma=3.0, maxiters=5):
    """astropy.stats.sigma_clip(values, sigma, maxiters, cenfunc='median', stdfunc='std', masked=False) of a short float64
    vector: the surviving values, in order."""
    v = np.asarray(values, np.float64).ravel()
    v = v[np.isfinite(v)]
    for _ in range(maxiters):
        if v.size == 0:
            break
        med, std = np.median(v), np.std(v)
        keep = (v >= med - std * sigma) & (v <= med + std * sigma)
        if keep.all():
            break
        v = v[keep]
    return v


def mad_std(values):
    """astropy.stats.mad_std: the median absolute deviation times 1 / Phi^-1(3/4)."""
    v = np.asarray(values, np.float64)
    if v.size == 0:
        return float('nan')
    return float(np.median(np.abs(v - np.median(v))) * 1.482602218505602)


class ApMeasureStars:
    """Measures stellar PSF size and symmetry in selected stars across an input image."""

    _circ_thresh_sigma = 3.0

    def __init__(self, img_data, srclist, init_fwhm, init_bglevel, full_srclist, fwhm_plot_file, fwhm_plot_title, loglevel, quiet):
        if fwhm_plot_file is not None:
            raise NotImplementedError('ApMeasureStars cannot plot the fits (matplotlib is not provided): pass fwhm_plot_file=None.')
        self._img_data = img_data
        self._init_fwhm = init_fwhm
        self._init_bglvl = init_bglevel
        self._loglevel = loglevel
        self._quiet = quiet
        self._plot_title = fwhm_plot_title
        self._logger = _common.make_logger('ApMeasureStars', loglevel)
        self._num_per_reg = 5
        self._skip_brightest = 0
        self._full_srcs = {k: np.asarray(v) for k, v in full_srclist.items() if k not in _DROPPED}
        keep = np.asarray(srclist['psbl_sat']) == False                                    # noqa: E712
        self._init_srcs = {k: np.asarray(v)[keep] for k, v in srclist.items() if k not in _DROPPED}
        self._logger.info(f'Size of input trimmed source list (filtered): {len(self._init_srcs["id"])}')
        self._logger.info(f'Size of full source list used for neighbor removal: {len(self._full_srcs["id"])}')
        self._rows, self._cols = int(img_data.shape[0]), int(img_data.shape[1])
        self._fit_box_initialization()
        self._fit_table = self._select_candidates()
        self._calculate_boxes()
        self._do_fitting()

    # -- host: plain NumPy ------------------------------------------------------------------------------
    def _fit_box_initialization(self):
        self._box_width_pix = max(2 * int(3.0 * self._init_fwhm), 12)
        self._edge_excl_pix = 2 * int(math.ceil(self._box_width_pix / 4))
        self._logger.debug(f'Adopting a fit box width of {self._box_width_pix} pixels, edge exclusion of {self._edge_excl_pix} pixels.')

    def _trim_neighbors(self, chunk=1024):
        """Drops the stars of _init_srcs with a neighbour of _full_srcs closer than the box width (the second-smallest distance:
        the smallest is the star itself)."""
        rad = self._box_width_pix
        x, y = np.asarray(self._init_srcs['xcenter'], np.float64), np.asarray(self._init_srcs['ycenter'], np.float64)
        fx, fy = np.asarray(self._full_srcs['xcenter'], np.float64), np.asarray(self._full_srcs['ycenter'], np.float64)
        nn = np.full(x.size, np.inf)
        if fx.size >= 2:
            for s in range(0, x.size, chunk):
                dx = x[s:s + chunk, None] - fx[None, :]
                dy = y[s:s + chunk, None] - fy[None, :]
                d2 = dx * dx + dy * dy
                nn[s:s + chunk] = np.sqrt(np.partition(d2, 1, axis=1)[:, 1])
        self._init_srcs['nn_dist'] = nn
        mask = nn >= rad
        removed = int(x.size - mask.sum())
        self._init_srcs = {k: v[mask] for k, v in self._init_srcs.items()}
        self._logger.info(f'Nearest neighbor filtering removed {removed} stars from consideration.')

    def _select_candidates(self):
        """Up to five of the brightest stars of the centre (CN) and of each outer quadrant, away from the image edges."""
        self._trim_neighbors()
        t = self._init_srcs
        radius = float(min(self._cols, self._rows)) / 4
        xcen, ycen = float(self._cols) / 2, float(self._rows) / 2
        t['dx'] = np.asarray(t['xcenter'], np.float64) - xcen
        t['dy'] = np.asarray(t['ycenter'], np.float64) - ycen
        t['radius'] = np.sqrt(np.square(t['dx']) + np.square(t['dy']))
        is_right, is_top = t['dx'] >= 0, t['dy'] >= 0
        region = np.full(len(t['dx']), 'XX', dtype='<U2')
        region[is_top & is_right] = 'TR'
        region[is_top & ~is_right] = 'TL'
        region[~is_top & is_right] = 'BR'
        region[~is_top & ~is_right] = 'BL'
        region[t['radius'] <= radius] = 'CN'
        t['region'] = region
        # the edge limits as the reference writes them (:899-902): they are not symmetric
        xmin, xmax = self._edge_excl_pix - 1, self._cols - self._edge_excl_pix - 1
        ymin, ymax = self._edge_excl_pix, self._rows - self._edge_excl_pix - 1
        ok = (t['xcenter'] >= xmin) & (t['xcenter'] <= xmax) & (t['ycenter'] >= ymin) & (t['ycenter'] <= ymax)
        self._logger.debug(f'There are {int(ok.sum())} stars more than {self._edge_excl_pix} pixels away from the edge of the detector.')
        rows = []
        for reg in _REGIONS:
            idx = np.nonzero(ok & (region == reg))[0]
            if idx.size == 0:
                self._logger.warning(f'There are no candidates in the {reg} region.')
                continue
            idx = idx[np.argsort(np.asarray(t['magnitude'])[idx], kind='stable')]
            rows.append(idx[self._skip_brightest:self._skip_brightest + self._num_per_reg] if idx.size >= self._num_per_reg
                        else idx)
        sel = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        return {k: np.asarray(v)[sel] for k, v in t.items()}

    def _calculate_boxes(self):
        half_width = self._box_width_pix / 2
        t = self._fit_table
        nx = np.rint(np.asarray(t['xcenter'], np.float64)).astype(int)
        ny = np.rint(np.asarray(t['ycenter'], np.float64)).astype(int)
        t['xmin'], t['xmax'] = nx - half_width, nx + half_width
        t['ymin'], t['ymax'] = ny - half_width, ny + half_width

    # -- device ---------------------------------------------------------------------------------------
    def _do_fitting(self):
        from .. import ops
        t = self._fit_table
        n = len(t['id'])
        self._logger.info(f'Starting to fit Const2D+Gaussian2D model to {n} star cutouts.')
        if n == 0:
            for k, v in _FIT_DEFAULTS.items():
                t[k] = np.zeros(0, bool if isinstance(v, bool) else np.float64)
            return
        r = ops.gauss2d_fit(self._img_data, t['xcenter'], t['ycenter'], t['peak_adu'], t['bgmed_per_pix'], self._init_fwhm,
                            box_width=self._box_width_pix)
        for k in _FIT_DEFAULTS:
            t[k] = r[k]
        t['bg_fit'] = r['bg_fit']
        for i in np.nonzero(~r['fit_ok'])[0]:
            self._logger.warning(f'Non-nominal fit status for star {i}')

    # -- results ---------------------------------------------------------------------------------------
    @classmethod
    def is_circular(cls, fwhm_x, fwhm_y, fwhm_xerr, fwhm_yerr):
        """True if fwhm_y is within _circ_thresh_sigma standard deviations (fwhm_yerr) of fwhm_x."""
        with np.errstate(all='ignore'):
            sigma = np.float64(math.fabs(fwhm_y - fwhm_x)) / np.float64(fwhm_yerr)
        return not bool(sigma > cls._circ_thresh_sigma)

    def median_fwhm(self, direction):
        """(sigma-clipped median of the fitted FWHM over the stars that fitted, its MAD standard deviation, values used) for
        direction 'both', 'x' or 'y'."""
        ok = np.asarray(self._fit_table['fit_ok'], bool)
        ok_x = np.asarray(self._fit_table['fwhm_x'], np.float64)[ok]
        ok_y = np.asarray(self._fit_table['fwhm_y'], np.float64)[ok]
        if 'both' in direction:
            ok_fwhm = np.concatenate((ok_x, ok_y))
        elif 'x' in direction:
            ok_fwhm = ok_x
        elif 'y' in direction:
            ok_fwhm = ok_y
        else:
            raise ValueError(f'Unexpected direction={direction}: expecting "both", "x" or "y".')
        clipped = sigma_clipped(ok_fwhm, sigma=3.0, maxiters=5)
        num_used = len(clipped)
        if num_used == 0:
            return (float('nan'), float('nan'), 0)
        return (float(np.median(clipped)), mad_std(clipped), num_used)

    def results_table(self):
        """The fit results: a dict of NumPy columns, one row per fitted star."""
        return self._fit_table
