"""ApRemoveGradient - removal of the large-scale sky gradient of a finished co-add (light pollution, moonlight, residual vignetting):
the step PixInsight calls DBE / ABE and Siril background extraction.

The reference has no such stage, so it is defined by this project (restated in tests/gradient_model.py; PARITY UNPINNED).
It sits between ap_coadd / ap_drizzle and ap_continuum_subtract, ap_deconvolve, ap_multiscale and ap_composite, which all take one
sky level per image.

  device  the source mask (the ops ApMeasureBackground._make_source_mask calls), the sigma-clipped median of every sample box, the
          fitted surface on a coarse lattice in float64, and one pass over the image that interpolates the lattice and subtracts
          or divides (csrc/gradient.hip), FITS decode and encode
  host    where the samples lie, and the robust fit of a polynomial or a thin-plate spline to a few hundred of them (ops.fit_surface)

Out of scope: kriging, per-channel linked fits and colour neutralisation, an iterated source mask, samples of other
shapes, a surface on the coarse mesh of ApMeasureBackground, multi-GPU.
"""
import math
import os

import numpy as np

from . import _common

MODELS = ('poly', 'tps')
MODES = ('subtract', 'divide')
CARDS = ('GRADMODE', 'GRADMODL', 'GRADNSMP', 'GRADNREJ', 'GRADSMTH', 'GRADSTEP', 'GRADPED', 'GRADRMS')


class ApRemoveGradient:
    """Fits a smooth surface to sigma-clipped samples of the sky and subtracts it from (or divides it into) a float32 image."""

    def __init__(self, loglevel='INFO'):
        self._loglevel = loglevel
        self._logger = _common.make_logger('ApRemoveGradient', loglevel)

    # -- tensors -------------------------------------------------------------------------------------------------------------
    def source_mask(self, image):
        """The source mask of ApMeasureBackground: uint8 device tensor [H, W]."""
        from .ApMeasureBackground import ApMeasureBackground
        return ApMeasureBackground(self._loglevel)._make_source_mask(image)

    def remove(self, image, mask=None, model='poly', degree=3, smoothing=0.1, samples_per_row=16, box_radius=12, samples=None, exclude=(),
               mode='subtract', pedestal=None, k_high=2.0, k_low=3.0, max_rounds=5, step=16, sigma=3.0, maxiters=5, min_fraction=0.5,
               want_surface=True, out=None):
        """image: float32 device tensor [H, W], NaN = no data.  mask: non-zero pixels take no part in the samples; None builds the
        source mask of ApMeasureBackground.  samples: [K, 2] whole-pixel centres (x, y) in place of the automatic grid of
        samples_per_row columns; exclude: rectangles (x0, y0, x1, y1) whose samples are dropped.  A sample is used when at least
        min_fraction of its in-image pixels survive the clip.  pedestal: added back after the subtraction (the level the image is
        scaled to in 'divide'); None: the median of the kept samples.  out may be the image.

        Returns dict(image, surface (float32 plane or None), samples (float64 [K, 5]: x, y, value, sigma, kept), kept, model,
        pedestal, sigma_r, n_used)."""
        from .. import ops
        _common.need_image_f32(image)
        if model not in MODELS:
            raise ValueError(f'Unexpected model {model!r}. Allowed models are: {list(MODELS)}')
        if mode not in MODES:
            raise ValueError(f'Unexpected mode {mode!r}. Allowed modes are: {list(MODES)}')
        if not 0.0 <= float(min_fraction) <= 1.0:
            raise ValueError(f'min_fraction must lie in 0 .. 1, got {min_fraction!r}')
        shape = tuple(image.shape)
        image = image.contiguous()
        if samples is None:
            centres = ops.gradient_samples(shape, samples_per_row, exclude)
        else:
            centres = np.asarray(samples.cpu() if hasattr(samples, 'cpu') else samples)
            if centres.ndim != 2 or centres.shape[1] < 2:
                raise ValueError('samples must be [K, 2] (x, y), got shape %s' % (centres.shape,))
            centres = centres[:, :2]
            centres = centres[ops.exclude_samples(centres, exclude)]
        if mask is None:
            mask = self.source_mask(image)
        stats = ops.sample_clipped_stats(image, mask, centres, box_radius, sigma, maxiters).cpu().numpy()
        centres = np.asarray(centres, np.float64).reshape(-1, 2)
        inside = ops.sample_pixels(shape, centres, box_radius)
        used = (stats[:, 2] >= 1) & (stats[:, 2] >= float(min_fraction) * inside) & np.isfinite(stats[:, 0])
        sigmas = ops.sample_sigmas(np.where(used, stats[:, 1], np.nan), stats[:, 2])
        surface, kept, sigma_r = ops.fit_surface(centres, stats[:, 0], sigmas, shape, model, degree, smoothing, k_high, k_low, max_rounds, used)
        ped = float(np.median(stats[kept, 0])) if pedestal is None else float(pedestal)
        lattice = ops.surface_lattice(surface, shape, step, device=image.device)
        r = ops.surface_apply(image, lattice, step, mode, ped, out=out, surface_out=True if want_surface else None)
        result, plane = r if want_surface else (r, None)
        table = np.column_stack([centres, stats[:, 0], np.where(used, sigmas, np.nan), kept.astype(np.float64)])
        self._logger.info('Gradient removal (%s, %s): %d samples, %d used, %d rejected by the fit, residual sigma %.6g, pedestal %.6g'
                          % (model, mode, len(centres), int(used.sum()), int(used.sum() - kept.sum()), sigma_r, ped))
        return dict(image=result, surface=plane, samples=table, kept=kept, model=surface, pedestal=ped, sigma_r=sigma_r, n_used=int(used.sum()),
                    mode=mode, step=int(step))

    # -- files ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def read_samples(path):
        """The sample centres of a file --samples_out wrote (or a user wrote by hand): float64 [K, 2] (x, y)."""
        import yaml
        with open(os.path.expanduser(str(path))) as fh:
            doc = yaml.safe_load(fh) or {}
        rows = doc.get('samples') if isinstance(doc, dict) else doc
        if not rows:
            raise ValueError(f'{path}: no samples')
        try:
            return np.array([[float(r['x']), float(r['y'])] if isinstance(r, dict) else [float(r[0]), float(r[1])] for r in rows], np.float64)
        except (KeyError, IndexError, TypeError, ValueError) as exc:
            raise ValueError(f'{path}: a sample is x, y[, value, sigma, kept]: {exc}') from None

    @staticmethod
    def write_samples(path, table):
        """x, y, value, sigma, kept of every sample, in the format read_samples reads."""
        import yaml

        def num(v):
            return float(v) if math.isfinite(v) else None
        doc = dict(samples=[dict(x=int(r[0]), y=int(r[1]), value=num(r[2]), sigma=num(r[3]), kept=bool(r[4])) for r in table])
        with open(os.path.expanduser(str(path)), 'w') as fh:
            yaml.safe_dump(doc, fh, sort_keys=False)

    def remove_files(self, input_file, output_file, background_out=None, samples_out=None, samples_file=None, overwrite=True, **kwargs):
        """FITS in, FITS out (float32).  background_out: the surface as a FITS image.  samples_out: the sample table as YAML;
        samples_file: such a file (or a hand-written list of x, y) in place of the automatic grid.  The other arguments are
        remove()'s.  The output header is the input's plus the GRAD* cards and HISTORY.  Returns remove()'s dict."""
        image, hdr = _common.read_image_f32(self._logger, input_file)
        if samples_file is not None:
            kwargs['samples'] = self.read_samples(samples_file)
        kwargs['want_surface'] = background_out is not None
        r = self.remove(image, **kwargs)
        out_hdr = hdr.copy()
        surface = r['model']
        n_used = r['n_used']
        out_hdr['GRADMODE'] = (r['mode'].upper(), 'how the sky surface was applied')
        modl = 'POLY%d' % surface['degree'] if surface['model'] == 'poly' else 'TPS'
        out_hdr['GRADMODL'] = (modl, 'model of the sky surface')
        out_hdr['GRADNSMP'] = (int(n_used), 'samples used by the fit')
        out_hdr['GRADNREJ'] = (int(n_used - r['kept'].sum()), 'of them rejected by the fit')
        out_hdr['GRADSMTH'] = (float(surface.get('smoothing', 0.0)), 'smoothing of the thin-plate spline')
        out_hdr['GRADSTEP'] = (int(r['step']), '[pix] step of the surface lattice')
        out_hdr['GRADPED'] = (float(r['pedestal']), 'pedestal')
        out_hdr['GRADRMS'] = (float(r['sigma_r']), 'robust sigma of the kept samples about the surface')
        out_hdr['HISTORY'] = f'ApRemoveGradient: {r["mode"]} {modl}, {int(r["kept"].sum())}/{len(r["kept"])} samples kept, rms {r["sigma_r"]:.4g}'
        names = [(str(output_file), r['image'])]
        _common.write_images(self._logger, names, out_hdr, overwrite)
        if background_out is not None:
            bg_hdr = out_hdr.copy()
            bg_hdr['IMAGETYP'] = 'Background Sky'
            _common.write_images(self._logger, [(str(background_out), r['surface'])], bg_hdr, overwrite)
        if samples_out is not None:
            self.write_samples(samples_out, r['samples'])
            self._logger.info(f'Wrote {samples_out}')
        return r
