"""ApComposite - colour composites of three co-added images: the step scripts/composite_all.sh hands to the external program
STIFF, which is no longer packaged and no longer compiles (composite_all.sh:34-36).

STIFF's arithmetic is not in the reference tree, so this stage is defined here (PARITY UNPINNED): the intensity
levels of each channel are exact quantiles of its finite pixels (or manual values), the luminance gets the POWER-LAW curve
Y^(1 / (gamma gamma_fac)) and the colours are stretched about the luminance by colour_sat.  One launch of the composite kernel
reads the three planes once and writes every (gamma_fac, colour_sat) variant asked for (csrc/composite.hip).

  device  quantile levels (radix select), the composite of all variants
  host    the tone tables (41 KB each), FITS input, TIFF output (tiffio)
"""
import os

import numpy as np

from .. import fitsio, tiffio
from . import _common

MAX_VARIANTS = 16
LEVEL_TYPES = ('QUANTILE', 'MANUAL')


def _three(value, name):
    a = np.asarray(value, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise ValueError(f'{name} takes one value or one per channel, got {value!r}.')
    return a


def _three_types(value, name):
    t = [value] * 3 if isinstance(value, str) else list(value)
    t = [str(v).strip().upper() for v in t]
    if len(t) != 3 or any(v not in LEVEL_TYPES for v in t):
        raise ValueError(f'{name} must be QUANTILE or MANUAL (one value or one per channel), got {value!r}.')
    return t


def variant_grid(gamma_fac, colour_sat):
    """The (gamma_fac, colour_sat) pairs of a grid, gamma_fac outermost: the loop order of composite_all.sh:234-239."""
    gf = np.asarray(gamma_fac, np.float64).reshape(-1)
    cs = np.asarray(colour_sat, np.float64).reshape(-1)
    if gf.size == 0 or cs.size == 0:
        raise ValueError('No gamma_fac or colour_sat given.')
    return [(float(g), float(s)) for g in gf for s in cs]


class ApComposite:
    """Three co-added planes (red, green, blue) -> RGB images."""

    def __init__(self, loglevel='INFO'):
        self._loglevel = loglevel
        self._logger = _common.make_logger('ApComposite', loglevel)
        self.n_finite = None            # device int64 [3] of the last levels() call
        self.variants = None            # (gamma_fac, colour_sat) of the images of the last composite() call

    # -- input ------------------------------------------------------------------------------------------
    def _planes(self, inputs):
        """[3, H, W] float32 device tensor from three FITS file names, three 2-D device tensors or one [3, H, W] tensor."""
        import torch
        if torch.is_tensor(inputs):
            planes = inputs
        else:
            inputs = list(inputs)
            if len(inputs) != 3:
                raise ValueError(f'Three inputs (red, green, blue) are needed, got {len(inputs)}.')
            parts = []
            for img in inputs:
                if isinstance(img, (str, os.PathLike)):
                    _common.check_file_exists(self._logger, img)
                    data, _ = fitsio.read_device(str(img))
                    if data is None or data.dim() != 2:
                        raise RuntimeError(f'{img}: expected a 2-D primary image.')
                    img = data
                parts.append(img)
            shapes = [tuple(p.shape) for p in parts]
            if any(p.dim() != 2 for p in parts) or len(set(shapes)) != 1:
                raise RuntimeError(f'The three images must be 2-D and of one shape, got {shapes}.')
            planes = torch.stack([p.to(device='cuda', dtype=torch.float32) for p in parts])
        if planes.dim() != 3 or planes.shape[0] != 3:
            raise RuntimeError(f'Expected [3, H, W] planes, got {tuple(planes.shape)}.')
        if not planes.is_cuda:
            raise ValueError('ApComposite works on device tensors; there is no CPU path.')
        return planes.to(torch.float32).contiguous()

    # -- levels -----------------------------------------------------------------------------------------
    def levels(self, inputs, min_level=0.60, max_level=0.999, min_type='QUANTILE', max_type='QUANTILE'):
        """The [3, 2] float32 device tensor of (lo, hi) per channel.  A level of type QUANTILE is the exact quantile of the
        channel's finite pixels (np.quantile, method='lower'), one of type MANUAL is the value given.  The defaults are the
        values in effect in composite_all.sh (:179-182).  Nothing is read back to the host."""
        from .. import ops
        planes = self._planes(inputs)
        lv = np.stack([_three(min_level, 'min_level'), _three(max_level, 'max_level')], axis=1)
        ty = list(zip(_three_types(min_type, 'min_type'), _three_types(max_type, 'max_type')))
        q = np.zeros((3, 2))
        manual = np.full((3, 2), np.nan, np.float32)
        for c in range(3):
            for t in range(2):
                if ty[c][t] == 'MANUAL':
                    if not np.isfinite(lv[c, t]):
                        raise ValueError('A MANUAL level must be finite.')
                    manual[c, t] = lv[c, t]
                else:
                    q[c, t] = lv[c, t]
        levels, self.n_finite = ops.quantile_levels(planes, q, manual if np.isfinite(manual).any() else None)
        return levels

    # -- composite --------------------------------------------------------------------------------------
    def composite(self, inputs, gamma=2.2, gamma_fac=1.0, colour_sat=1.0, bits=8, flip=True, levels=None, min_level=0.60,
                  max_level=0.999, min_type='QUANTILE', max_type='QUANTILE', gamma_type='POWER-LAW'):
        """RGB images of every (gamma_fac, colour_sat) pair of the grid (variant_grid's order; self.variants lists them): a
        device tensor [V, H, W, 3] of uint8 (bits = 8) or uint16 (bits = 16).  With flip (STIFF's orientation) the first image
        row is the last FITS row.  levels: a [3, 2] tensor from levels(); None: computed with the level arguments."""
        import torch
        from .. import ops
        planes = self._planes(inputs)
        if levels is None:
            levels = self.levels(planes, min_level, max_level, min_type, max_type)
        grid = variant_grid(gamma_fac, colour_sat)
        tables = {gf: ops.tone_table(gamma, gf, gamma_type) for gf in dict.fromkeys(g for g, _ in grid)}
        H, W = int(planes.shape[1]), int(planes.shape[2])
        out = torch.empty((len(grid), H, W, 3), dtype=torch.uint8 if bits == 8 else torch.uint16, device=planes.device)
        for v0 in range(0, len(grid), MAX_VARIANTS):               # one launch per 16 variants
            part = grid[v0:v0 + MAX_VARIANTS]
            ops.composite_rgb(planes, levels, np.stack([tables[g] for g, _ in part]), [s for _, s in part], bits=bits, flip=flip,
                              out=out[v0:v0 + len(part)])
        self.variants = grid
        self._logger.debug(f'Composited {len(grid)} variants of {W} x {H} pixels at {bits} bits.')
        return out

    def composite_files(self, red, green, blue, out_tiffs, gamma=2.2, gamma_fac=1.0, colour_sat=1.0, bits=8, flip=True,
                        min_level=0.60, max_level=0.999, min_type='QUANTILE', max_type='QUANTILE', description='', copyright='',
                        overwrite=True):
        """Reads three FITS images and writes one TIFF per variant: out_tiffs is a file name (one variant) or a list with one
        name per (gamma_fac, colour_sat) pair in variant_grid's order.  Returns the list of files written."""
        names = [out_tiffs] if isinstance(out_tiffs, (str, os.PathLike)) else list(out_tiffs)
        grid = variant_grid(gamma_fac, colour_sat)
        if len(names) != len(grid):
            raise ValueError(f'{len(grid)} variants need {len(grid)} output files, got {len(names)}.')
        planes = self._planes([red, green, blue])
        tiffio.layout(planes.shape[1], planes.shape[2], bits, description, copyright)      # refuses what TIFF cannot hold, early
        out = self.composite(planes, gamma=gamma, gamma_fac=gamma_fac, colour_sat=colour_sat, bits=bits, flip=flip,
                             min_level=min_level, max_level=max_level, min_type=min_type, max_type=max_type)
        pool = fitsio.shared_write_pool()
        try:
            for v, name in enumerate(names):
                tiffio.write_device(str(name), out[v], description=description, copyright=copyright, overwrite=overwrite, pool=pool)
        finally:
            pool.wait()
        for (gf, cs), name in zip(grid, names):
            self._logger.info(f'Wrote {name} (gamma_fac {gf:g}, colour_sat {cs:g}, {bits} bits)')
        return [str(n) for n in names]
