"""ApDrizzle - drizzle co-add of dithered frames onto a finer grid (variable-pixel linear reconstruction, Fruchter & Hook 2002).

The reference has no such stage, so it is defined by this project (restated in tests/drizzle_model.py).  Where ap_coadd
interpolates every frame (right for well-sampled data), drizzle shrinks each input pixel to a drop of `pixfrac` times its size, lays
it on a grid of `scale` output pixels per input pixel and averages it in with the overlap area as its weight: the sub-pixel dithers
that ap_register measures become resolution, a bad pixel costs its own drop only, and the weight map is the true coverage.  With
cfa=True only the pixels of colour c feed plane c of a one-shot-colour mosaic - no demosaic at all.

  device  the drizzle itself, one launch for all frames (csrc/drizzle.hip); the blot-and-compare flags; the frame noise behind the
          weights (the clipped standard deviation of ops.background_weights); the median reference (ops.coadd); FITS decode
  host    the transforms' composition, weights, headers

Header cards: NCOMBINE, TEXPTIME, IFILEnnn, BUNIT, HISTORY as ApResample; COMBINET = 'DRIZZLE'; DRIZSCAL (output pixels per input
pixel), DRIZPIXF (pixfrac), DRIZKERN = 'TURBO', DRIZNREJ (pixels flagged by the rejection, all frames).

Rejection in CFA mode is refused (ValueError): its reference would have to be built per colour from a quarter of the pixels; flag the
mosaics beforehand (ap_fix_cosmic_rays) or pass frame masks to drizzle().

Lens distortion (DESIGN 4.3e'): with `maps` (one distortion.PolyMap per frame, what ap_register --model polyN writes) the drizzle,
the median reference and the rejection take one transform per 16 x 64 tile - of the output, of the scale-1 grid and of the input
frame - instead of one per frame; footprint, weight and flux factor are then each tile's own.

Out of scope: the exact polygon ("square") kernel and the point, Gaussian and Lanczos drop kernels; TAN-WCS registration; per-pixel
input weight maps; a second rejection pass with tighter thresholds; multi-GPU sharding.
"""
from datetime import datetime, timezone
from pathlib import Path

import numpy as np

from .. import __version__, fitsio
from . import _common

WEIGHTINGS = ('background', 'none')
CARDS = ('NCOMBINE', 'COMBINET', 'DRIZSCAL', 'DRIZPIXF', 'DRIZKERN', 'DRIZNREJ', 'TEXPTIME')


class ApDrizzle:
    """Drizzle co-add of registered, dithered frames (device tensors or FITS files)."""

    CARDS = CARDS

    def __init__(self, loglevel='INFO', scale=2.0, pixfrac=0.5, reject=False, k=3.5, grow=1.2, weighting='background', conserve_flux=False,
                 gain_keyword='EGAIN'):
        """scale: output pixels per input pixel.  pixfrac: side of a drop in input pixels, (0, 1].  reject: flag outliers against a
        median co-add first (k, grow: a pixel is flagged when it is more than k sigma_i + grow d from the reference under it, d being
        the reference's local spread).  weighting: 'background' (inverse variance of the flux-scaled background noise, as ap_coadd's
        WEIGHTED) or 'none'.  conserve_flux: scale by the pixel-area ratio (totals kept) instead of keeping surface brightness."""
        import math
        self._name = 'ApDrizzle'
        self._logger = _common.make_logger(self._name, loglevel)
        self.scale, self.pixfrac = float(scale), float(pixfrac)
        if not (math.isfinite(self.scale) and self.scale > 0.0):
            raise ValueError(f'scale must be a positive number, got {scale!r}')
        if not 0.0 < self.pixfrac <= 1.0:
            raise ValueError(f'pixfrac must be in (0, 1], got {pixfrac!r}')
        self.reject, self.k, self.grow = bool(reject), float(k), float(grow)
        if not (math.isfinite(self.k) and math.isfinite(self.grow) and self.k >= 0.0 and self.grow >= 0.0):
            raise ValueError(f'k and grow must be finite and >= 0, got {k!r} and {grow!r}')
        if weighting not in WEIGHTINGS:
            raise ValueError(f'Unexpected weighting {weighting!r}. Allowed values are: {list(WEIGHTINGS)}')
        self.weighting = weighting
        self.conserve_flux = bool(conserve_flux)
        self.gain_keyword = gain_keyword

    # -- tensors -----------------------------------------------------------------------------------------
    def drizzle(self, frames, affines, fscale=None, weights=None, mask=None, frame_masks=None, out_shape=None, cfa=None, sigmas=None,
                maps=None, max_tile_error=0.01):
        """frames [N,H,W] float32 device tensor, affines one 2x3 transform per frame (reference pixel -> input pixel).  weights: None
        takes the constructor's weighting.  cfa: None or (pattern, channel).  With reject (not with cfa) the frames are first compared
        with their own median co-add on the scale-1 grid and the flags are added to frame_masks; sigmas: the frames' noise in
        flux-scaled units (None: measured).  maps: one distortion.PolyMap per frame, used in place of `affines` through per-tile
        transforms (ValueError when a tile's linearisation would cost more than max_tile_error input pixels).

        Returns dict(image, weight, rejected): rejected = flagged pixels per frame (numpy int64 [N]) or None."""
        import torch
        from .. import ops
        if frames.dim() == 2:
            frames = frames[None]
        N = frames.shape[0]
        in_shape = tuple(frames.shape[1:])
        co_affines = rej_affines = affines                               # what the median reference and the rejection take
        if maps is not None:
            maps = list(maps)
            if len(maps) != N:
                raise ValueError(f'{len(maps)} distortion maps given for {N} frames.')
            shape = ops.drizzle_out_shape(in_shape, self.scale) if out_shape is None else out_shape
            affines, est = ops.poly_tile_affines(maps, shape, scale=self.scale, max_tile_error=max_tile_error, composed=False,
                                                 device=frames.device)
            self._logger.info(f'Distortion maps of degree {maps[0].degree}: one transform per 16 x 64 output tile, linearisation error at '
                              f'most {est:.2e} input pixels.')
            if self.reject:
                co_affines, _ = ops.poly_tile_affines(maps, in_shape, max_tile_error=max_tile_error, device=frames.device)
                rej_affines = ops.poly_input_tile_affines(maps, in_shape)
        fs = np.ones(N) if fscale is None else np.broadcast_to(np.asarray(fscale, np.float64).reshape(-1), (N,))
        sd = None
        if weights is None and self.weighting == 'background' or self.reject and sigmas is None:
            sd = np.sqrt(1.0 / ops.background_weights(frames, fs))      # fscale_i x the clipped standard deviation of frame i
        if weights is None and self.weighting == 'background':
            weights = 1.0 / sd ** 2
        rejected = None
        if self.reject:
            if cfa is not None:
                raise ValueError('Rejection is not available in CFA mode: flag the mosaics beforehand or pass frame_masks.')
            ref = ops.coadd(frames, co_affines, fscale=fs.astype(np.float32), mask=mask, out_shape=in_shape, combine='MEDIAN', conserve_flux=False)
            flags = ops.drizzle_reject(frames, rej_affines, ref['image'], 1.0, fscale=fs, sigmas=sd if sigmas is None else sigmas, k=self.k,
                                       grow=self.grow)
            rejected = flags.reshape(N, -1).sum(1, dtype=torch.int64).cpu().numpy()
            for i, n in enumerate(rejected):
                self._logger.info(f'  Frame {i:3d}: {int(n)} pixels flagged against the median co-add (k {self.k:g}, grow {self.grow:g})')
            if frame_masks is not None:
                flags |= (frame_masks != 0).to(torch.uint8)
            frame_masks = flags
        res = ops.drizzle(frames, affines, scale=self.scale, pixfrac=self.pixfrac, fscale=fs, weights=weights, mask=mask,
                          frame_masks=frame_masks, out_shape=out_shape, conserve_flux=self.conserve_flux, cfa=cfa)
        res['rejected'] = rejected
        return res

    # -- files ---------------------------------------------------------------------------------------------
    def _exposure(self, hdr, fname):
        for kw in ('EXPOSURE', 'EXPTIME'):
            if kw in hdr:
                return float(hdr[kw])
        raise RuntimeError(f'Error, could not find EXPOSURE keyword in {fname}.')

    def drizzle_files(self, input_files, affines, output_file, weight_file=None, mask_file=None, cfa=False, pattern=None, out_shape=None,
                      maps=None, max_tile_error=0.01):
        """Drizzles FITS files.  affines: one [a00, a01, a02, a10, a11, a12] per file (what ap_register writes).  Flux scale per
        file = 1 / EXPOSURE (or EXPTIME).  cfa: the files are Bayer mosaics; the pattern is `pattern` (RGGB, BGGR, GRBG, GBRG or four
        colour indices) or the first file's BAYERPAT shifted by XBAYROFF / YBAYROFF, and three files OUT_r.fits, OUT_g.fits, OUT_b.fits
        are written (OUT = output_file without .fits), with weight maps W_r/_g/_b.fits when weight_file = W.fits is given.  maps: as
        drizzle takes them.
        Returns the result of drizzle() (cfa: a list of three)."""
        import torch
        from .ApStack import _apply_pedestals
        input_files = [str(f) for f in input_files]
        if not input_files:
            raise RuntimeError('No input files to drizzle.')
        affines = np.asarray(affines, dtype=np.float64).reshape(-1, 6)
        if len(affines) != len(input_files):
            raise RuntimeError(f'Error, {len(affines)} transforms given for {len(input_files)} files.')
        if cfa and self.reject:
            raise ValueError('Rejection is not available in CFA mode: flag the mosaics beforehand.')
        for f in input_files:
            _common.check_file_exists(self._logger, f)
        slab, hdrs = fitsio.read_slab_device(input_files, dtype=torch.float32)
        slab = _apply_pedestals(slab, hdrs)
        fscale, texp = [], 0.0
        for f, hdr in zip(input_files, hdrs):
            exp = self._exposure(hdr, f)
            texp += exp
            fscale.append(1.0 / exp)
            self._logger.info(f'  File {Path(f).name:40s} EXPOSURE {exp:8.3f} FSCALE {fscale[-1]:8.6f}')
        in_shape = tuple(slab.shape[1:])
        mask = None
        if mask_file is not None:
            m, _, _ = _common.read_fits(self._logger, mask_file)
            if m.shape != in_shape:
                raise RuntimeError(f'Error, mask shape {m.shape} differs from the image shape {in_shape}.')
            mask = torch.from_numpy((np.asarray(m) != 0).astype(np.uint8)).cuda()
        pat = None
        if cfa:
            from .ApDebayer import ApDebayer
            pat = ApDebayer._pattern_from(None, hdrs[0], pattern)
        outputs = [(None, str(output_file), None if weight_file is None else str(weight_file))]
        if cfa:
            root = str(output_file)[:-5] if str(output_file).lower().endswith('.fits') else str(output_file)
            wroot = None if weight_file is None else (str(weight_file)[:-5] if str(weight_file).lower().endswith('.fits') else str(weight_file))
            outputs = [(c, f'{root}_{n}.fits', None if wroot is None else f'{wroot}_{n}.fits') for c, n in enumerate('rgb')]
        results = []
        for channel, out_name, w_name in outputs:
            res = self.drizzle(slab, affines, fscale=np.asarray(fscale), mask=mask, out_shape=out_shape,
                               cfa=None if channel is None else (pat, channel), maps=maps, max_tile_error=max_tile_error)
            results.append(res)
            nrej = 0 if res['rejected'] is None else int(res['rejected'].sum())
            hdr = hdrs[0].copy()
            for kw in ('BSCALE', 'BZERO', 'PEDESTAL') + (('BAYERPAT', 'XBAYROFF', 'YBAYROFF') if cfa else ()):
                if kw in hdr:
                    del hdr[kw]
            hdr['NCOMBINE'] = (len(input_files), 'Number of frames combined')
            hdr['COMBINET'] = ('DRIZZLE', 'Co-add combine type')
            hdr['DRIZSCAL'] = (self.scale, 'Output pixels per input pixel and axis')
            hdr['DRIZPIXF'] = (self.pixfrac, 'Side of a drop in input pixels (pixfrac)')
            hdr['DRIZKERN'] = ('TURBO', 'Drizzle kernel')
            hdr['DRIZNREJ'] = (nrej, 'Input pixels flagged by the rejection')
            if channel is not None:
                hdr['DRIZCHAN'] = ('RGB'[channel], 'Colour of the CFA pixels drizzled')
            hdr['TEXPTIME'] = (texp, '[s] Total exposure of the inputs')
            hdr['BUNIT'] = ('adu/s', 'Pixel value units (flux scaled by 1/EXPOSURE)')
            for idx, fname in enumerate(input_files):
                hdr[f'IFILE{idx:03d}'] = Path(fname).name
            tnow = datetime.now().isoformat(timespec='milliseconds')
            hdr['DATE'] = (datetime.now(timezone.utc).isoformat(timespec='seconds'), 'Date/time file was created.')
            hdr['HISTORY'] = f'Processed by {self._name} {__version__} at {tnow}'
            hdr['HISTORY'] = (f'ApDrizzle: scale {self.scale:g}, pixfrac {self.pixfrac:g}, turbo kernel, weighting {self.weighting}, '
                              f'{"rejection k %g grow %g" % (self.k, self.grow) if self.reject else "no rejection"}')
            fitsio.write(out_name, res['image'].cpu().numpy(), hdr, overwrite=True)
            self._logger.info(f'Wrote drizzled image to {out_name}')
            if w_name is not None:
                wh = fitsio.Header()
                wh['NCOMBINE'] = (len(input_files), 'Number of frames combined')
                wh['HISTORY'] = f'Weight map (sum of weight x drop cover per pixel) by {self._name} {__version__} at {tnow}'
                fitsio.write(w_name, res['weight'].cpu().numpy(), wh, overwrite=True)
                self._logger.info(f'Wrote weight image to {w_name}')
        return results if cfa else results[0]
