"""ApRegister - relative registration of frames from their star lists (new: the reference obtains its geometry from
astrometry.net through ApAstrometry, a network service that is out of scope here).

The frames' brightness-ordered source lists (ApFindStars) are matched with the list of a reference frame by triangle
similarity (Groth 1986; Valdes et al. 1995) and one affine per frame is fitted - with model 'poly2' .. 'poly5' also a polynomial
distortion map on top of it (DESIGN 4.3e': camera lenses, short refractors, two telescopes) -, in the convention ApResample.coadd,
ops.resample_affine and ``ap_coadd --transforms`` use: ``x_frame = a0 x + a1 y + a2, y_frame = a3 x + a4 y + a5`` for (x, y)
on the reference frame's grid, 0-based, integer = pixel centre.  The rule is DESIGN 4.3e; the triangle and neighbour searches
are HIP kernels (csrc/register.hip), the fits a few float64 NumPy lines (ops.register_lists).

  device  triangles of the K brightest stars -> votes for star pairs -> nearest neighbours under the current transform
  host    seeds from the votes, the least-squares fits, the YAML file
"""
import math
import os

import numpy as np

from .. import fitsio
from . import _common

MAX_STARS = 4096


class ApRegister:
    """Register frames on a reference frame from their star lists."""

    def __init__(self, loglevel='INFO', K=40, eps=0.002, match_radius=3.0, model='affine', allow_mirror=False, min_side=5.0):
        if model not in ('affine', 'similarity', 'poly2', 'poly3', 'poly4', 'poly5'):
            raise ValueError(f"model must be 'affine', 'similarity' or 'poly2' .. 'poly5', got {model!r}.")
        self._loglevel = loglevel
        self._K = int(K)
        self._eps = float(eps)
        self._match_radius = float(match_radius)
        self._model = model
        self._allow_mirror = bool(allow_mirror)
        self._min_side = float(min_side)
        self._logger = _common.make_logger('ApRegister', loglevel)
        self._names = None
        self._result = None

    # -- input ------------------------------------------------------------------------------------------
    @staticmethod
    def _positions(src):
        """[n, 2] float64 (x, y) of an ApFindStars object, a table with xcenter / ycenter, or an [n, 2] array."""
        table = getattr(src, '_phot_table', src)
        if isinstance(table, dict):
            return np.stack([np.asarray(table['xcenter'], np.float64), np.asarray(table['ycenter'], np.float64)], axis=1)
        return np.asarray(table, np.float64).reshape(-1, 2)

    def register_lists(self, lists, names=None):
        """Registers lists[1:] on lists[0].  A list is an ApFindStars object, a photometry table (dict with xcenter and
        ycenter) or an [n, 2] array of (x, y), brightest star first.  Returns the result of ops.register_lists."""
        from .. import ops
        pos = [self._positions(s) for s in lists]
        if not pos:
            raise ValueError('No star list given.')
        for f, p in enumerate(pos):
            if len(p) > MAX_STARS:
                self._logger.warning(f'List {f} holds {len(p)} stars: the brightest {MAX_STARS} are used.')
        pos = [p[:MAX_STARS] for p in pos]
        M = max(1, max(len(p) for p in pos))
        xy = np.zeros((len(pos), M, 2))
        for f, p in enumerate(pos):
            xy[f, :len(p)] = p
        count = np.array([len(p) for p in pos], np.int32)
        self._names = [str(n) for n in names] if names is not None else ['frame-%04d' % f for f in range(len(pos))]
        if len(self._names) != len(pos):
            raise ValueError('names must hold one entry per list.')
        self._result = ops.register_lists(xy, count, K=self._K, eps=self._eps, min_side=self._min_side,
                                          match_radius=self._match_radius, model=self._model, allow_mirror=self._allow_mirror)
        for f, name in enumerate(self._names):
            q = self.quality(f)
            if q['ok']:
                self._logger.info('{}: {} seeds, {} matched, rms {:.3f} pix, rotation {:.4f} deg, scale {:.6f}, shift ({:.3f}, {:.3f})'
                                  .format(name, q['n_seed'], q['n_matched'], q['rms'], q['rotation_deg'], q['scale'], q['shift_x'],
                                          q['shift_y']))
                if 'order' in q:
                    self._logger.info('{}: polynomial of order {}, rms {:.3f} pix after {:.3f} pix of the affine'
                                      .format(name, q['order'], q['rms'], q['rms_affine']))
            else:
                self._logger.warning(f'{name}: not registered ({q["n_seed"]} seeds, {q["n_matched"]} matched).')
        return self._result

    def register_source_lists(self, files):
        """The same for source-list files written by ApFindStars.write_source_list (extension AP_L1MAG, xcenter / ycenter).
        A frame is named after the image in its list's IMG_FILE card, or after the list file if there is none."""
        lists, names = [], []
        for path in files:
            _common.check_file_exists(self._logger, path)
            cols, _, prim = fitsio.read_table(str(path), 'AP_L1MAG')
            lists.append({'xcenter': cols['xcenter'], 'ycenter': cols['ycenter']})
            names.append(os.path.basename(str(prim['IMG_FILE']).strip()) if 'IMG_FILE' in prim else os.path.basename(str(path)))
        return self.register_lists(lists, names)

    def register_images(self, files_or_tensors, search_fwhm=3.0, search_nsigma=7.0, max_sources=None, names=None):
        """Runs ApFindStars on every image (a FITS file name, or a 2-D CUDA tensor) and registers the source lists."""
        from .ApFindStars import ApFindStars
        lists, auto = [], []
        for f, img in enumerate(files_or_tensors):
            if isinstance(img, (str, os.PathLike)):
                fs = ApFindStars(str(img), 0, search_fwhm, search_nsigma, 16, max_sources, False, 0.80, self._loglevel, None, True)
                auto.append(os.path.basename(str(img)))
            else:
                fs = ApFindStars.from_device(img, search_fwhm=search_fwhm, search_nsigma=search_nsigma, max_sources=max_sources,
                                             loglevel=self._loglevel)
                auto.append('frame-%04d' % f)
            lists.append(fs)
        return self.register_lists(lists, names if names is not None else auto)

    # -- output -----------------------------------------------------------------------------------------
    def _need_result(self):
        if self._result is None:
            raise RuntimeError('Nothing has been registered yet.')
        return self._result

    def quality(self, f):
        """ok, seeds, matches, rms and the rotation / scale / shift the transform of frame f amounts to."""
        r = self._need_result()
        q = {'ok': bool(r['ok'][f]), 'n_seed': int(r['n_seed'][f]), 'n_matched': int(r['n_matched'][f])}
        if q['ok']:
            a = r['coeffs'][f]
            q.update(rms=float(r['rms'][f]), rotation_deg=math.degrees(math.atan2(a[3] - a[1], a[0] + a[4])),
                     scale=math.sqrt(abs(a[0] * a[4] - a[1] * a[3])), shift_x=float(a[2]), shift_y=float(a[5]))
            if 'order' in r:
                q.update(order=int(r['order'][f]), rms_affine=float(r['rms_affine'][f]))
        return q

    def _failed(self):
        r = self._need_result()
        return [n for n, ok in zip(self._names, r['ok']) if not ok]

    def affines(self, skip_failed=False):
        """The transforms as ApResample.coadd takes them: one list of 6 coefficients per frame, in input order.  A frame that
        was not registered is an error, or left out with skip_failed."""
        r = self._need_result()
        if self._failed() and not skip_failed:
            raise RuntimeError('Not registered: ' + ', '.join(self._failed()))
        return [[float(v) for v in r['coeffs'][f]] for f in range(len(self._names)) if r['ok'][f]]

    def maps(self, skip_failed=False):
        """The distortion maps (distortion.PolyMap, one degree, origin and scale) of the frames `affines` lists, in that order, with
        a polynomial model; None with 'affine' or 'similarity'."""
        r = self._need_result()
        if self._failed() and not skip_failed:
            raise RuntimeError('Not registered: ' + ', '.join(self._failed()))
        return [m for m, ok in zip(r['maps'], r['ok']) if ok] if 'maps' in r else None

    def names(self, skip_failed=False):
        r = self._need_result()
        return [n for n, ok in zip(self._names, r['ok']) if ok or not skip_failed]

    def write_transforms(self, path, skip_failed=False):
        """Writes the YAML file ``ap_coadd --transforms`` reads: ``transforms:`` frame name -> 6 coefficients, plus
        ``quality:`` frame name -> quality(f) (ap_coadd ignores it).  With a polynomial model also ``distortion:`` {origin, scale,
        frames: frame name -> {order, x, y}} (distortion.to_document), which ap_coadd and ap_drizzle use in place of the affine."""
        import yaml
        r = self._need_result()
        if self._failed() and not skip_failed:
            raise RuntimeError('Not registered: ' + ', '.join(self._failed()))
        for n in self._failed():
            self._logger.warning(f'{n}: not registered, left out of {path}.')
        if len(set(self._names)) != len(self._names):
            raise RuntimeError('Two frames share a name: the transforms file is keyed by name.')
        doc = {'transforms': {n: [float(v) for v in r['coeffs'][f]] for f, n in enumerate(self._names) if r['ok'][f]},
               'quality': {n: self.quality(f) for f, n in enumerate(self._names)}}
        if 'maps' in r:
            from ..distortion import to_document
            doc['distortion'] = to_document(r['maps'], r['order'], self._names)
        with open(path, 'w') as fh:
            yaml.safe_dump(doc, fh, sort_keys=False)
        self._logger.info(f'Wrote the transforms of {len(doc["transforms"])} frames to {path}')
