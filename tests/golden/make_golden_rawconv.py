#!/opt/conda/bin/python3.9 -B
"""Golden group G18: the white balance RawConv takes from the image (core/RawConv.py:291-366), computed by the reference class.

RUN ONLY IN THE BUILD CONTAINER:   /opt/conda/bin/python3.9 -B tests/golden/make_golden_rawconv.py

RawConv imports rawpy and exifread (neither present, neither used here): both get stub modules.  A RawConv object is made with
__new__ (its __init__ reads a RAW file) and given what _build_raw_channel_images would have set from a synthetic RGGB mosaic:
_rawim_*, _mask_*, _nrows, _ncols.  With a black level the class's own _subtract_black_levels runs first.  get_whitebalance is
recorded for 'auto' and two 'region[...]' strings as float64.  The fixture holds the mosaics, the black levels, the region lists
and the results, nothing else.
"""
import logging
import os
import sys
import types

import numpy as np


class _Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith('__'):
            raise AttributeError(k)
        return _Stub(self.__name__ + '.' + k)


for m in ['rawpy', 'exifread', 'exif', 'matplotlib', 'matplotlib.pyplot', 'yaml']:
    try:
        __import__(m)
    except Exception:
        sys.modules[m] = _Stub(m)

HERE = os.path.dirname(os.path.abspath(__file__))
logging.disable(logging.CRITICAL)

# RawConv.py does `from .logger import logger` and `from .. import __version__`: two bare parent packages stand in for the
# reference's own (importing those would pull in every other class and its dependencies).
import importlib.util
_top = types.ModuleType('AstroPhotography')
_top.__path__, _top.__version__ = [], '0.5.1'
_core = types.ModuleType('AstroPhotography.core')
_core.__path__ = []
_log = types.ModuleType('AstroPhotography.core.logger')
_log.logger = logging.getLogger('AstroPhotography')
sys.modules.update({'AstroPhotography': _top, 'AstroPhotography.core': _core, 'AstroPhotography.core.logger': _log})
_spec = importlib.util.spec_from_file_location('AstroPhotography.core.RawConv', '/root/reference/AstroPhotography/core/RawConv.py')
_mod = importlib.util.module_from_spec(_spec)
sys.modules['AstroPhotography.core.RawConv'] = _mod
_spec.loader.exec_module(_mod)
RawConv = _mod.RawConv

PATTERN = (0, 1, 3, 2)          # RGGB: the colour of cell position (r & 1) 2 + (c & 1)


def mosaic(shape, seed):
    rng = np.random.default_rng(seed)
    r, c = np.indices(shape)
    k = np.asarray(PATTERN)[(r & 1) * 2 + (c & 1)]
    level = np.array([900.0, 2100.0, 1400.0, 2050.0])[k]           # a sky with a colour cast; some samples fall below black 256
    m = rng.poisson(level * (0.1 + 0.9 * rng.random(shape))).astype(np.float64) + 200.0 * rng.random(shape)
    return np.clip(m, 0, 65535).astype(np.uint16)


def reference_gains(m, black, wb_method):
    r, c = np.indices(m.shape)
    cmap = np.asarray(PATTERN)[(r & 1) * 2 + (c & 1)]
    rc = RawConv.__new__(RawConv)
    rc._rawpy = None                                        # (read by __del__)
    rc.R, rc.G1, rc.B, rc.G2 = 0, 1, 2, 3
    rc._nrows, rc._ncols = m.shape
    for name, k in (('r', 0), ('g1', 1), ('b', 2), ('g2', 3)):
        mask = cmap == k
        setattr(rc, '_mask_' + name, mask)
        setattr(rc, '_rawim_' + name, np.where(mask, m, 0))
    rc._black_levels = [black] * 4
    rc._black_subtracted = False
    if black:
        rc._subtract_black_levels()
    return np.array([float(v) for v in rc.get_whitebalance(wb_method)], np.float64)


def main():
    out = {'pattern': np.array(PATTERN, np.int32)}
    cases = []
    for tag, shape, seed, regions in (('a', (14, 14), 11, [[2, 9, 3, 12], [5, 6, 0, 13]]),
                                      ('b', (48, 64), 12, [[7, 40, 10, 33], [30, 200, 41, 63]])):
        m = mosaic(shape, seed)
        out['mosaic_' + tag] = m
        for black in (0, 256):
            for i, reg in enumerate([None] + regions):
                wb = 'auto' if reg is None else 'region' + str(reg)
                name = '%s_b%d_%d' % (tag, black, i)
                out['gains_' + name] = reference_gains(m, black, wb)
                out['region_' + name] = np.array([-1] * 4 if reg is None else reg, np.int64)
                out['black_' + name] = np.array([black] * 4, np.int32)
                cases.append(name)
    out['cases'] = np.array(cases)
    np.savez_compressed(os.path.join(HERE, 'g18_whitebalance.npz'), **out)
    for name in cases:
        print(name, out['gains_' + name])


if __name__ == '__main__':
    main()
