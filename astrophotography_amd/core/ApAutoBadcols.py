"""ApAutoBadcols - host shell over apgpu_axis_nanmedian / apgpu_sliding_clipped_stats (reference:
core/ApAutoBadcols.py).

``ApAutoBadcols(loglevel)``; ``process(data, nsigma=None, window_len=None)`` finds the columns and rows whose median
lies nsigma (default 5.0) or more clipped standard deviations from the sigma-clipped mean of a sliding window of
window_len (default 11) medians around it (:180-258), and returns the 0-based indices ``(badcols, badrows)``, each an
int64 array or None.  ``process_fits(file)`` reads the primary HDU as float32 with the PEDESTAL added (:73-141).
``process_slab(frames)`` is new: one launch sequence for a slab [N, H, W] and a list of per-frame results.
Every number is the reference's, bit for bit (G13).
"""
import numpy as np

from .. import __version__
from . import _common


class ApAutoBadcols:
    """Detects the worst bad columns and rows of an image on the GPU."""

    def __init__(self, loglevel):
        self._name = 'ApAutoBadcols'
        self._version = __version__
        self._loglevel = loglevel
        self._logger = _common.make_logger(self._name, loglevel)

    def process_fits(self, fitsimg, nsigma=None, window_len=None):
        """Bad columns / rows of extension 0 of a FITS file (integers -> float32, PEDESTAL added)."""
        data, _, _ = _common.read_fits(self._logger, fitsimg, to_float32=True)
        return self.process(data, nsigma, window_len)

    def process(self, data_array, nsigma=None, window_len=None):
        """(badcols, badrows) of a 2-D numpy array or CUDA tensor: 0-based int64 indices, or None when there are none."""
        if getattr(data_array, 'ndim', None) != 2:
            raise ValueError('process takes a 2-D image, got shape %s' % (tuple(data_array.shape),))
        return self._run(data_array, nsigma, window_len)[0]

    def process_slab(self, frames, nsigma=None, window_len=None):
        """One call for a slab [N, H, W] (numpy array or CUDA tensor): a list of N (badcols, badrows) pairs."""
        if getattr(frames, 'ndim', None) != 3:
            raise ValueError('process_slab takes a slab [N, H, W], got shape %s' % (tuple(frames.shape),))
        return self._run(frames, nsigma, window_len)

    # -------------------------------------------------------------------------------------------
    @staticmethod
    def _to_device(data):
        import torch
        from .. import ops
        if isinstance(data, torch.Tensor):
            if not data.is_cuda:
                raise ValueError('libapgpu operates on device tensors (got a %s tensor); there is no CPU path' % data.device)
            return data
        a = np.asarray(data)
        if a.dtype == np.uint16:
            return ops.to_device_u16(a)
        if a.dtype == np.uint32:
            a = a.astype(np.int64)
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def _run(self, data, nsigma, window_len):
        from .. import ops
        if nsigma is None:
            nsigma = 5.0        # Want to be sure these are really clearly bad.
        if window_len is None:
            window_len = 11
        d = self._to_device(data)
        r = ops.auto_badcols(d, nsigma=nsigma, window_len=window_len)
        # the only host reads: the per-line arrays
        host = {tag: {k: t.cpu().numpy() for k, t in v.items()} for tag, v in r.items()}
        single = d.dim() == 2
        nframes = 1 if single else d.shape[0]
        out = []
        for f in range(nframes):
            res = []
            for tag, axis in (('cols', 0), ('rows', 1)):
                h = host[tag]
                pick = (lambda a: a) if single else (lambda a, f=f: a[f])
                res.append(self._report(pick(h['median']), pick(h['mean']), pick(h['std']), pick(h['nsig']),
                                        pick(h['flag']).astype(bool), axis))
            out.append(tuple(res))
        return out

    def _report(self, median_array, sldng_mean, sldng_std, nsigma_from_mean, bad_mask, axis_used):
        """The log lines and the return convention of _process (:202-258)."""
        type_str = 'column'
        short_str = 'col'
        if axis_used == 1:
            type_str = 'row'
            short_str = 'row'
        nvals = median_array.size
        nbad = int(np.sum(bad_mask))
        self._logger.info(f'Found {nbad} bad {type_str}s out of {nvals} {type_str}s.')
        if self._logger.isEnabledFor(10):       # logging.DEBUG: the reference's diagnostics table
            nalways = 40
            dbg_str_list = []
            hdr_str = '{:>4s}, {:>10s}, {:>10s}, {:>10s}, {:>10s}, {:>6s}'.format(short_str, 'median', 'local_mean', 'local_std',
                                                                                 'nsigma', 'isbad?')
            dbg_str_list.append(f'Diagnostics for first {nalways} {type_str}s and all bad {type_str}:')
            dbg_str_list.append(hdr_str)
            for idx in range(nvals):
                if (idx < nalways) or (bad_mask[idx]):
                    dbg_str = (f'{idx:04d}, {median_array[idx]:10.2f}, {sldng_mean[idx]:10.2f}, {sldng_std[idx]:10.2f}, '
                               f'{nsigma_from_mean[idx]:10.2f}, {bad_mask[idx]}')
                    dbg_str_list.append(dbg_str)
            self._logger.debug('\n'.join(dbg_str_list))
        if nbad > 0:
            return np.arange(nvals)[bad_mask]
        return None
