"""Array-level entry points: torch tensors in HBM -> libapgpu.so kernels (include/apgpu.h).

These are the slab/array forms underneath the file-based Ap* classes (the reference has no in-memory
API for this path: "TODO: Allow calibration of images in memory", core/ApCalibrate.py:3).  PyTorch
only owns device memory and streams here; every computation is a hand-written HIP kernel.  All calls are
asynchronous on the current torch stream.
"""
import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import APGPU_F32, APGPU_F64, APGPU_U16, StackArgs, check
from .fitsio import widen_u16


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _aligned16(t):
    """A contiguous tensor whose storage starts on a 16-byte boundary (the vectorised kernels require it): a frame cut out
    of a slab with an odd pixel count is copied once."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError('libapgpu operates on device tensors (got a %s tensor); there is no CPU path' % t.device)


def _f32c(t, name):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError('%s must be float32, got %s' % (name, t.dtype))
    return t.contiguous()


def _image_f32(data, name='data'):
    """A non-empty 2-D float32 device image, contiguous."""
    _need_cuda(data)
    data = _f32c(data, name)
    if data.dim() != 2 or data.numel() == 0:
        raise ValueError('%s must be a non-empty 2-D image, got shape %s' % (name, tuple(data.shape)))
    return data


def _plane_like(t, name, like):
    """... of the shape of `like`."""
    t = _image_f32(t, name)
    if tuple(t.shape) != tuple(like.shape):
        raise ValueError('%s must have the image shape %s, got %s' % (name, tuple(like.shape), tuple(t.shape)))
    return t


def _out_f32(out, like, *distinct, shape=None, name='out'):
    """An output argument: None (a new tensor of `shape`, that of `like` unless given), or a contiguous float32 device tensor of
    that shape that is none of `distinct`."""
    if out is None:
        return torch.empty_like(like) if shape is None else torch.empty(shape, dtype=torch.float32, device=like.device)
    shape = tuple(like.shape if shape is None else shape)
    _need_cuda(out)
    if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or \
            any(out.data_ptr() == t.data_ptr() for t in distinct):
        raise ValueError('%s must be a contiguous float32 device tensor of shape %s%s' % (name, shape, ', distinct from the input planes' if distinct else ''))
    return out


def _workspace(ws, need, device, maker):
    """A workspace argument: None (a new one), or a contiguous, 16-byte aligned uint8 device tensor of at least `need` bytes."""
    if ws is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    _need_cuda(ws)
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need or ws.data_ptr() % 16:
        raise ValueError('ws must be a contiguous, 16-byte aligned uint8 device tensor of at least %d bytes (ops.%s)' % (need, maker))
    return ws


def _mask_u8(mask, shape, message, error=ValueError):
    """A mask argument: None, or a device tensor of `shape` as contiguous uint8 (another dtype: != 0)."""
    if mask is None:
        return None
    _need_cuda(mask)
    if tuple(mask.shape) != tuple(shape):
        raise error(message)
    return (mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)).contiguous()


def _raw_dtype(t):
    if t.dtype == torch.float32:
        return APGPU_F32
    if t.dtype in (torch.uint16, torch.int16):          # int16 storage is reinterpreted as uint16
        return APGPU_U16
    raise TypeError('frame data must be float32 or uint16, got %s' % t.dtype)


def to_device_u16(a, device='cuda'):
    """numpy uint16 array -> device tensor with dtype torch.uint16."""
    a = np.ascontiguousarray(a, dtype=np.uint16)
    return torch.from_numpy(a.view(np.int16)).to(device).view(torch.uint16)


def _per_frame(x, n, device):
    """python float / sequence / tensor -> float32 device tensor [n] (float32 cast like numpy's weak scalar)."""
    if x is None:
        return None
    if torch.is_tensor(x):
        t = x.to(device=device, dtype=torch.float32).reshape(-1)
        if t.numel() == 1 and n > 1:
            t = t.expand(n)
        return t.contiguous()
    a = np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---------------------------------------------------------------------------------------------------
def _dtype_tag(t, what, allow_u16=False):
    if t.dtype == torch.float32:
        return APGPU_F32
    if t.dtype == torch.float64:
        return APGPU_F64
    if allow_u16 and t.dtype in (torch.uint16, torch.int16):
        return APGPU_U16
    raise TypeError('%s must be float32 or float64%s, got %s' % (what, ' or uint16' if allow_u16 else '', t.dtype))


def flat_normalize(flat):
    """A1 ApCalibrate._generate_flat (ApCalibrate.py:166-190): returns (nflat, norm[1] device tensor), both in the
    flat's own dtype - float32, or float64 for a float64 master (the reference keeps float FITS data as stored,
    ApCalibrate.py:301-305).  A flat that does not start on a 16-byte boundary is copied once (the kernels take aligned planes)."""
    _need_cuda(flat)
    lib = _lib.load()
    if flat.dtype == torch.float64:
        flat = _aligned16(flat)                             # both forms take a 16-byte aligned plane
        n = flat.numel()
        ws_bytes = lib.apgpu_flat_normalize_f64_ws_bytes(n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=flat.device)
        nflat = torch.empty_like(flat)
        norm = torch.empty(1, dtype=torch.float64, device=flat.device)
        check(lib.apgpu_flat_normalize_f64(_ptr(flat), _ptr(nflat), _ptr(norm), n, _ptr(ws), ws_bytes, _stream()))
        return nflat, norm
    flat = _aligned16(_f32c(flat, 'flat'))
    n = flat.numel()
    ws_bytes = lib.apgpu_flat_normalize_ws_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=flat.device)
    nflat = torch.empty_like(flat)
    norm = torch.empty(1, dtype=torch.float32, device=flat.device)
    check(lib.apgpu_flat_normalize_f32(_ptr(flat), _ptr(nflat), _ptr(norm), n, _ptr(ws), ws_bytes, _stream()))
    return nflat, norm


def calibrate(raw, bias, dark, nflat, exp_ratio, pedestal=None, dark_still_biased=False, out=None):
    """A2 ApCalibrate.calibrate arithmetic (ApCalibrate.py:439-464) on raw[H,W] or a slab raw[N,H,W].

    The float32 kernel takes 16-byte aligned planes: raw, bias, dark and nflat are copied once when they are not (a frame cut out of
    a slab with an odd pixel count); the results are the same bits.  out, when given, must itself start on a 16-byte boundary
    (every torch allocation does): the library refuses any other."""
    _need_cuda(raw, bias, dark, nflat)
    lib = _lib.load()
    raw = raw.contiguous()
    if any(t is not None and t.dtype == torch.float64 for t in (raw, bias, dark, nflat)):
        return _calibrate_mixed(raw, bias, dark, nflat, exp_ratio, pedestal, dark_still_biased, out)
    dt = _raw_dtype(raw)
    raw = _aligned16(raw)                                   # apgpu_calibrate takes 16-byte aligned planes
    single = raw.dim() == 2
    N = 1 if single else raw.shape[0]
    P = raw[0].numel() if not single else raw.numel()
    bias, dark, nflat = (None if t is None else _aligned16(t) for t in (_f32c(bias, 'bias'), _f32c(dark, 'dark'), _f32c(nflat, 'nflat')))
    for nm, t in (('bias', bias), ('dark', dark), ('nflat', nflat)):
        if t is not None and t.numel() != P:
            raise RuntimeError('%s has %d pixels, frames have %d' % (nm, t.numel(), P))
    e = _per_frame(exp_ratio, N, raw.device)
    ped = _per_frame(pedestal, N, raw.device)
    if out is None:
        out = torch.empty(raw.shape, dtype=torch.float32, device=raw.device)
    check(lib.apgpu_calibrate(_ptr(raw), dt, _ptr(bias), _ptr(dark), _ptr(nflat), _ptr(e), _ptr(ped),
                              int(bool(dark_still_biased)), _ptr(out), N, P, _stream()))
    return out


def _per_frame_f64(x, n, device):
    if x is None:
        return None
    if torch.is_tensor(x):
        t = x.to(device=device, dtype=torch.float64).reshape(-1)
        return (t.expand(n) if t.numel() == 1 and n > 1 else t).contiguous()
    return torch.from_numpy(np.array(np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)))).to(device)


def _calibrate_mixed(raw, bias, dark, nflat, exp_ratio, pedestal, dark_still_biased, out):
    """A2 with float64 inputs (apgpu_calibrate_mixed): NumPy's per-operation promotion; the result is float64 if any
    participating array is float64."""
    lib = _lib.load()
    single = raw.dim() == 2
    N = 1 if single else raw.shape[0]
    P = raw.numel() // N
    rt = _dtype_tag(raw, 'raw', allow_u16=True)
    bias, dark = bias.contiguous(), dark.contiguous()
    nflat = None if nflat is None else nflat.contiguous()
    bt, dk = _dtype_tag(bias, 'bias'), _dtype_tag(dark, 'dark')
    nt = _dtype_tag(nflat, 'nflat') if nflat is not None else APGPU_F32
    for nm, t in (('bias', bias), ('dark', dark), ('nflat', nflat)):
        if t is not None and t.numel() != P:
            raise RuntimeError('%s has %d pixels, frames have %d' % (nm, t.numel(), P))
    r64, b64, d64 = rt == APGPU_F64, bt == APGPU_F64, dk == APGPU_F64
    t3 = (r64 or b64) or ((d64 or b64) if dark_still_biased else d64)
    t4 = (t3 or nt == APGPU_F64) if nflat is not None else t3
    odt = torch.float64 if t4 else torch.float32
    e = _per_frame_f64(exp_ratio, N, raw.device)
    ped = _per_frame_f64(pedestal, N, raw.device)
    if out is None:
        out = torch.empty(raw.shape, dtype=odt, device=raw.device)
    elif out.dtype != odt or out.shape != raw.shape or not out.is_contiguous():
        raise TypeError('out must be a contiguous %s tensor of the raw shape' % odt)
    check(lib.apgpu_calibrate_mixed(_ptr(raw), rt, _ptr(bias), bt, _ptr(dark), dk, _ptr(nflat), nt, _ptr(e), _ptr(ped),
                                    int(bool(dark_still_biased)), _ptr(out), APGPU_F64 if t4 else APGPU_F32, N, P, _stream()))
    return out


def _stack_args(frames, calib, pixmask, keep):
    if frames.dim() < 2:
        raise ValueError('frames must be [N, ...]')
    N = frames.shape[0]
    shp = tuple(frames.shape[1:])
    P = frames[0].numel()
    # a row stripe frames_full[:, r0:r1] of a contiguous slab is reduced in place (frame_stride > P)
    if not (frames[0].is_contiguous() and (N == 1 or frames.stride(0) >= P)):
        frames = frames.contiguous()
    a = StackArgs()
    a.frames = frames.data_ptr()
    a.dtype = _raw_dtype(frames)
    a.n_frames = N
    a.n_pixels = P
    a.frame_stride = frames.stride(0) if N > 1 else P
    keep.append(frames)
    if calib is not None:
        bias, dark = _f32c(calib['bias'], 'bias'), _f32c(calib['dark'], 'dark')
        nflat = _f32c(calib.get('nflat'), 'nflat')
        e = _per_frame(calib['exp_ratio'], N, frames.device)
        ped = _per_frame(calib.get('pedestal'), N, frames.device)
        for nm, t in (('bias', bias), ('dark', dark), ('nflat', nflat)):
            if t is not None and t.numel() != P:
                raise RuntimeError('%s has %d pixels, frames have %d' % (nm, t.numel(), P))
        keep += [bias, dark, nflat, e, ped]
        a.bias, a.dark = bias.data_ptr(), dark.data_ptr()
        a.nflat = nflat.data_ptr() if nflat is not None else None
        a.exp_ratio = e.data_ptr()
        a.pedestal = ped.data_ptr() if ped is not None else None
        a.dark_still_biased = int(bool(calib.get('dark_still_biased', False)))
    if pixmask is not None:
        if pixmask.dtype != torch.uint8 or pixmask.numel() != P:
            raise TypeError('pixmask must be uint8 with one entry per pixel')
        pixmask = pixmask.contiguous()
        keep.append(pixmask)
        a.pixmask = pixmask.data_ptr()
    return a, N, P, shp, frames.device


# Workspaces of the stack's two-kernel scheme (apgpu_stack_args.workspace): one per (device, stream, pixel count), zeroed once
# - the library leaves the part that must be zero as it found it.  Keyed by the stream because a workspace must not be shared
# by calls that may run concurrently (parallel.stack_nshard alternates two compute streams).
_stack_ws = {}


def stack_workspace(n_pixels, device):
    lib = _lib.load()
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream, int(n_pixels))
    ws = _stack_ws.get(key)
    if ws is None:
        zero = C.c_size_t(0)
        nbytes = lib.apgpu_stack_ws_bytes(int(n_pixels), C.byref(zero))
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        ws[:(zero.value + 7) // 8].zero_()
        if len(_stack_ws) >= 32:                             # many image sizes in one process: forget the oldest
            _stack_ws.pop(next(iter(_stack_ws)))
        _stack_ws[key] = ws
    return ws


def _attach_workspace(a, P, dev):
    ws = stack_workspace(P, dev)
    a.workspace = ws.data_ptr()
    a.workspace_bytes = ws.numel() * 8
    return ws


def stack_redo_stats(reset=False):
    """What the fast kernels of the stack left to the redo pass, summed over this process's workspaces: dict(calls, pixels,
    pixels_listed, blocks_given_up (64-pixel blocks), fraction = share of the pixels that did not finish on the fast path).  Synchronises."""
    tot = np.zeros(4, dtype=np.int64)
    for ws in _stack_ws.values():
        torch.cuda.synchronize(ws.device)
        o = _lib.STACK_WS_STATS_OFFSET // 8
        tot += ws[o:o + 4].cpu().numpy()
        if reset:
            ws[o:o + 4].zero_()
    calls, pixels, listed, blocks = (int(x) for x in tot)
    return dict(calls=calls, pixels=pixels, pixels_listed=listed, blocks_given_up=blocks,
                fraction=((listed + 64 * blocks) / pixels if pixels else 0.0))


def stack_sigclip(frames, sigma=3.0, sigma_lower=None, sigma_upper=None, maxiters=5, cenfunc='median',
                  stdfunc='std', calib=None, pixmask=None, outputs=('mean',), exact=False, moments_mean_only=False,
                  single_kernel=False, workspace=True, nonfinite_unclipped=False):
    """Per-pixel sigma-clipped reduction along N = astropy sigma_clipped_stats(cube, axis=0)
    (sigma_clipping.py:298-383, 924-937), optionally fused with the calibration of each value.

    calib: None or dict(bias, dark, nflat=None, exp_ratio, pedestal=None, dark_still_biased=False).
    outputs: any of 'mean', 'median', 'std', 'count' (float32 / int32 planes), 'mean_f64', 'std_f64' (the unrounded
    float64 statistics, as ccdproc.combine keeps them), 'moments' (float32 [3, ...]: sum, count, sumsq) or
    'moments_f64' (dict(sum, sumsq: float64 planes, count: int32 plane) - views of one 20-byte-per-pixel buffer) or
    'moments_f64p' (the packed float64 layout float64 [3, ...] = sum, count, sumsq: dict(sum, count, sumsq, buffer,
    prefix = buffer[:2]) - what parallel.stack_nshard all-reduces in ONE call per stripe)
    -> dict of device tensors.
    exact: APGPU_STACK_EXACT_MOMENTS (float64 clip only: the mean is the float64 mean of the survivors rounded once);
    moments_mean_only: APGPU_STACK_MOMENTS_MEAN (the float64 moments will only be turned into a mean).
    single_kernel: APGPU_STACK_SINGLE_KERNEL (one complete kernel instead of the fast kernel + redo pass pair);
    nonfinite_unclipped: APGPU_STACK_NONFINITE_UNCLIPPED (stdfunc='mad_std' only): a column holding a non-finite value is not
    clipped - ccdproc >= 2.2's Combiner.sigma_clipping through astropy.stats.sigma_clip (golden group G12, arrays c*_b_*);
    workspace: True = this module's cached workspace for the two-kernel scheme (stack_workspace), False = none (the
    library then allocates a stream-ordered temporary per call), or a tensor from stack_workspace().
    """
    _need_cuda(frames)
    lib = _lib.load()
    keep = []
    a, N, P, shp, dev = _stack_args(frames, calib, pixmask, keep)
    a.center = _lib.CENTER[cenfunc]
    a.dev = _lib.DEV[stdfunc]
    a.maxiters = -1 if maxiters is None else int(maxiters)
    a.sigma_lower = float(sigma if sigma_lower is None else sigma_lower)
    a.sigma_upper = float(sigma if sigma_upper is None else sigma_upper)
    res = {}
    for k in outputs:
        if k in ('mean', 'median', 'std'):
            res[k] = torch.empty(shp, dtype=torch.float32, device=dev)
        elif k == 'count':
            res[k] = torch.empty(shp, dtype=torch.int32, device=dev)
        elif k in ('mean_f64', 'std_f64'):
            res[k] = torch.empty(shp, dtype=torch.float64, device=dev)
        elif k == 'moments':
            if a.moments:
                raise ValueError('ask for one moment layout')
            res[k] = torch.empty((3,) + shp, dtype=torch.float32, device=dev)
            a.moments = res[k].data_ptr()
            continue
        elif k in ('moments_f64', 'moments_f64p'):
            if a.moments:
                raise ValueError('ask for one moment layout')
            res[k] = alloc_moments_f64(shp, dev, packed=(k == 'moments_f64p'))
            a.moments = res[k]['buffer'].data_ptr()
            a.moments_f64 = 3 if k == 'moments_f64p' else 1
            continue
        else:
            raise ValueError('unknown output %r' % (k,))
        setattr(a, k, res[k].data_ptr())
    a.flags = ((_lib.STACK_EXACT_MOMENTS if exact else 0) | (_lib.STACK_MOMENTS_MEAN if moments_mean_only else 0) |
               (_lib.STACK_SINGLE_KERNEL if single_kernel else 0) | (_lib.STACK_NONFINITE_UNCLIPPED if nonfinite_unclipped else 0))
    if workspace is True:
        keep.append(_attach_workspace(a, P, dev))
    elif workspace is not False and workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    check(lib.apgpu_stack_sigclip(C.byref(a), _stream()))
    return res


def stack_reject(frames, method='winsorized', sigma=3.0, sigma_lower=None, sigma_upper=None, maxiters=None, nlow=1, nhigh=1,
                 calib=None, pixmask=None, outputs=('mean',), scale=None, offset=None, weights=None, box=None, row0=0,
                 esd_outliers=0.3, esd_significance=0.05, esd_low_relaxation=1.5, esd_table=None):
    """The rejection rules of small stacks (5 .. 30 registered light frames, where an outlier inflates the standard deviation
    a sigma clip judges it by), per pixel along N, at most _lib.STACK_REJECT_MAX (128) frames; include/apgpu.h has the definition.

    method 'winsorized': rounds of a median-centred clip at sigma_lower / sigma_upper (default: sigma) whose deviation is the
    Winsorized estimate - the column clamped to median +- 1.5 sig, sig = 1.134 std of that, repeated until it settles;
    maxiters rounds (None: until a round removes nothing).
    method 'minmax': the nlow lowest and the nhigh highest values of a column are dropped (ties: by frame index).
    method 'esd': the generalized extreme Studentized deviate test (Rosner 1983), for a couple of dozen frames and more: at most
    the fraction esd_outliers (0 .. 0.5) of a column's values are candidates, taken one at a time from its two ends (a low one's
    deviation divided by esd_low_relaxation >= 1), and the largest prefix of removals significant at level esd_significance
    goes - a clean column loses a value with about that probability.  esd_table: the critical values, float64
    [N + 1, max_outliers] (default: esd_lambda(N, esd_outliers, esd_significance)).
    calib / pixmask: as stack_sigclip.  outputs: any of 'mean', 'std', 'count' (float32 / int32 planes), 'mean_f64', 'std_f64'
    -> dict of device tensors; the statistics are numpy's of the survivors in frame order, the float32 planes their roundings.
    scale / offset / weights (APGPU_STACK_FRAME_PARAMS; all None: not used): one value per frame, missing ones 1 / 0 / 1.  The
    rule then runs on v = float32(float32(scale_i x) + offset_i), and the mean is sum w_i v_i / sum w_i over the survivors
    (float64, frame order); std and count stay unweighted.  Not together with calib; see frame_normalization.
    box (an int or (bh, bw); APGPU_STACK_FRAME_LOCAL): the LOCAL normalisation - frames is [N, H, W], offset a mesh [N, ny, nx]
    with one value per bh x bw box (the geometry of box_clipped_stats), scale such a mesh or None (= 1), weights one value per
    frame or None; a pixel's scale and offset are the meshes interpolated bilinearly between the box centres, held beyond the
    outer ones (see local_stats / local_normalization).  row0: the image row of frames[:, 0] when frames is a row stripe
    full[:, r0:r1] of the image the meshes describe."""
    loc = fp = None
    if box is not None:
        loc = _frame_local(frames, scale, offset, weights, box, row0, calib)
    else:
        fp = _frame_params(frames, scale, offset, weights, calib)
    if method not in ('winsorized', 'minmax', 'esd'):
        raise ValueError("method must be 'winsorized', 'minmax' or 'esd', not %r" % (method,))
    bad = [k for k in outputs if k not in ('mean', 'std', 'count', 'mean_f64', 'std_f64')]
    if bad or not outputs:
        raise ValueError('outputs of stack_reject are mean, std, count, mean_f64, std_f64; got %r' % (tuple(outputs),))
    if frames.dim() < 2:
        raise ValueError('frames must be [N, ...]')
    if frames.shape[0] > _lib.STACK_REJECT_MAX:
        raise ValueError('stack_reject takes at most %d frames (STACK_REJECT_MAX), got %d' % (_lib.STACK_REJECT_MAX, frames.shape[0]))
    if method == 'minmax':
        for nm, c in (('nlow', nlow), ('nhigh', nhigh)):
            if isinstance(c, bool) or int(c) != c or not 0 <= int(c) <= 127:
                raise ValueError('%s must be a whole number in 0 .. 127, got %r' % (nm, c))
        lo, hi, mi = float(int(nlow)), float(int(nhigh)), 1
    elif method == 'esd':
        lo, hi, mi = float(esd_outliers), float(esd_low_relaxation), 1
        if not 0.0 <= lo <= 0.5:
            raise ValueError('esd_outliers is the largest fraction of outliers, 0 .. 0.5, got %r' % (esd_outliers,))
        if not (hi >= 1.0 and np.isfinite(hi)):
            raise ValueError('esd_low_relaxation must be >= 1 and finite, got %r' % (esd_low_relaxation,))
        if esd_table is None:
            esd_table = esd_lambda(frames.shape[0], lo, esd_significance)
        esd_table = np.ascontiguousarray(esd_table, dtype=np.float64)
        if esd_table.ndim != 2 or esd_table.shape[0] != frames.shape[0] + 1 or not 1 <= esd_table.shape[1] <= 64:
            raise ValueError('esd_table must be float64 [N + 1, max_outliers] with N = %d and max_outliers in 1 .. 64, got shape %s'
                             % (frames.shape[0], esd_table.shape))
        if np.isnan(esd_table).any():
            raise ValueError('esd_table must not hold NaN')
    else:
        lo = float(sigma if sigma_lower is None else sigma_lower)
        hi = float(sigma if sigma_upper is None else sigma_upper)
        mi = -1 if maxiters is None else int(maxiters)
        if not (lo >= 0.0 and hi >= 0.0):
            raise ValueError('sigma must be >= 0')
        if mi == 0:
            raise ValueError('maxiters must be >= 1 or None')
    _need_cuda(frames)
    lib = _lib.load()
    keep = []
    a, N, P, shp, dev = _stack_args(frames, calib, pixmask, keep)
    a.center, a.dev, a.maxiters = _lib.CENTER['median'], _lib.DEV['std'], mi
    a.sigma_lower, a.sigma_upper = lo, hi
    res = {}
    for k in outputs:
        res[k] = torch.empty(shp, dtype={'count': torch.int32, 'mean_f64': torch.float64, 'std_f64': torch.float64}.get(k, torch.float32),
                             device=dev)
        setattr(a, k, res[k].data_ptr())
    a.flags = {'winsorized': _lib.STACK_REJECT_WINSORIZED, 'minmax': _lib.STACK_REJECT_MINMAX, 'esd': _lib.STACK_REJECT_ESD}[method]
    if fp is not None:
        block = torch.from_numpy(fp).to(dev)                 # float32 [3, N]: scale, offset, weight
        keep.append(block)
        a.exp_ratio = block.data_ptr()
        a.flags |= _lib.STACK_FRAME_PARAMS
    if loc is not None:
        # the meshes go up once, as one block each; the descriptor lives on the host until the call has returned
        d = _lib.StackLocal()
        d.width, d.row0 = frames.shape[2], int(row0)
        d.box_height, d.box_width = loc['box']
        d.ny, d.nx = loc['offset'].shape[1:]
        for nm in ('scale', 'offset', 'weight'):
            if loc[nm] is not None:
                t = torch.from_numpy(loc[nm]).to(dev)
                keep.append(t)
                setattr(d, nm, t.data_ptr())
        keep.append(d)
        a.workspace, a.workspace_bytes = C.addressof(d), C.sizeof(d)
        a.flags |= _lib.STACK_FRAME_LOCAL
    if method == 'esd':
        # the table goes up once; the descriptor lives on the host until the call has returned and names the meshes' one
        e = _lib.StackEsd()
        t = torch.from_numpy(esd_table).to(dev)
        keep.append(t)
        e.lambda_, e.max_outliers, e.reserved = t.data_ptr(), esd_table.shape[1], 0
        e.local = C.addressof(d) if loc is not None else None
        keep.append(e)
        a.workspace, a.workspace_bytes = C.addressof(e), C.sizeof(e)
    check(lib.apgpu_stack_sigclip(C.byref(a), _stream()))
    return res


def _betacf(a, b, x):
    """The continued fraction of the incomplete beta function (modified Lentz), to the last bits of float64."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 1000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        c = 1.0 + aa / c
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        c = 1.0 + aa / c
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h


def _betainc(a, b, x):
    """The regularized incomplete beta function I_x(a, b), 0 <= x <= 1."""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    bt = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        return bt * _betacf(a, b, x) / a
    return 1.0 - bt * _betacf(b, a, 1.0 - x) / b


def _student_t_upper(q, df):
    """t > 0 with P(T > t) = q for Student's t with df degrees of freedom, 0 < q < 0.5: the upper tail is
    I_x(df / 2, 1 / 2) / 2 at x = df / (df + t^2); a bisection brackets the root, Newton steps on log(tail) finish it."""
    def tail(t):
        return 0.5 * _betainc(0.5 * df, 0.5, df / (df + t * t))
    lo, hi = 0.0, 1.0
    while tail(hi) > q:
        lo, hi = hi, 2.0 * hi
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        if tail(mid) > q:
            lo = mid
        else:
            hi = mid
    t = 0.5 * (lo + hi)
    lognorm = math.lgamma(0.5 * (df + 1.0)) - math.lgamma(0.5 * df) - 0.5 * math.log(df * math.pi)
    for _ in range(50):
        sf = tail(t)
        pdf = math.exp(lognorm - 0.5 * (df + 1.0) * math.log1p(t * t / df))
        step = sf * math.log(sf / q) / pdf                   # Newton on log(tail(t)) - log(q)
        t_new = min(max(t + step, lo), hi)
        if abs(t_new - t) <= 4e-16 * t:
            t = t_new
            break
        t = t_new
    return t


@functools.lru_cache(maxsize=None)
def _esd_critical(m, alpha):
    """The critical value of one ESD step with m values left: p = 1 - alpha / (2 m), t the p-quantile of Student's t with
    m - 2 degrees of freedom, lambda = (m - 1) t / sqrt((m - 2 + t^2) m)."""
    t = _student_t_upper(alpha / (2.0 * m), m - 2.0)
    return (m - 1.0) * t / math.sqrt((m - 2.0 + t * t) * m)


def esd_lambda(n_frames, frac=0.3, alpha=0.05, max_outliers=None):
    """The table of critical values the ESD rule of stack_reject takes (include/apgpu.h, APGPU_STACK_REJECT_ESD): float64
    [n_frames + 1, max_outliers], row n for a column of n finite values, entry i for step i - m = n - i values left.  Entries
    with i >= K_n = min(floor(frac n), n - 3, max_outliers) and the rows n < 4 hold +inf.  max_outliers: default the largest
    K_n (at least 1), at most 64.  Plain Python: the package does not depend on SciPy."""
    n_frames, frac, alpha = int(n_frames), float(frac), float(alpha)
    if n_frames < 1:
        raise ValueError('n_frames must be >= 1')
    if not 0.0 <= frac <= 0.5:
        raise ValueError('frac is the largest fraction of outliers, 0 .. 0.5, got %r' % (frac,))
    if not 0.0 < alpha < 1.0:
        raise ValueError('alpha (the significance level) must lie in (0, 1), got %r' % (alpha,))
    kn = [min(int(np.floor(frac * n)), n - 3) for n in range(n_frames + 1)]
    if max_outliers is None:
        max_outliers = min(max(max(kn), 1), 64)
    max_outliers = int(max_outliers)
    if not 1 <= max_outliers <= 64:
        raise ValueError('max_outliers must lie in 1 .. 64, got %r' % (max_outliers,))
    lam = np.full((n_frames + 1, max_outliers), np.inf)
    for n in range(4, n_frames + 1):
        for i in range(min(kn[n], max_outliers)):
            lam[n, i] = _esd_critical(n - i, alpha)
    return lam


def _box_pair(box):
    """box as (bh, bw): an int or a pair, each 1 .. 32768."""
    bh, bw = (box, box) if np.ndim(box) == 0 else tuple(box)
    if isinstance(bh, bool) or isinstance(bw, bool) or int(bh) != bh or int(bw) != bw or not (1 <= int(bh) <= 32768 and 1 <= int(bw) <= 32768):
        raise ValueError('box must be a whole number or a pair (bh, bw) in 1 .. 32768, got %r' % (box,))
    return int(bh), int(bw)


def _frame_local(frames, scale, offset, weights, box, row0, calib):
    """The meshes and weights of APGPU_STACK_FRAME_LOCAL on the host as float32, checked (the library cannot look at device
    values): dict(box=(bh, bw), scale [N, ny, nx] or None, offset [N, ny, nx], weight [N] or None)."""
    if calib is not None:
        raise ValueError('box (the local normalisation) does not go with calib: it is for calibrated light frames')
    if frames.dim() != 3:
        raise ValueError('with box, frames must be [N, H, W]')
    if isinstance(row0, bool) or int(row0) != row0 or int(row0) < 0:
        raise ValueError('row0 must be a whole number >= 0, got %r' % (row0,))
    N = frames.shape[0]
    out = dict(box=_box_pair(box), scale=None, weight=None)
    if offset is None:
        raise ValueError('with box, offset is a mesh [N, ny, nx]')
    shape = None
    for nm, x in (('offset', offset), ('scale', scale)):
        if x is None:
            continue
        if torch.is_tensor(x):
            x = x.detach().cpu().numpy()
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 3 or x.shape[0] != N or x.size == 0 or (shape is not None and x.shape != shape):
            raise ValueError('%s must be a mesh [N, ny, nx] with N = %d%s, got shape %s'
                             % (nm, N, '' if shape is None else ' of the shape of offset', x.shape))
        shape = x.shape
        with np.errstate(over='ignore'):
            out[nm] = np.ascontiguousarray(x.astype(np.float32))
        if not np.isfinite(out[nm]).all():
            raise ValueError('%s must be finite (as float32)' % nm)
    if weights is not None:
        w = weights.detach().cpu().numpy() if torch.is_tensor(weights) else weights
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        if w.size != N:
            raise ValueError('weights must hold one value per frame (%d), got %d' % (N, w.size))
        with np.errstate(over='ignore'):
            out['weight'] = w.astype(np.float32)
        if not np.isfinite(out['weight']).all():
            raise ValueError('weights must be finite (as float32)')
        if not (out['weight'] > 0).all():
            raise ValueError('weights must be > 0 (as float32)')
    return out


def _frame_params(frames, scale, offset, weights, calib):
    """The float32 [3, N] block of APGPU_STACK_FRAME_PARAMS on the host, checked (the library cannot look at device values);
    None when none of the three is given."""
    if scale is None and offset is None and weights is None:
        return None
    if calib is not None:
        raise ValueError('scale / offset / weights do not go with calib: frame parameters are for calibrated light frames')
    if frames.dim() < 2:
        raise ValueError('frames must be [N, ...]')
    N = frames.shape[0]
    block = np.empty((3, N), dtype=np.float32)
    for row, (nm, x, default) in enumerate((('scale', scale, 1.0), ('offset', offset, 0.0), ('weights', weights, 1.0))):
        if x is None:
            block[row] = default
            continue
        if torch.is_tensor(x):
            x = x.detach().cpu().numpy()
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if x.size != N:
            raise ValueError('%s must hold one value per frame (%d), got %d' % (nm, N, x.size))
        with np.errstate(over='ignore'):
            block[row] = x.astype(np.float32)
        if not np.isfinite(block[row]).all():
            raise ValueError('%s must be finite (as float32)' % nm)
    if not (block[2] > 0).all():
        raise ValueError('weights must be > 0 (as float32)')
    return block


def frame_stats(frames, sigma=3.0, maxiters=5):
    """Per frame, the sigma-clipped median and standard deviation of its finite values (the A3 kernels, sigclip_global): what
    frame_normalization takes as a frame's location and scale.  All N reductions are queued without a host synchronisation in
    between.  Returns a float64 [N, 2] device tensor (median, std); a frame without a finite pixel has NaN."""
    _need_cuda(frames)
    if frames.dim() < 2:
        raise ValueError('frames must be [N, ...]')
    N = frames.shape[0]
    out = torch.empty((N, 2), dtype=torch.float64, device=frames.device)
    for i in range(N):
        out[i] = sigclip_global(frames[i], sigma=sigma, maxiters=maxiters)[1:3]
    return out


NORMALIZE_MODES = ('none', 'additive', 'multiplicative', 'additive+scaling')


def frame_normalization(stats, mode, reference=0, weighting=None):
    """Per-frame (scale a, offset b, weights w) - float64 numpy [N] each - that bring frames to the reference frame's level:
    v = a x + b.  stats: [N, 2] location L and scale S of every frame (frame_stats; a device tensor costs one copy to the host).

        'additive'            a = 1           b = L_r - L_i
        'multiplicative'      a = L_r / L_i   b = 0                  (every L > 0)
        'additive+scaling'    a = S_r / S_i   b = L_r - a L_i
        'none'                a = 1           b = 0

    weighting 'noise': w_i = 1 / (a_i S_i)^2 divided by the largest (0 < w <= 1); None (or 'none'): ones."""
    if mode not in NORMALIZE_MODES:
        raise ValueError('normalize must be one of ' + ', '.join(NORMALIZE_MODES) + ', not %r' % (mode,))
    if weighting not in (None, 'none', 'noise'):
        raise ValueError("weighting must be None or 'noise', not %r" % (weighting,))
    st = stats.detach().cpu().numpy() if torch.is_tensor(stats) else np.asarray(stats)
    st = np.asarray(st, dtype=np.float64)
    if st.ndim != 2 or st.shape[1] != 2 or st.shape[0] < 1:
        raise ValueError('stats must be [N, 2] (location, scale)')
    N = st.shape[0]
    r = int(reference)
    if not 0 <= r < N:
        raise ValueError('reference = %d is not a frame index (N = %d)' % (r, N))
    L, S = st[:, 0], st[:, 1]
    need_L = mode != 'none'
    need_S = mode == 'additive+scaling' or weighting == 'noise'
    for i in range(N):
        if (need_L and not np.isfinite(L[i])) or (need_S and not np.isfinite(S[i])):
            raise ValueError('frame %d has no finite pixel: no statistics to normalise it by' % i)
        if need_S and not S[i] > 0:
            raise ValueError('frame %d has scale S = %g (a constant frame): it cannot be scaled or weighted by its noise' % (i, S[i]))
        if mode == 'multiplicative' and not L[i] > 0:
            raise ValueError('frame %d has location L = %g: multiplicative normalisation needs every L > 0' % (i, L[i]))
    if mode == 'additive':
        a, b = np.ones(N), L[r] - L
    elif mode == 'multiplicative':
        a, b = L[r] / L, np.zeros(N)
    elif mode == 'additive+scaling':
        a = S[r] / S
        b = L[r] - a * L
    else:
        a, b = np.ones(N), np.zeros(N)
    if weighting == 'noise':
        w = 1.0 / (a * S) ** 2
        w = w / w.max()
    else:
        w = np.ones(N)
    return a, b, w


def local_stats(frames, box, sigma=3.0, maxiters=5):
    """Per frame and per box of bh x bw pixels (box: an int or (bh, bw)), the sigma-clipped median and standard deviation of the
    box's finite pixels: box_clipped_stats(frames[i], None, bh, bw) for every frame, all N launches queued without a host
    synchronisation in between.  frames: [N, H, W] float32 or uint16 (widened frame by frame).  Returns a float64
    [N, ny, nx, 4] device tensor = median, std, survivors, pixels masked before clipping (outside the image or not finite);
    what local_normalization takes."""
    _need_cuda(frames)
    if frames.dim() != 3:
        raise ValueError('frames must be [N, H, W]')
    bh, bw = _box_pair(box)
    N, H, W = frames.shape
    out = torch.empty((N, -(-H // bh), -(-W // bw), 4), dtype=torch.float64, device=frames.device)
    for i in range(N):
        f = frames[i] if frames.dtype == torch.float32 else widen_u16(frames[i], torch.float32)
        out[i] = box_clipped_stats(f, None, bh, bw, sigma=sigma, maxiters=maxiters)
    return out


def local_normalization(stats, mode, reference=0, weighting=None, min_fraction=0.5, filter_size=1, box=None):
    """Per-frame MESHES of scale a and offset b (and one weight per frame) that bring every box of every frame to the level the
    reference frame has in that box: v = a(y, x) x + b(y, x) inside stack_reject(..., box=).  stats: [N, ny, nx, 4] from
    local_stats (a device tensor costs one copy to the host; the rest is float64 NumPy on a few hundred numbers).

    A box of frame i is USABLE when its survivors are at least min_fraction of the full box area bh * bw (box: as given to
    local_stats; None: the largest survivors + masked count in stats stands in for the area) - so partial boxes at the edges
    and resampling holes drop out - in frame i AND in the reference; for 'additive+scaling' and weighting='noise' both scales S
    must also be > 0, for 'multiplicative' both locations L.  In usable boxes frame_normalization's table holds per box:

        'additive'            a = 1 (scale is returned as None)   b = L_r - L_i
        'multiplicative'      a = L_r / L_i                       b = 0
        'additive+scaling'    a = S_r / S_i                       b = L_r - a L_i
        'none'                a = 1 (None)                        b = 0

    Unusable boxes are filled by inverse-distance weighting over the nearest usable ones (mesh.fill_excluded, as the sky-
    background model does) and every mesh then passes a nanmedian filter of filter_size (mesh.nanmedian_filter; 1: none).  The
    default is NO filter: the filter's windows are cut off at the mesh's rim, so the rim cells of a sloping mesh - the very thing
    this normalisation is for - are pulled inwards by up to half a box of slope (DESIGN 4.1f has the figures); ask for 3 where
    single boxes may be off and the sky is flat.  The reference frame is exactly (1, 0) everywhere.  A frame without one usable
    box raises ValueError.
    weighting 'noise': w_i = 1 / (median over frame i's usable boxes of a_i S_i)^2, divided by the largest; None: ones.
    Returns (scale float32 [N, ny, nx] or None, offset float32 [N, ny, nx], weights float64 [N])."""
    from .mesh import fill_excluded, nanmedian_filter
    if mode not in NORMALIZE_MODES:
        raise ValueError('normalize must be one of ' + ', '.join(NORMALIZE_MODES) + ', not %r' % (mode,))
    if weighting == 'none':
        weighting = None
    if weighting not in (None, 'noise'):
        raise ValueError("weighting must be None or 'noise', not %r" % (weighting,))
    st = stats.detach().cpu().numpy() if torch.is_tensor(stats) else np.asarray(stats)
    st = np.asarray(st, dtype=np.float64)
    if st.ndim != 4 or st.shape[3] != 4 or st.size == 0:
        raise ValueError('stats must be [N, ny, nx, 4] (median, std, survivors, masked)')
    N = st.shape[0]
    r = int(reference)
    if not 0 <= r < N:
        raise ValueError('reference = %d is not a frame index (N = %d)' % (r, N))
    if not 0.0 <= float(min_fraction) <= 1.0:
        raise ValueError('min_fraction must be in 0 .. 1, got %r' % (min_fraction,))
    L, S, cnt = st[..., 0], st[..., 1], st[..., 2]
    if box is None:
        area = float((st[..., 2] + st[..., 3]).max())
    else:
        bh, bw = _box_pair(box)
        area = float(bh * bw)
    need_S = mode == 'additive+scaling' or weighting == 'noise'
    ok = (cnt >= float(min_fraction) * area) & (cnt > 0) & np.isfinite(L) & np.isfinite(S)
    if need_S:
        ok &= S > 0
    if mode == 'multiplicative':
        ok &= L > 0
    scaled = mode in ('multiplicative', 'additive+scaling')
    A = np.ones(st.shape[:3])
    B = np.zeros(st.shape[:3])
    w = np.ones(N)
    for i in range(N):
        good = ok[i] & ok[r]
        if not good.any():
            raise ValueError('frame %d has no usable box (%s): nothing to normalise it by'
                             % (i, 'none of its own' if not ok[i].any() else 'none shared with the reference frame %d' % r))
        with np.errstate(invalid='ignore', divide='ignore'):
            if mode == 'additive':
                a, b = np.ones_like(L[i]), L[r] - L[i]
            elif mode == 'multiplicative':
                a, b = L[r] / L[i], np.zeros_like(L[i])
            elif mode == 'additive+scaling':
                a = S[r] / S[i]
                b = L[r] - a * L[i]
            else:
                a, b = np.ones_like(L[i]), np.zeros_like(L[i])
        if weighting == 'noise':
            w[i] = 1.0 / float(np.median((a * S[i])[good])) ** 2
        if i == r:
            continue                                         # exactly (1, 0) everywhere
        if scaled:
            A[i] = nanmedian_filter(fill_excluded(np.where(good, a, np.nan), good), int(filter_size))
        if mode != 'none':
            B[i] = nanmedian_filter(fill_excluded(np.where(good, b, np.nan), good), int(filter_size))
    if weighting == 'noise':
        if not np.isfinite(w).all():
            raise ValueError('a frame has no measurable noise in its usable boxes: it cannot be weighted by it')
        w = w / w.max()
    with np.errstate(over='ignore'):
        A32, B32 = A.astype(np.float32), B.astype(np.float32)
    if not (np.isfinite(A32).all() and np.isfinite(B32).all()):
        raise ValueError('the normalisation meshes are not finite as float32')
    return (A32 if scaled else None), B32, w


def stack_sigclip_chunked(frames, chunk=None, want_std=False, packed=False, finalize=True, exact=False, **clip):
    """A stack of MORE than APGPU_MAX_STACK (512) frames on one GPU: the frames are reduced in chunks of at most `chunk`
    (default: the largest equal split not above 512), every chunk clipped against its own statistics, and the float64
    moments of the chunks accumulate in one buffer (apgpu_stack_args.moments_f64 = 2) - the single-GPU form of the
    N-shard combine (parallel.stack_nshard).  Exact for an unclipped mean; for a clipped stack the semantics are
    hierarchical (SURVEY 8(e) option ii), NOT the full-N clip.  clip: sigma, maxiters, cenfunc, stdfunc, calib, pixmask.
    packed: accumulate in the packed float64 layout (sum, count, sumsq planes) the N-shard exchange all-reduces;
    finalize=False returns the moment dict itself (a rank's share of a hierarchical stack, parallel.stack_nshard).
    Returns dict(mean, count[, std])."""
    _need_cuda(frames)
    lib = _lib.load()
    N = frames.shape[0]
    if chunk is None:
        parts = -(-N // _lib.MAX_STACK)
        chunk = -(-N // parts)
    chunk = int(min(chunk, _lib.MAX_STACK))
    shp = tuple(frames.shape[1:])
    mom = alloc_moments_f64(shp, frames.device, packed=packed)
    calib = clip.pop('calib', None)
    pixmask = clip.pop('pixmask', None)
    for k, lo in enumerate(range(0, N, chunk)):
        hi = min(N, lo + chunk)
        c = None
        if calib is not None:
            c = dict(calib)
            for key in ('exp_ratio', 'pedestal'):
                v = c.get(key)
                if v is not None and not np.isscalar(v):
                    c[key] = v[lo:hi]
        keep = []
        a, n, P, _, dev = _stack_args(frames[lo:hi], c, pixmask, keep)
        a.center = _lib.CENTER[clip.get('cenfunc', 'median')]
        a.dev = _lib.DEV[clip.get('stdfunc', 'std')]
        mi = clip.get('maxiters', 5)
        a.maxiters = -1 if mi is None else int(mi)
        sg = clip.get('sigma', 3.0)
        sl, su = clip.get('sigma_lower'), clip.get('sigma_upper')
        a.sigma_lower = float(sg if sl is None else sl)      # an explicit 0.0 is a value, not "unset"
        a.sigma_upper = float(sg if su is None else su)
        a.moments = mom['buffer'].data_ptr()
        a.moments_f64 = (3 if k == 0 else 4) if packed else (1 if k == 0 else 2)
        a.flags = (0 if want_std else _lib.STACK_MOMENTS_MEAN) | (_lib.STACK_EXACT_MOMENTS if exact else 0)   # exact: float64 clip only
        keep.append(_attach_workspace(a, P, dev))
        check(lib.apgpu_stack_sigclip(C.byref(a), _stream()))
    if not finalize:
        return mom
    out = moments_finalize(mom, want_std=want_std)
    res = dict(count=mom['count'].to(torch.int32) if packed else mom['count'])
    if want_std:
        res['mean'], res['std'] = out
    else:
        res['mean'] = out
    return res


def combine_f64(frames, sigma_lower=5.0, sigma_upper=5.0, maxiters=1, cenfunc='median', stdfunc='mad_std', form='astropy'):
    """The ccdproc.combine configuration (scripts/ap_combine_darks.py:394-420) on a FLOAT64 slab [N, ...]: one strict
    pass about the median with mad_std, float64 mean / std / count -> dict(mean_f64, std_f64, count).  float64 frames are
    never narrowed to float32 (apgpu_combine_ccdproc_f64: a correctness path, bit-identical to the oracle).
    form: 'astropy' (ccdproc >= 2.2: astropy.stats.sigma_clip) or 'legacy' (ccdproc <= 2.1), see include/apgpu.h."""
    _need_cuda(frames)
    if frames.dtype != torch.float64:
        raise TypeError('combine_f64 takes a float64 slab, got %s' % frames.dtype)
    if maxiters != 1 or cenfunc != 'median' or stdfunc != 'mad_std':
        raise ValueError('combine_f64 implements the ccdproc.combine configuration only: maxiters=1, median, mad_std')
    lib = _lib.load()
    N = frames.shape[0]
    shp = tuple(frames.shape[1:])
    P = frames[0].numel()
    if not (frames[0].is_contiguous() and (N == 1 or frames.stride(0) >= P)):
        frames = frames.contiguous()
    dev = frames.device
    res = dict(mean_f64=torch.empty(shp, dtype=torch.float64, device=dev), std_f64=torch.empty(shp, dtype=torch.float64, device=dev),
               count=torch.empty(shp, dtype=torch.int32, device=dev))
    nb = lib.apgpu_combine_ccdproc_f64_ws_bytes(N, P)
    ws = torch.empty(nb // 8, dtype=torch.float64, device=dev)
    check(lib.apgpu_combine_ccdproc_f64(_ptr(frames), N, P, frames.stride(0) if N > 1 else P, float(sigma_lower), float(sigma_upper),
                                        _lib.CCDPROC_FORM[form], _ptr(res['mean_f64']), _ptr(res['count']), _ptr(res['std_f64']), _ptr(ws), nb, _stream()))
    return res


def stack_kernel_name(n_frames, dtype='f32', calibrated=True, outputs=('mean',), median_only=False, stdfunc='std',
                      moments_mean_only=False, exact=False, maxiters=5, rejection=None):
    """Name of the kernel variant the library dispatches for such a stack call (apgpu_stack_kernel_name): what the
    bench line and the profiles call the dominant kernel.  Needs no device.  rejection: None, 'winsorized', 'minmax' or 'esd'
    (stack_reject)."""
    if rejection not in (None, 'winsorized', 'minmax', 'esd'):
        raise ValueError("rejection must be None, 'winsorized', 'minmax' or 'esd'")
    lib = _lib.load()
    a = StackArgs()
    a.frames = 0x1000                                     # placeholders: aligned, never dereferenced by the query
    a.dtype = APGPU_F32 if dtype in ('f32', torch.float32) else APGPU_U16
    a.n_frames = int(n_frames)
    a.n_pixels = 1 << 20
    a.frame_stride = 1 << 20
    if calibrated:
        a.bias = a.dark = a.nflat = a.exp_ratio = 0x1000
    a.center, a.dev, a.maxiters = 0, _lib.DEV[stdfunc], int(maxiters)
    a.sigma_lower = a.sigma_upper = 3.0
    if median_only:
        a.median = 0x1000
    for k in outputs:
        if k in ('moments_f64', 'moments_f64p'):
            a.moments, a.moments_f64 = 0x1000, (3 if k == 'moments_f64p' else 1)
        elif k == 'moments':
            a.moments = 0x1000
        else:
            setattr(a, k, 0x1000)
    a.flags = (_lib.STACK_EXACT_MOMENTS if exact else 0) | (_lib.STACK_MOMENTS_MEAN if moments_mean_only else 0)
    if rejection is not None:
        a.flags |= {'winsorized': _lib.STACK_REJECT_WINSORIZED, 'minmax': _lib.STACK_REJECT_MINMAX, 'esd': _lib.STACK_REJECT_ESD}[rejection]
        if rejection == 'minmax':
            a.sigma_lower = a.sigma_upper = 1.0
        if rejection == 'esd':
            a.sigma_lower, a.sigma_upper = 0.3, 1.5
            e = _lib.StackEsd()
            e.lambda_, e.max_outliers = 0x1000, 1
            a.workspace, a.workspace_bytes = C.addressof(e), C.sizeof(e)
    buf = C.create_string_buffer(256)
    check(lib.apgpu_stack_kernel_name(C.byref(a), int(bool(median_only)), buf, 256))
    return buf.value.decode()


def stack_median(frames, calib=None, pixmask=None, want_count=False):
    """np.nanmedian(cube, axis=0) (config 4), optionally fused with calibration."""
    _need_cuda(frames)
    lib = _lib.load()
    keep = []
    a, N, P, shp, dev = _stack_args(frames, calib, pixmask, keep)
    med = torch.empty(shp, dtype=torch.float32, device=dev)
    a.median = med.data_ptr()
    cnt = None
    if want_count:
        cnt = torch.empty(shp, dtype=torch.int32, device=dev)
        a.count = cnt.data_ptr()
    check(lib.apgpu_stack_median(C.byref(a), _stream()))
    return (med, cnt) if want_count else med


def alloc_moments_f64(shape, device, packed=False):
    """The float64 moment layouts of include/apgpu.h.  Default: one buffer = double sum[P], double sumsq[P], int32 count[P]
    -> dict(sum, sumsq, count, buffer) of views with the image shape.  packed: float64 [3][P] = sum, count, sumsq ->
    dict(sum, count, sumsq, buffer, prefix) with prefix = the contiguous (sum, count) planes a mean-only exchange sends."""
    shape = tuple(shape)
    P = int(np.prod(shape)) if shape else 1
    if packed:
        buf = torch.empty((3,) + shape, dtype=torch.float64, device=device)
        return dict(sum=buf[0], count=buf[1], sumsq=buf[2], buffer=buf, prefix=buf[:2], packed=True)
    buf = torch.empty(2 * P + (P + 1) // 2, dtype=torch.float64, device=device)
    return dict(sum=buf[:P].view(shape), sumsq=buf[P:2 * P].view(shape),
                count=buf[2 * P:].view(torch.int32)[:P].view(shape), buffer=buf)


def moments_finalize(moments, want_std=None, out_mean=None, want_f64=False):
    """Mean (and std) of the survivors from (all-reduced) partial moments.

    moments: the float32 tensor [2 or 3, ...] = (sum, cnt[, sumsq]) -> mean = sum / cnt in float32; no std from this
    layout (sumsq / cnt - mean^2 of float32 sums about zero cancels: ask for 'moments_f64' instead); or the dict
    stack_sigclip(..., outputs=('moments_f64',)) returns -> mean = sum / cnt, std = sqrt(sumsq / cnt - mean^2)
    evaluated in float64 and rounded once (want_f64: also return the float64 planes)."""
    lib = _lib.load()
    if want_std is None:
        want_std = isinstance(moments, dict) and moments.get('sumsq') is not None
    if isinstance(moments, dict):
        sm, sq, cnt = moments['sum'], moments.get('sumsq'), moments['count']
        _need_cuda(sm, sq, cnt)
        shp = tuple(sm.shape)
        P = sm.numel()
        packed = cnt.dtype == torch.float64                  # the packed layout carries the count as a float64 plane
        for t, dt, nm in ((sm, torch.float64, 'sum'), (sq, torch.float64, 'sumsq'), (cnt, torch.float64 if packed else torch.int32, 'count')):
            if t is not None and (t.dtype != dt or t.numel() != P or not t.is_contiguous()):
                raise TypeError('moments_f64[%r] must be a contiguous %s plane' % (nm, dt))
        if want_std and sq is None:
            raise ValueError('std needs the sumsq plane')
        if out_mean is None:
            mean = torch.empty(shp, dtype=torch.float32, device=sm.device)
        else:
            mean = out_mean
            if mean.dtype != torch.float32 or mean.numel() != P or not mean.is_contiguous():
                raise TypeError('out_mean must be a contiguous float32 tensor with one entry per pixel')
        std = torch.empty(shp, dtype=torch.float32, device=sm.device) if want_std else None
        m64 = torch.empty(shp, dtype=torch.float64, device=sm.device) if want_f64 else None
        s64 = torch.empty(shp, dtype=torch.float64, device=sm.device) if (want_f64 and want_std) else None
        if packed:
            check(lib.apgpu_moments_finalize_f64p(_ptr(sm), _ptr(cnt), _ptr(sq) if want_std else None, _ptr(mean), _ptr(std),
                                                  _ptr(m64), _ptr(s64), P, _stream()))
        else:
            check(lib.apgpu_moments_finalize_f64(_ptr(sm), _ptr(sq) if want_std else None, _ptr(cnt), _ptr(mean), _ptr(std),
                                                 _ptr(m64), _ptr(s64), P, _stream()))
        out = (mean, std) if want_std else mean
        if want_f64:
            return out, ((m64, s64) if want_std else m64)
        return out
    _need_cuda(moments)
    if want_std:
        raise ValueError("no standard deviation from float32 moments (sumsq/cnt - mean^2 cancels for CCD-range data): "
                         "use outputs=('moments_f64',)")
    moments = _f32c(moments, 'moments')
    shp = tuple(moments.shape[1:])
    P = moments[0].numel()
    if out_mean is None:
        mean = torch.empty(shp, dtype=torch.float32, device=moments.device)
    else:
        mean = out_mean
        if mean.dtype != torch.float32 or mean.numel() != P or not mean.is_contiguous():
            raise TypeError('out_mean must be a contiguous float32 tensor with one entry per pixel')
    std = torch.empty(shp, dtype=torch.float32, device=moments.device) if want_std else None
    check(lib.apgpu_moments_finalize(_ptr(moments), _ptr(mean), _ptr(std), P, _stream()))
    return (mean, std) if want_std else mean


def sigclip_global(data, sigma=3.0, sigma_lower=None, sigma_upper=None, maxiters=5):
    """A3 sigma_clipped_stats(data, sigma) with axis=None (ApFindBadPixels.py:191).

    float32 data -> numpy's float32 statistics; float64 and integer data (widened exactly) -> float64
    statistics, as numpy computes them.  Returns a float64 device tensor [10] =
    mean, median, std, lo, hi, iterations, survivors, min, max, 0."""
    _need_cuda(data)
    lib = _lib.load()
    if data.dtype == torch.float32:
        f64 = False
        data = data.contiguous()
    else:
        f64 = True
        if data.dtype == torch.uint16:
            data = widen_u16(data, torch.float64)
        else:
            data = data.to(torch.float64)
        data = data.contiguous()
    n = data.numel()
    ws_bytes = (lib.apgpu_sigclip_global_f64_ws_bytes if f64 else lib.apgpu_sigclip_global_ws_bytes)(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=data.device)
    stats = torch.empty(10, dtype=torch.float64, device=data.device)
    sl = float(sigma if sigma_lower is None else sigma_lower)
    su = float(sigma if sigma_upper is None else sigma_upper)
    fn = lib.apgpu_sigclip_global_f64 if f64 else lib.apgpu_sigclip_global_f32
    check(fn(_ptr(data), n, sl, su, -1 if maxiters is None else int(maxiters), _ptr(stats), _ptr(ws), ws_bytes, _stream()))
    return stats


def _median_dtype(x):
    """F5 inputs: float32 stays float32; float64 and integer tensors -> float64 (numpy takes the median of integers in
    float64; every integer converts monotonically, so widening first selects the same element)."""
    if x.dtype == torch.float32:
        return x.contiguous(), APGPU_F32
    if x.dtype == torch.uint16:
        return x.contiguous(), APGPU_U16                # widened to float64 inside the kernel
    if x.dtype not in (torch.float64, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        raise TypeError('axis medians take float32, float64 or integer data, got %s' % x.dtype)
    return x.to(torch.float64).contiguous(), APGPU_F64


def axis_nanmedian(x, axis):
    """F5 np.nanmedian(x, axis) of an image [H, W] or of every frame of a slab [N, H, W] (ApAutoBadcols.py:196, :200).

    axis 0 (or -2): per column -> [W] / [N, W]; axis 1 (or -1): per row -> [H] / [N, H].  float32 data gives float32
    medians, float64 and integer data float64 medians, bit-exact with numpy 1.26 (both of its nanmedian paths)."""
    _need_cuda(x)
    if x.dim() not in (2, 3):
        raise ValueError('axis_nanmedian takes [H, W] or [N, H, W], got shape %s' % (tuple(x.shape),))
    if axis not in (0, 1, -1, -2):
        raise ValueError('axis must be 0 or 1 (an axis of one image), got %r' % (axis,))
    axis = axis % 2
    single = x.dim() == 2
    x3 = x.unsqueeze(0) if single else x
    N, H, W = x3.shape
    if N == 0 or H == 0 or W == 0:
        raise ValueError('axis_nanmedian: empty input of shape %s' % (tuple(x.shape),))
    d, dt = _median_dtype(x3)
    out = torch.empty((N, W if axis == 0 else H), dtype=torch.float32 if dt == APGPU_F32 else torch.float64, device=d.device)
    check(_lib.load().apgpu_axis_nanmedian(_ptr(d), dt, N, H, W, axis, _ptr(out), _stream()))
    return out[0] if single else out


def sliding_clipped_stats(v, window_len, sigma=3.0, maxiters=5, nsigma=5.0):
    """F5 ApAutoBadcols._sliding_stats_1d (ApAutoBadcols.py:143-167) and the flag of _process (:225-227) for one line
    [L] or a batch of lines [B, L] (float32 or float64; numpy's statistics in that dtype).

    maxiters None = until convergence.  Returns dict(mean, std, nsig: float64, flag: uint8), each shaped like v."""
    _need_cuda(v)
    if v.dim() not in (1, 2) or v.numel() == 0:
        raise ValueError('sliding_clipped_stats takes a non-empty [L] or [B, L] tensor, got shape %s' % (tuple(v.shape),))
    window_len = int(window_len)
    if window_len < 1:
        raise ValueError('window_len must be >= 1, got %d' % window_len)
    if v.dtype == torch.float32:
        dt = APGPU_F32
    elif v.dtype == torch.float64:
        dt = APGPU_F64
    else:
        raise TypeError('sliding_clipped_stats takes float32 or float64 values, got %s' % v.dtype)
    v2 = v.reshape(1, -1) if v.dim() == 1 else v
    v2 = v2.contiguous()
    B, L = v2.shape
    lib = _lib.load()
    ws_bytes = lib.apgpu_sliding_clipped_stats_ws_bytes(dt, B, L, window_len)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=v.device)
    mean = torch.empty((B, L), dtype=torch.float64, device=v.device)
    std = torch.empty_like(mean)
    nsig = torch.empty_like(mean)
    flag = torch.empty((B, L), dtype=torch.uint8, device=v.device)
    check(lib.apgpu_sliding_clipped_stats(_ptr(v2), dt, B, L, window_len, float(sigma), -1 if maxiters is None else int(maxiters),
                                          float(nsigma), _ptr(mean), _ptr(std), _ptr(nsig), _ptr(flag), _ptr(ws), ws_bytes,
                                          _stream()))
    r = dict(mean=mean, std=std, nsig=nsig, flag=flag)
    return {k: t.reshape(v.shape) for k, t in r.items()}


def auto_badcols(data, nsigma=5.0, window_len=11):
    """F5 ApAutoBadcols.process (ApAutoBadcols.py:180-258) on the device, for an image [H, W] or a slab [N, H, W]:
    column and row medians, their sliding clipped statistics and the bad flags, launched back to back on the current
    stream without a host synchronisation.

    Returns {'cols': dict(median, mean, std, nsig, flag), 'rows': ...}, device tensors shaped [W] / [H] (or [N, W] /
    [N, H]); indices with flag 1 are the reference's bad columns / rows (0-based)."""
    out = {}
    for tag, axis in (('cols', 0), ('rows', 1)):
        med = axis_nanmedian(data, axis)
        r = sliding_clipped_stats(med, window_len, nsigma=nsigma)
        r['median'] = med
        out[tag] = r
    return out


def image_difference(a, b, bad1=None, bad2=None):
    """F2 ApImageDifference (ap_calc_read_noise.py:122): float64(a) - float64(b), NaN where bad1|bad2."""
    _need_cuda(a, b, bad1, bad2)
    a, b = a.contiguous(), b.contiguous()
    dt = _raw_dtype(a)
    if _raw_dtype(b) != dt or a.shape != b.shape:
        raise RuntimeError('Error, data array shapes do not match: First file=%s, second file=%s' % (tuple(a.shape), tuple(b.shape)))
    for m in (bad1, bad2):
        if m is not None and (m.dtype != torch.uint8 or m.shape != a.shape):
            raise TypeError('bad-pixel masks must be uint8 with the image shape')
    bad1 = None if bad1 is None else bad1.contiguous()
    bad2 = None if bad2 is None else bad2.contiguous()
    out = torch.empty(a.shape, dtype=torch.float64, device=a.device)
    check(_lib.load().apgpu_image_difference_f64(_ptr(a), _ptr(b), dt, _ptr(bad1), _ptr(bad2), _ptr(out), a.numel(), _stream()))
    return out


def threshold_mask(data, lothresh=0.0, hithresh=0.0, thresholds=None):
    """A4 ApFindBadPixels._generate_sigmaclip_mask (ApFindBadPixels.py:199-216).

    thresholds: optional float64 device tensor [2] read on the device instead of the two floats.
    Returns (mask uint8, nbad int64[1] device tensor)."""
    _need_cuda(data, thresholds)
    lib = _lib.load()
    data = _aligned16(_f32c(data, 'data'))
    mask = torch.empty(data.shape, dtype=torch.uint8, device=data.device)
    nbad = torch.empty(1, dtype=torch.int64, device=data.device)
    if thresholds is not None and (thresholds.dtype != torch.float64 or thresholds.numel() < 2):
        raise TypeError('thresholds must be a float64 tensor with 2 entries')
    check(lib.apgpu_threshold_mask_f32(_ptr(data), data.numel(), float(lothresh), float(hithresh), _ptr(thresholds),
                                       _ptr(mask), _ptr(nbad), _stream()))
    return mask, nbad


def mask_add_rects(mask, rects, value=2):
    """A4 overlays (ApFindBadPixels.py:90,128,154): mask[r0:r1, c0:c1] += value in place."""
    _need_cuda(mask)
    if mask.dtype != torch.uint8 or mask.dim() != 2 or not mask.is_contiguous():
        raise TypeError('mask must be a contiguous 2-D uint8 tensor')
    r = np.ascontiguousarray(np.asarray(rects, dtype=np.int32).reshape(-1, 4))
    if r.shape[0] == 0:
        return mask
    H, W = mask.shape
    if (r[:, 0] < 0).any() or (r[:, 1] > H).any() or (r[:, 2] < 0).any() or (r[:, 3] > W).any():
        raise ValueError('rectangle outside the image')
    rd = torch.from_numpy(r).to(mask.device)
    check(_lib.load().apgpu_mask_add_rects_u8(_ptr(mask), H, W, _ptr(rd), r.shape[0], int(value), _stream()))
    return mask


def fix_badpix(data, mask, deltapix=1, min_valid=4):
    """A5 ApFixBadPixels.fix_bad_pixels (ApFixBadPixels.py:292-445).

    float32 or float64 images (medians in the image's own type, as np.median); any deltapix >= 0.
    Returns (out, stats int64[3] device tensor = nbad, nfixed, nremaining)."""
    _need_cuda(data, mask)
    f64 = data.dtype == torch.float64
    data = data.contiguous() if f64 else _f32c(data, 'data')
    if data.dim() != 2:
        raise ValueError('data must be 2-D')
    m8 = _mask_u8(mask, data.shape, 'Error, the shape of the input data array (%s) does not match that of the bad pixel '
                  'mask array (%s).' % (tuple(data.shape), tuple(mask.shape)), RuntimeError)
    out = torch.empty_like(data)
    stats = torch.empty(3, dtype=torch.int64, device=data.device)
    fn = _lib.load().apgpu_fix_badpix_f64 if f64 else _lib.load().apgpu_fix_badpix_f32
    check(fn(_ptr(data), _ptr(m8), data.shape[0], data.shape[1], int(deltapix), int(min_valid), _ptr(out), _ptr(stats), _stream()))
    return out, stats


def imarith(a, op, b):
    """A8 ApImArith op block (ApImArith.py:320-333): a (op) b, b a tensor or a python float."""
    _need_cuda(a)
    a = a.contiguous()
    opi = _lib.OPS[op]
    b_is_t = torch.is_tensor(b)
    if a.dtype == torch.float64 or (b_is_t and b.dtype == torch.float64 and a.dtype == torch.float32):
        # float64 somewhere: computed in float64, stored in a's dtype (numpy, out=zeros_like(data1))
        out = torch.empty_like(a)
        adt = _dtype_tag(a, 'a')
        if b_is_t:
            _need_cuda(b)
            if b.shape != a.shape:
                raise RuntimeError('Error, the dimension of the second data array does not match the first.')
            b = b.contiguous()
            check(_lib.load().apgpu_imarith_f64(_ptr(a), adt, _ptr(b), _dtype_tag(b, 'b'), 0.0, opi, _ptr(out), a.numel(), _stream()))
        else:
            check(_lib.load().apgpu_imarith_f64(_ptr(a), adt, None, APGPU_F64, float(b), opi, _ptr(out), a.numel(), _stream()))
        return out
    dt = _raw_dtype(a)
    a = _aligned16(a)
    out = torch.empty_like(a)
    if torch.is_tensor(b):
        _need_cuda(b)
        if b.shape != a.shape:
            raise RuntimeError('Error, the dimension of the second data array does not match the first.')
        if _raw_dtype(b) != dt:
            raise TypeError('operands must have the same dtype')
        b = _aligned16(b)
        check(_lib.load().apgpu_imarith(_ptr(a), _ptr(b), 0.0, opi, dt, _ptr(out), a.numel(), _stream()))
    else:
        check(_lib.load().apgpu_imarith(_ptr(a), None, float(b), opi, dt, _ptr(out), a.numel(), _stream()))
    return out


def bayer_split(raw, pattern=(0, 1, 3, 2), black=None):
    """A9 RawConv split geometry (RawConv.py:111-128): four full-size planes [4,H,W] (R, G1, B, G2)."""
    _need_cuda(raw)
    if _raw_dtype(raw) != APGPU_U16 or raw.dim() != 2:
        raise TypeError('raw must be a 2-D uint16 tensor')
    raw = raw.contiguous()
    H, W = raw.shape
    planes = torch.empty((4, H, W), dtype=raw.dtype, device=raw.device)
    pat = (C.c_int32 * 4)(*[int(x) for x in pattern])
    blk = (C.c_int32 * 4)(*[int(x) for x in black]) if black is not None else None
    check(_lib.load().apgpu_bayer_split_u16(_ptr(raw), H, W, pat, blk, _ptr(planes), _stream()))
    return planes


def bayer_flat_normalize(flat):
    """Per-channel flat normalisation for a Bayer mosaic (config 4): every 2x2 cell position (R, G1, G2, B)
    is normalised by the nanmean of its own quarter-plane with the A1 kernel, i.e. four applications of
    ApCalibrate._generate_flat (ApCalibrate.py:166-190) on the planes RawConv.split separates
    (RawConv.py:111-128).  Returns (nflat[H,W], norms[2,2] device tensor)."""
    _need_cuda(flat)
    flat = _f32c(flat, 'flat')
    if flat.dim() != 2 or flat.shape[0] % 2 or flat.shape[1] % 2:
        raise ValueError('a Bayer mosaic needs an even number of rows and columns')
    nflat = torch.empty_like(flat)
    norms = torch.empty((2, 2), dtype=torch.float32, device=flat.device)
    for r0 in (0, 1):
        for c0 in (0, 1):
            plane = flat[r0::2, c0::2].contiguous()
            npl, norm = flat_normalize(plane)
            nflat[r0::2, c0::2] = npl
            norms[r0, c0] = norm[0]
    return nflat, norms


# ---------------------------------------------------------------------------------------------------
# F3: registration resample (what the reference runs SWarp for, scripts/resample_all.sh:123-131, 330-342)
# ---------------------------------------------------------------------------------------------------
_LUT_CACHE = {}


def lanczos3_table(n_phases=1024, device='cuda'):
    """[n_phases + 1, 6] float32 device tensor: row p = normalised Lanczos-3 weights of the taps
    floor(x)-2 .. floor(x)+3 for a fractional offset t = p / n_phases (tap k at distance d = k - 2 - t,
    L(d) = sinc(d) sinc(d/3) for |d| < 3).  Built once per (n_phases, device) in float64 on the host."""
    import numpy as np
    key = (int(n_phases), str(device))
    if key not in _LUT_CACHE:
        t = np.arange(n_phases + 1, dtype=np.float64)[:, None] / n_phases
        d = np.arange(6, dtype=np.float64)[None, :] - 2.0 - t
        w = np.sinc(d) * np.sinc(d / 3.0)
        w[np.abs(d) >= 3.0] = 0.0
        w[np.abs(w) < 1e-12] = 0.0              # np.sinc(integer) is ~1e-17, not 0: whole-pixel offsets are exact copies
        w /= w.sum(axis=1, keepdims=True)
        _LUT_CACHE[key] = torch.from_numpy(np.ascontiguousarray(w.astype(np.float32))).to(device)
    return _LUT_CACHE[key]


def _resample_args(frames, affines, fscale, mask, out_shape, n_phases):
    """Shared argument preparation of the resample entry points: frames [N,H,W] float32 contiguous, transforms as a float64 device
    tensor ([N,6] or per-tile [N,ty,tx,6]), flux scales, mask as uint8, the weight table -> (frames, N, H, W, h, w, aff, per_tile, fs, mk, lut)."""
    _need_cuda(frames)
    frames = _f32c(frames, 'frames')
    if frames.dim() == 2:
        frames = frames[None]
    if frames.dim() != 3:
        raise ValueError('frames must be [N,H,W] or [H,W]')
    N, H, W = frames.shape
    dev = frames.device
    h, w = (H, W) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
    aff = torch.as_tensor(affines, dtype=torch.float64)
    per_tile = aff.dim() == 4
    if per_tile:
        ty, tx = (h + 15) // 16, (w + 63) // 64
        if tuple(aff.shape) != (N, ty, tx, 6):
            raise ValueError('per-tile affines must be [N, %d, %d, 6] for a %d x %d output' % (ty, tx, h, w))
    else:
        aff = aff.reshape(-1, 6)
        if aff.shape[0] == 1 and N > 1:
            aff = aff.expand(N, 6)
        if aff.shape[0] != N:
            raise ValueError('affines must hold one 2x3 transform per frame')
    aff = aff.contiguous().to(dev)
    fs = None
    if fscale is not None:
        fs = torch.as_tensor(fscale, dtype=torch.float32).reshape(-1)
        if fs.numel() == 1 and N > 1:
            fs = fs.expand(N)
        if fs.numel() != N:
            raise ValueError('fscale must hold one value per frame')
        fs = fs.contiguous().to(dev)
    mk = _mask_u8(mask, (H, W), 'mask must be [H,W]')
    return frames, N, H, W, h, w, aff, per_tile, fs, mk, lanczos3_table(n_phases, dev)


def resample_affine(frames, affines, fscale=None, mask=None, out_shape=None, n_phases=1024, out=None, weight=True,
                    conserve_flux=False):
    """Affine Lanczos-3 resample of [N,H,W] (or [H,W]) float32 frames onto a common grid.

    affines: [N,6] float64 (tensor / array / nested list): xin = A0*x + A1*y + A2, yin = A3*x + A4*y + A5 maps an
    OUTPUT pixel (x = column, y = row) to INPUT coordinates; or [N, tiles_y, tiles_x, 6] with one transform per
    16 x 64 output tile (wcs.tile_affines: a piecewise-affine TAN -> TAN registration).  fscale: per-frame flux scale (SWarp's FSCALE,
    1/EXPTIME in resample_all.sh:298) or None.  conserve_flux: also scale by the local pixel-area ratio |det A| (SWarp's
    FSCALASTRO_TYPE VARIABLE, resample_all.sh:129).  mask: [H,W] uint8, non-zero = bad pixel, shared by all frames.
    Returns (resampled [N,h,w] float32 with NaN where undefined, weight uint8 [N,h,w] or None).  The co-add is
    stack_median / stack_sigclip on the result (both skip NaN)."""
    frames, N, H, W, h, w, aff, per_tile, fs, mk, lut = _resample_args(frames, affines, fscale, mask, out_shape, n_phases)
    dev = frames.device
    if out is None:
        out = torch.empty((N, h, w), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (N, h, w) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError('out must be a contiguous float32 [N,h,w] tensor')
    wt = torch.empty((N, h, w), dtype=torch.uint8, device=dev) if weight else None
    check(_lib.load().apgpu_resample_affine_f32(_ptr(frames), N, H, W, _ptr(mk) if mk is not None else None, _ptr(aff),
                                                int(per_tile), int(bool(conserve_flux)), _ptr(fs) if fs is not None else None, _ptr(lut), int(n_phases), _ptr(out),
                                                _ptr(wt) if wt is not None else None, h, w, _stream()))
    return out, wt


_fused_ws = {}


def resample_stack_sigclip(frames, affines, fscale=None, mask=None, out_shape=None, n_phases=1024, conserve_flux=False,
                           sigma=3.0, sigma_lower=None, sigma_upper=None, maxiters=5, cenfunc='median', outputs=('mean',),
                           exact=False, moments_mean_only=False):
    """resample_affine + stack_sigclip in ONE launch (apgpu_resample_stack_sigclip): the co-add of registered frames without
    the resampled slab - every output pixel's N Lanczos-3 values go straight into the clip (scripts/resample_all.sh:330-342,
    one SWarp call there).  frames [N <= 16, H, W] float32; affines / fscale / mask / out_shape / n_phases / conserve_flux as
    resample_affine; the clip's arguments as stack_sigclip (stdfunc 'std'); outputs among 'mean', 'count', 'moments',
    'moments_f64', 'moments_f64p'.  Same survivors as the two-step form; the mean within the float32 fast path's rounding."""
    frames, N, H, W, h, w, aff, per_tile, fs, mk, lut = _resample_args(frames, affines, fscale, mask, out_shape, n_phases)
    if N > 16:
        raise ValueError('resample_stack_sigclip takes up to 16 frames per call (resample_affine + stack_sigclip beyond)')
    dev = frames.device
    lib = _lib.load()
    a = StackArgs()
    a.frames = frames.data_ptr()
    a.dtype = _raw_dtype(frames)
    a.n_frames = N
    a.n_pixels = h * w
    a.frame_stride = H * W
    a.center = _lib.CENTER[cenfunc]
    a.dev = _lib.DEV['std']
    a.maxiters = -1 if maxiters is None else int(maxiters)
    a.sigma_lower = float(sigma if sigma_lower is None else sigma_lower)
    a.sigma_upper = float(sigma if sigma_upper is None else sigma_upper)
    shp = (h, w)
    res = {}
    for k in outputs:
        if k == 'mean':
            res[k] = torch.empty(shp, dtype=torch.float32, device=dev)
        elif k == 'count':
            res[k] = torch.empty(shp, dtype=torch.int32, device=dev)
        elif k == 'moments':
            if a.moments:
                raise ValueError('ask for one moment layout')
            res[k] = torch.empty((3,) + shp, dtype=torch.float32, device=dev)
            a.moments = res[k].data_ptr()
            continue
        elif k in ('moments_f64', 'moments_f64p'):
            if a.moments:
                raise ValueError('ask for one moment layout')
            res[k] = alloc_moments_f64(shp, dev, packed=(k == 'moments_f64p'))
            a.moments = res[k]['buffer'].data_ptr()
            a.moments_f64 = 3 if k == 'moments_f64p' else 1
            continue
        else:
            raise ValueError('unknown output %r (mean, count, moments, moments_f64, moments_f64p)' % (k,))
        setattr(a, k, res[k].data_ptr())
    a.flags = (_lib.STACK_EXACT_MOMENTS if exact else 0) | (_lib.STACK_MOMENTS_MEAN if moments_mean_only else 0)
    nb = lib.apgpu_resample_stack_ws_bytes(N, H, W, h, w, int(mk is not None))
    key = (dev.index, int(torch.cuda.current_stream(dev).cuda_stream))
    ws = _fused_ws.get(key)
    if ws is None or ws.numel() < nb:
        ws = torch.empty(nb + 64, dtype=torch.uint8, device=dev)        # (torch allocations are 512-byte aligned)
        _fused_ws[key] = ws
    check(lib.apgpu_resample_stack_sigclip(C.byref(a), H, W, _ptr(mk) if mk is not None else None, _ptr(aff), int(per_tile),
                                           int(bool(conserve_flux)), _ptr(fs) if fs is not None else None, _ptr(lut), int(n_phases),
                                           h, w, _ptr(ws), ws.numel(), _stream()))
    return res


def oversampled_affines(affines, oversampling, out_shape):
    """The transforms of the n-times finer grid whose n x n blocks are the output pixels: fine pixel (u, v) has its centre at
    output coordinates ((u + 0.5) / n - 0.5, (v + 0.5) / n - 0.5).  Single transform per frame only ([N, 6])."""
    n = int(oversampling)
    aff = torch.as_tensor(affines, dtype=torch.float64).reshape(-1, 6).clone()
    off = 0.5 / n - 0.5
    fine = aff.clone()
    fine[:, 0] = aff[:, 0] / n
    fine[:, 1] = aff[:, 1] / n
    fine[:, 2] = aff[:, 2] + (aff[:, 0] + aff[:, 1]) * off
    fine[:, 3] = aff[:, 3] / n
    fine[:, 4] = aff[:, 4] / n
    fine[:, 5] = aff[:, 5] + (aff[:, 3] + aff[:, 4]) * off
    return fine, (int(out_shape[0]) * n, int(out_shape[1]) * n)


def block_mean(fine, oversampling):
    """[n*h, n*w] float32 -> [h, w]: mean of the n x n sub-samples of every output pixel (NaN if any is NaN)."""
    _need_cuda(fine)
    fine = _f32c(fine, 'fine')
    n = int(oversampling)
    hf, wf = fine.shape
    if hf % n or wf % n:
        raise ValueError('the fine grid must be a whole multiple of the oversampling factor')
    out = torch.empty((hf // n, wf // n), dtype=torch.float32, device=fine.device)
    check(_lib.load().apgpu_block_mean_f32(_ptr(fine), hf // n, wf // n, n, _ptr(out), _stream()))
    return out


def _oversampling_args(frames, affines, oversampling, fscale, out_shape, conserve_flux, fine_affines, tile_scale):
    frames = _f32c(frames, 'frames')
    if frames.dim() == 2:
        frames = frames[None]
    N, H, W = frames.shape
    n = int(oversampling)
    if n < 1 or n > 16:
        raise ValueError('oversampling must be 1..16')
    h, w = (H, W) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
    if fine_affines is None:
        fine_aff, _ = oversampled_affines(affines, n, (h, w))
        if fine_aff.shape[0] == 1 and N > 1:
            fine_aff = fine_aff.expand(N, 6)
        if fine_aff.shape[0] != N:
            raise ValueError('affines must hold one 2x3 transform per frame')
    else:
        fine_aff = torch.as_tensor(fine_affines, dtype=torch.float64)
        ty, tx = -(-h * n // (16 * tile_scale)), -(-w * n // (64 * tile_scale))
        if tuple(fine_aff.shape) != (N, ty, tx, 6):
            raise ValueError('per-tile fine affines must be [N, %d, %d, 6] for a %d x %d output at oversampling %d' % (ty, tx, h, w, n))
    fs = torch.ones(N, dtype=torch.float32) if fscale is None else torch.as_tensor(fscale, dtype=torch.float32).reshape(-1).cpu()
    if fs.numel() == 1 and N > 1:
        fs = fs.expand(N)
    if fs.numel() != N:
        raise ValueError('fscale must hold one value per frame')
    # |det| of the fine transform is 1 / n^2 of the output pixel's: the block MEAN of flux-conserving fine values times n^2
    # is the output pixel's value, so the scale goes into the per-frame flux factor
    area = float(n * n) if conserve_flux else 1.0
    return frames, N, H, W, n, h, w, fine_aff, (fs.to(torch.float64) * area).to(torch.float32)


def resample_oversampled(frames, affines, oversampling, fscale=None, mask=None, out_shape=None, n_phases=1024, conserve_flux=False,
                         fine_affines=None):
    """SWarp's OVERSAMPLING n (resample_all.sh:112, 339): every output pixel is the mean of n x n Lanczos-3 interpolations at
    the centres of its sub-pixels, in ONE kernel (apgpu_resample_oversampled_f32: the sub-samples of a pixel are evaluated and
    averaged in registers; the n-times finer image never exists).  `fine_affines`: transforms of the FINE grid per OUTPUT
    tile ([N, ceil(h/16), ceil(w/64), 6], e.g. wcs.tile_affines(fine_wcs, in_wcs, fine_shape, tile_scale=n)) instead of one
    transform per frame.  Returns [N, h, w] float32, NaN where undefined."""
    _need_cuda(frames)
    frames, N, H, W, n, h, w, fine_aff, fs = _oversampling_args(frames, affines, oversampling, fscale, out_shape, conserve_flux,
                                                                 fine_affines, int(oversampling))
    dev = frames.device
    mk = _mask_u8(mask, (H, W), 'mask must be [H,W]')
    fine_aff = fine_aff.contiguous().to(dev)
    fs = fs.contiguous().to(dev)
    lut = lanczos3_table(n_phases, dev)
    out = torch.empty((N, h, w), dtype=torch.float32, device=dev)
    check(_lib.load().apgpu_resample_oversampled_f32(_ptr(frames), N, H, W, _ptr(mk) if mk is not None else None, _ptr(fine_aff),
                                                     int(fine_aff.dim() == 4), int(bool(conserve_flux)), _ptr(fs), _ptr(lut), int(n_phases), n,
                                                     _ptr(out), None, h, w, _stream()))
    return out


def resample_oversampled_two_step(frames, affines, oversampling, fscale=None, mask=None, out_shape=None, n_phases=1024,
                                  conserve_flux=False, fine_affines=None):
    """The two-step form of resample_oversampled (rounds 2-3a): one frame at a time through the n-times finer grid (n^2 x the
    output size in HBM: apgpu_resample_affine_f32), then apgpu_block_mean_f32.  Bit-identical to the fused kernel for one
    transform per frame; kept as its cross-check and for the benchmark.  `fine_affines` here is per tile of the FINE grid."""
    frames, N, H, W, n, h, w, fine_aff, fs = _oversampling_args(frames, affines, oversampling, fscale, out_shape, conserve_flux,
                                                                 fine_affines, 1)
    out = torch.empty((N, h, w), dtype=torch.float32, device=frames.device)
    for i in range(N):
        fine, _ = resample_affine(frames[i:i + 1], fine_aff[i:i + 1], fscale=fs[i:i + 1], mask=mask, out_shape=(h * n, w * n),
                                  n_phases=n_phases, weight=False, conserve_flux=conserve_flux)
        check(_lib.load().apgpu_block_mean_f32(_ptr(fine), h, w, n, _ptr(out[i]), _stream()))
    return out


def weighted_mean(slab, weights):
    """COMBINE_TYPE WEIGHTED with one weight per frame: (sum w_i x_i / sum w_i over the finite x_i, sum of those w_i) per pixel:
    float32 [H, W] each; NaN / 0 where no frame contributes."""
    _need_cuda(slab)
    slab = _f32c(slab, 'slab')
    N = slab.shape[0]
    wts = torch.as_tensor(weights, dtype=torch.float32).reshape(-1).to(slab.device).contiguous()
    if wts.numel() != N:
        raise ValueError('weights must hold one value per frame')
    if not bool(torch.isfinite(wts).all()) or not bool((wts > 0).all()):
        raise ValueError('weights must be finite and positive')
    P = slab[0].numel()
    mean = torch.empty(slab.shape[1:], dtype=torch.float32, device=slab.device)
    wsum = torch.empty_like(mean)
    check(_lib.load().apgpu_weighted_mean_f32(_ptr(slab), N, P, _ptr(wts), _ptr(mean), _ptr(wsum), _stream()))
    return mean, wsum


def background_weights(frames, fscale=None, sigma=3.0, maxiters=5):
    """SWarp's weights without weight maps (WEIGHT_TYPE NONE): a frame counts with the inverse variance of its flux-scaled
    background noise, w_i = 1 / (fscale_i * sigma_i)^2.  sigma_i here = the sigma-clipped standard deviation of the whole
    frame (the A3 kernels); SWarp measures it on its own background mesh.  Returns float64 numpy [N]."""
    import numpy as np
    N = frames.shape[0]
    fs = np.ones(N) if fscale is None else np.broadcast_to(np.asarray(fscale, dtype=np.float64).reshape(-1), (N,))
    sd = np.array([float(sigclip_global(frames[i], sigma=sigma, maxiters=maxiters)[2].item()) for i in range(N)])
    if not np.all(np.isfinite(sd)) or np.any(sd <= 0):
        raise ValueError('a frame has no measurable background noise (constant or empty): give explicit weights')
    return 1.0 / (fs * sd) ** 2


COADD_COMBINE = ('MEDIAN', 'AVERAGE', 'WEIGHTED', 'SUM', 'CLIPPED', 'WINSORIZED', 'MINMAX', 'ESD')
COADD_REJECT = ('WINSORIZED', 'MINMAX', 'ESD')                 # the rules of stack_reject: normalize, weighting and norm_box go with them


def coadd(frames, affines, fscale=None, mask=None, out_shape=None, combine='MEDIAN', sigma=3.0, maxiters=5, n_phases=1024,
          conserve_flux=False, oversampling=1, weights=None, fine_affines=None, fused=False, nlow=1, nhigh=1,
          normalize='none', reference=0, weighting=None, norm_box=None, esd_outliers=0.3, esd_significance=0.05,
          esd_low_relaxation=1.5):
    """Resample + combine: SWarp's COMBINE_TYPE MEDIAN / AVERAGE / WEIGHTED / SUM (resample_all.sh:60-73 add modes) plus
    CLIPPED (sigma-clipped mean, median-centred), WINSORIZED (Winsorized sigma clip at `sigma`, `maxiters` rounds) and MINMAX
    (the nlow lowest and nhigh highest values of a pixel dropped) - the two rules for stacks of few frames (stack_reject; up to
    128 frames; fused does not apply) - and ESD, the generalized ESD test for a couple of dozen frames and more (esd_outliers,
    esd_significance, esd_low_relaxation: stack_reject; normalize, weighting and norm_box go with it as with WINSORIZED);
    oversampling = SWarp's OVERSAMPLING.  WEIGHTED takes one weight per frame
    (default: background_weights).  Returns dict(image, count[, weight]) - count = frames contributing, weight = the sum
    of their weights (WEIGHTED only).
    fused=True (CLIPPED / AVERAGE, up to 16 frames, oversampling 1): one launch, no [N, h, w] slab of resampled frames in
    memory (resample_stack_sigclip: same survivors; 6.2 against 5.1 ms for C5's share on one MI355X, but 4 N h w bytes less HBM -
    DESIGN 4.4d).
    normalize ('none', 'additive', 'multiplicative', 'additive+scaling'; frame_normalization) brings the resampled frames to
    the level of frame `reference` before they are combined: the statistics (frame_stats) are taken on the resampled slab -
    those are the values that get compared.  WINSORIZED / MINMAX apply v = a x + b inside the kernel (stack_reject) and take
    weighting='noise' (the survivors' mean weighted by 1 / (a S)^2); the other modes get the same float32 map on the slab
    in place and take no weighting (WEIGHTED has `weights`).  The result then also holds scale, offset and norm_weights
    (float64 numpy [N]).
    norm_box (an int or (bh, bw); WINSORIZED / MINMAX only): the LOCAL normalisation - the statistics are taken per box of the
    resampled slab (local_stats), scale and offset are meshes interpolated at every pixel inside the kernel
    (local_normalization, stack_reject(box=)): for frames whose sky differs in shape, not only in level.  The result then holds
    the meshes as scale (None without a scaling mode) and offset (float32 numpy [N, ny, nx]), norm_weights and norm_box."""
    combine = combine.upper()
    if combine not in COADD_COMBINE:
        raise ValueError('combine must be one of ' + ', '.join(COADD_COMBINE))
    if normalize is None:
        normalize = 'none'
    if weighting == 'none':
        weighting = None
    if normalize not in NORMALIZE_MODES:
        raise ValueError('normalize must be one of ' + ', '.join(NORMALIZE_MODES) + ', not %r' % (normalize,))
    if weighting not in (None, 'noise'):
        raise ValueError("weighting must be None or 'noise', not %r" % (weighting,))
    if weighting is not None and combine not in COADD_REJECT:
        raise ValueError('weighting goes with combine WINSORIZED and MINMAX only (WEIGHTED takes weights), not with %s' % combine)
    normed = normalize != 'none' or weighting is not None
    if norm_box is not None:
        norm_box = _box_pair(norm_box)
        if combine not in COADD_REJECT:
            raise ValueError('norm_box (the local normalisation) goes with combine WINSORIZED and MINMAX only, not with %s '
                             '(MINMAX with nlow = nhigh = 0 is the normalised, weighted average)' % combine)
        normed = True
    if fused and normed:
        raise ValueError('fused=True does not go with a normalisation: the statistics are taken on the resampled slab')
    if combine in COADD_REJECT and frames.dim() == 3 and frames.shape[0] > _lib.STACK_REJECT_MAX:
        raise ValueError('combine %s takes at most %d frames (STACK_REJECT_MAX), got %d' % (combine, _lib.STACK_REJECT_MAX, frames.shape[0]))
    if fused and int(oversampling) == 1 and combine in ('CLIPPED', 'AVERAGE') and frames.dim() == 3 and frames.shape[0] <= 16:
        kw = dict(sigma=sigma, maxiters=maxiters) if combine == 'CLIPPED' else dict(sigma=1e30, maxiters=1, cenfunc='mean')
        r = resample_stack_sigclip(frames, affines, fscale=fscale, mask=mask, out_shape=out_shape, n_phases=n_phases,
                                   conserve_flux=conserve_flux, outputs=('mean', 'count'), **kw)
        return dict(image=r['mean'], count=r['count'])
    if int(oversampling) > 1:
        res = resample_oversampled(frames, affines, oversampling, fscale=fscale, mask=mask, out_shape=out_shape, n_phases=n_phases,
                                   conserve_flux=conserve_flux, fine_affines=fine_affines)
    else:
        res, _ = resample_affine(frames, affines, fscale=fscale, mask=mask, out_shape=out_shape, n_phases=n_phases, weight=False,
                                 conserve_flux=conserve_flux)
    rule_kw = {'WINSORIZED': dict(sigma=sigma, maxiters=maxiters), 'MINMAX': dict(nlow=nlow, nhigh=nhigh),
               'ESD': dict(esd_outliers=esd_outliers, esd_significance=esd_significance, esd_low_relaxation=esd_low_relaxation)}.get(combine)
    if combine == 'ESD' and not normed:
        r = stack_reject(res, 'esd', outputs=('mean', 'count'), **rule_kw)
        return dict(image=r['mean'], count=r['count'])
    if norm_box is not None:
        if res.dim() != 3:
            raise ValueError('norm_box needs frames [N, H, W]')
        a, b, w = local_normalization(local_stats(res, norm_box, sigma=3.0, maxiters=5), normalize, reference=reference,
                                      weighting=weighting, box=norm_box)
        r = stack_reject(res, combine.lower(), outputs=('mean', 'count'), scale=a, offset=b, weights=w, box=norm_box, **rule_kw)
        return dict(image=r['mean'], count=r['count'], scale=a, offset=b, norm_weights=w, norm_box=norm_box)
    if normed:
        a, b, w = frame_normalization(frame_stats(res, sigma=3.0, maxiters=5), normalize, reference=reference, weighting=weighting)
        extra = dict(scale=a, offset=b, norm_weights=w)
        if combine in COADD_REJECT:
            r = stack_reject(res, combine.lower(), outputs=('mean', 'count'), scale=a, offset=b, weights=w, **rule_kw)
            return dict(image=r['mean'], count=r['count'], **extra)
        # the other rules: the same float32 map on the slab in place - multiply, then add: two roundings
        bc = (res.shape[0],) + (1,) * (res.dim() - 1)
        res.mul_(torch.from_numpy(a.astype(np.float32)).to(res.device).reshape(bc))
        res.add_(torch.from_numpy(b.astype(np.float32)).to(res.device).reshape(bc))
        r = _coadd_combine(res, combine, sigma, maxiters, weights, frames, fscale, nlow, nhigh)
        r.update(extra)
        return r
    return _coadd_combine(res, combine, sigma, maxiters, weights, frames, fscale, nlow, nhigh)


def _coadd_combine(res, combine, sigma, maxiters, weights, frames, fscale, nlow, nhigh):
    """The combine step of coadd on a resampled slab."""
    if combine == 'MEDIAN':
        med, cnt = stack_median(res, want_count=True)
        return dict(image=med, count=cnt)
    if combine == 'WEIGHTED':
        if weights is None:
            fr = frames if frames.dim() == 3 else frames[None]
            weights = background_weights(fr, fscale)
        mean, wsum = weighted_mean(res, weights)
        cnt = stack_sigclip(res, sigma=1e30, maxiters=1, cenfunc='mean', outputs=('count',))['count']
        return dict(image=mean, count=cnt, weight=wsum)
    if combine in ('AVERAGE', 'SUM'):
        # one pass with bounds nothing can exceed = np.nanmean / np.nansum along N
        r = stack_sigclip(res, sigma=1e30, maxiters=1, cenfunc='mean',
                          outputs=('mean', 'count') if combine != 'SUM' else ('moments', 'count'))
        if combine == 'SUM':
            return dict(image=r['moments'][0], count=r['count'])
        return dict(image=r['mean'], count=r['count'])
    if combine == 'CLIPPED':
        r = stack_sigclip(res, sigma=sigma, maxiters=maxiters, outputs=('mean', 'count'))
        return dict(image=r['mean'], count=r['count'])
    if combine == 'WINSORIZED':
        r = stack_reject(res, 'winsorized', sigma=sigma, maxiters=maxiters, outputs=('mean', 'count'))
    else:
        r = stack_reject(res, 'minmax', nlow=nlow, nhigh=nhigh, outputs=('mean', 'count'))
    return dict(image=r['mean'], count=r['count'])


# ---------------------------------------------------------------------------------------------------
# F4: sky-background mesh (core/ApMeasureBackground.py:142-175, 382-415; photutils restated, parity unpinned)
# ---------------------------------------------------------------------------------------------------
def source_mask(above, min_pixels=5, dilate_size=13):
    """detect_sources(npixels=min_pixels, 8-connectivity) + make_source_mask(size=dilate_size) on a uint8 map of the pixels
    above the detection threshold.  Returns (mask uint8 [H,W], nsources int64[1] device tensor)."""
    _need_cuda(above)
    if above.dtype != torch.uint8 or above.dim() != 2:
        raise TypeError('above must be a 2-D uint8 tensor')
    above = above.contiguous()
    lib = _lib.load()
    H, W = above.shape
    ws_bytes = lib.apgpu_source_mask_ws_bytes(H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=above.device)
    out = torch.empty_like(above)
    nsrc = torch.empty(1, dtype=torch.int64, device=above.device)
    check(lib.apgpu_source_mask_u8(_ptr(above), H, W, int(min_pixels), int(dilate_size), _ptr(out), _ptr(nsrc), _ptr(ws), ws_bytes,
                                   _stream()))
    return out, nsrc


def box_clipped_stats(data, mask, box_height, box_width, sigma=3.0, maxiters=5):
    """Background2D's per-box SigmaClip(sigma, maxiters) + median / std: float64 device tensor [ny, nx, 4] =
    median, std, survivors, pixels masked before clipping (boxes sticking out of the image are padded with masked pixels)."""
    _need_cuda(data, mask)
    data = _f32c(data, 'data')
    if data.dim() != 2:
        raise ValueError('data must be 2-D')
    if mask is not None:
        if mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(data.shape):
            raise TypeError('mask must be uint8 with the image shape')
        mask = mask.contiguous()
    H, W = data.shape
    ny, nx = -(-H // int(box_height)), -(-W // int(box_width))
    out = torch.empty((ny, nx, 4), dtype=torch.float64, device=data.device)
    check(_lib.load().apgpu_box_clipped_stats_f32(_ptr(data), _ptr(mask), H, W, int(box_height), int(box_width), float(sigma),
                                                  int(maxiters), _ptr(out), _stream()))
    return out


def spline_zoom(coef, zoom_y, zoom_x, height, width, vmin, vmax):
    """scipy.ndimage.zoom(mesh, (zoom_y, zoom_x), order=3, mode='reflect', grid_mode=True)[:height, :width] from prefiltered
    B-spline coefficients coef [ny, nx] (float64 device tensor), clipped to [vmin, vmax]; float64 [height, width]."""
    _need_cuda(coef)
    if coef.dtype != torch.float64 or coef.dim() != 2:
        raise TypeError('coef must be a 2-D float64 tensor')
    coef = coef.contiguous()
    ny, nx = coef.shape
    out = torch.empty((int(height), int(width)), dtype=torch.float64, device=coef.device)
    check(_lib.load().apgpu_spline_zoom_f64(_ptr(coef), ny, nx, int(zoom_y), int(zoom_x), int(height), int(width), float(vmin),
                                            float(vmax), _ptr(out), _stream()))
    return out


# ---------------------------------------------------------------------------------------------------
# F4: L.A.Cosmic (core/ApFixCosmicRays.py:267-295 -> ccdproc -> astroscrappy; restated, parity unpinned)
# ---------------------------------------------------------------------------------------------------
def sepmedfilt(data, size):
    """astroscrappy's separable median filter: median of `size` (5, 7, 9) along rows, then along columns, borders copied."""
    _need_cuda(data)
    data = _f32c(data, 'data')
    out = torch.empty_like(data)
    ws = torch.empty(data.numel() * 4, dtype=torch.uint8, device=data.device)
    check(_lib.load().apgpu_sepmedfilt_f32(_ptr(data), data.shape[0], data.shape[1], int(size), _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def gauss_psf_kernel(fwhm, size=7, device='cuda'):
    """astroscrappy's gausskernel(psffwhm, kernsize): normalised float32 Gaussian, [size, size] device tensor."""
    x = np.tile(np.arange(size) - size // 2, (size, 1)).astype(np.float64)
    y = x.T.copy()
    sigma2 = fwhm * fwhm / 2.35482 / 2.35482
    k = np.exp(-0.5 * (x * x + y * y) / sigma2).astype(np.float32)
    return torch.from_numpy((k / k.sum()).astype(np.float32)).to(device)


def lacosmic(data_electrons, inmask=None, sigclip=4.5, sigfrac=0.3, objlim=5.0, readnoise=12.0, satlevel=65535.0, niter=6,
             psffwhm=3.5, fsmode='convolve'):
    """astroscrappy.detect_cosmics on a float32 image in electrons (device tensor): returns (cleaned float32 tensor,
    crmask uint8 tensor, iterations run).  Non-finite pixels must have been zeroed and put into inmask by the caller.
    One host read of the per-iteration cosmic-ray count decides whether to go on (astroscrappy stops at 0)."""
    _need_cuda(data_electrons, inmask)
    lib = _lib.load()
    clean = _f32c(data_electrons, 'data').clone()
    H, W = clean.shape
    if inmask is not None and (inmask.dtype != torch.uint8 or tuple(inmask.shape) != (H, W)):
        raise TypeError('inmask must be uint8 with the image shape')
    ws_bytes = lib.apgpu_lacosmic_ws_bytes(H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=clean.device)
    mask = torch.empty((H, W), dtype=torch.uint8, device=clean.device)
    check(lib.apgpu_lacosmic_satmask(_ptr(clean), _ptr(inmask.contiguous()) if inmask is not None else None, H, W, float(satlevel),
                                     _ptr(mask), _ptr(ws), ws_bytes, _stream()))
    # background level for cosmic rays without a good neighbour: np.median of the unmasked pixels (A3 kernels, no clipping)
    masked = torch.where(mask != 0, torch.full_like(clean, float('nan')), clean)
    bkg = float(sigclip_global(masked, sigma=1e30, maxiters=1)[1].item())
    if bkg != bkg:
        bkg = 0.0
    psfk = gauss_psf_kernel(psffwhm, 7, clean.device) if fsmode == 'convolve' else None
    crmask = torch.zeros((H, W), dtype=torch.uint8, device=clean.device)
    ncr = torch.zeros(1, dtype=torch.int64, device=clean.device)
    it = 0
    for it in range(1, int(niter) + 1):
        check(lib.apgpu_lacosmic_iterate(_ptr(clean), _ptr(mask), _ptr(crmask), H, W, float(sigclip), float(sigfrac), float(objlim),
                                         float(readnoise), _ptr(psfk), bkg, _ptr(ncr), _ptr(ws), ws_bytes, _stream()))
        if int(ncr.item()) == 0:
            break
    return clean, crmask, it


# ---------------------------------------------------------------------------------------------------
# F6: star finding (core/ApFindStars.py:299-340, 363-446; photutils' DAOStarFinder / find_peaks / aperture_photometry
# restated in tests/findstars_model.py, parity unpinned)
# ---------------------------------------------------------------------------------------------------
DAOFIND_RECORD = ('x_peak', 'y_peak', 'npix', 'peak', 'conv_peak', 'sharpness', 'roundness1', 'roundness2', 'dx', 'dy', 'hx', 'hy',
                  'xcentroid', 'ycentroid', 'flux', 'mag')
DAOFIND_MAX_RADIUS = 12


def daofind_kernel(fwhm, device=None):
    """The zero-sum DAOFIND kernel for a circular Gaussian of the given FWHM (sigma_radius 1.5, photutils' defaults) and
    the constants of the marginal fits, built in float64 on the host.

    dict(fwhm, sigma, R, K [2R+1, 2R+1] float64, fp bool footprint, npixels, relerr, p, consts{x, y}, tables [6, (2R+1)^2],
    quad [2R+1, 2R+1]); with `device` also dev = dict(K, fp (uint8), tables, quad) of device tensors."""
    import math
    fwhm = float(fwhm)
    if not fwhm > 0:
        raise ValueError('fwhm must be positive, got %r' % (fwhm,))
    sigma = fwhm / (2.0 * math.sqrt(2.0 * math.log(2.0)))
    R = max(2, int(1.5 * sigma))
    ax = np.arange(-R, R + 1, dtype=np.float64)
    r2 = ax[:, None] ** 2 + ax[None, :] ** 2
    g = np.exp(-r2 / (2.0 * sigma * sigma))
    fp = (g >= math.exp(-1.5 * 1.5 / 2.0)) | (r2 <= 4.0)
    npixels = int(fp.sum())
    gm = g * fp
    s1 = float(gm.sum())
    denom = float((gm * gm).sum()) - s1 * s1 / npixels
    K = ((gm - s1 / npixels) / denom) * fp
    n = 2 * R + 1
    # DAOFIND's triangular weights: 1 at the edge of the box, R + 1 in the middle
    w = R - np.abs(np.arange(n, dtype=np.float64) - R) + 1.0
    vec = R - np.arange(n, dtype=np.float64)
    ww = w[:, None] * w[None, :]
    tables = np.zeros((6, n, n), np.float64)
    tables[0] = fp
    tables[1] = ww
    consts = {}
    for axis, qg, qd in (('x', 2, 3), ('y', 4, 5)):
        sg = (g * w[:, None]).sum(axis=0) if axis == 'x' else (g * w[None, :]).sum(axis=1)
        dg = sg * vec
        consts[axis] = dict(sumg=float((w * sg).sum()), sumgsq=float((w * sg * sg).sum()), sdgd=float((w * dg).sum()),
                            sdgds=float((w * dg * dg).sum()), sgdgd=float((w * sg * dg).sum()))
        tables[qg] = ww * (sg[None, :] if axis == 'x' else sg[:, None])
        tables[qd] = ww * (dg[None, :] if axis == 'x' else dg[:, None])
    quad = np.zeros((n, n), np.float64)
    quad[0:R + 1, R + 1:] = -1.0
    quad[0:R, 0:R + 1] = 1.0
    quad[R:, 0:R] = -1.0
    quad[R + 1:, R:] = 1.0
    k = dict(fwhm=fwhm, sigma=sigma, R=R, K=K, fp=fp, npixels=npixels, relerr=1.0 / math.sqrt(denom), p=float(w.sum()), consts=consts,
             tables=tables.reshape(6, n * n), quad=quad)
    if device is not None:
        k['dev'] = dict(K=torch.from_numpy(np.ascontiguousarray(K)).to(device),
                        fp=torch.from_numpy(np.ascontiguousarray(fp.astype(np.uint8))).to(device),
                        tables=torch.from_numpy(np.ascontiguousarray(k['tables'])).to(device),
                        quad=torch.from_numpy(np.ascontiguousarray(quad)).to(device))
    return k


def _kernel_on(kernel, device):
    if 'dev' not in kernel or kernel['dev']['K'].device != device:
        kernel = dict(kernel)
        kernel['dev'] = dict(K=torch.from_numpy(np.ascontiguousarray(kernel['K'])).to(device),
                             fp=torch.from_numpy(np.ascontiguousarray(np.asarray(kernel['fp']).astype(np.uint8))).to(device),
                             tables=torch.from_numpy(np.ascontiguousarray(kernel['tables'])).to(device),
                             quad=torch.from_numpy(np.ascontiguousarray(kernel['quad'])).to(device))
    return kernel


def daofind_convolve(data, kernel, bg_median=0.0):
    """float32 image [H, W] -> the image convolved with the DAOFIND kernel (daofind_kernel(fwhm) or a fwhm), float32:
    d = data - float32(bg_median) inside the image, 0 outside; float64 accumulation over all taps in row-major tap order."""
    data = _image_f32(data)
    if not isinstance(kernel, dict):
        kernel = daofind_kernel(kernel)
    kernel = _kernel_on(kernel, data.device)
    out = torch.empty_like(data)
    check(_lib.load().apgpu_daofind_convolve_f32(_ptr(data), data.shape[0], data.shape[1], _ptr(kernel['dev']['K']), kernel['R'],
                                                 float(np.float32(bg_median)), _ptr(out), _stream()))
    return out


def local_peaks(values, footprint, threshold, mask=None, border=0, capacity=4096, list_out=None):
    """Local maxima of a float32 plane under a footprint (2-D bool / uint8 array or tensor; an int n = the n x n square of
    photutils' find_peaks(box_size=n)): no footprint pixel exceeds the value (outside the image counts as 0), value >
    threshold (strict), mask == 0, at least `border` pixels from every edge.

    Returns (idx, count): idx = int32 device tensor of flat indices sorted ascending, count = the true number of peaks (python
    int; one host read).  With count > capacity the list was too short and holds `capacity` of the peaks: call again with
    capacity=count (find_stars does).  list_out: a caller-owned int32 tensor of at least `capacity` entries to write into."""
    values = _image_f32(values, 'values')
    dev = values.device
    if isinstance(footprint, (int, np.integer)):
        footprint = np.ones((int(footprint), int(footprint)), np.uint8)
    if torch.is_tensor(footprint):
        fp = (footprint != 0).to(device=dev, dtype=torch.uint8).contiguous()
    else:
        fp = torch.from_numpy(np.ascontiguousarray((np.asarray(footprint) != 0).astype(np.uint8))).to(dev)
    if fp.dim() != 2:
        raise ValueError('footprint must be 2-D')
    mask = _mask_u8(mask, values.shape, 'mask must have the image shape')
    capacity = int(capacity)
    if list_out is None:
        list_out = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev)
    elif list_out.dtype != torch.int32 or list_out.numel() < capacity or not list_out.is_contiguous():
        raise TypeError('list_out must be a contiguous int32 tensor of at least `capacity` entries')
    count = torch.empty(1, dtype=torch.int32, device=dev)
    check(_lib.load().apgpu_local_peaks_f32(_ptr(values), values.shape[0], values.shape[1], _ptr(fp), fp.shape[0], fp.shape[1],
                                            float(threshold), _ptr(mask), int(border), _ptr(list_out), capacity, _ptr(count), _stream()))
    n = int(count.item())
    idx = torch.sort(list_out[:min(n, capacity)]).values          # order does not depend on scheduling
    return idx, n


def daofind_measure(data, conv, idx, kernel, threshold_eff, bg_median=0.0, sharplo=0.2, sharphi=1.0, roundlo=-1.0, roundhi=1.0):
    """The DAOFIND quantities of every candidate (int32 flat indices from local_peaks with border = kernel radius).
    Returns (records float64 [n, 16] in DAOFIND_RECORD order, keep uint8 [n]) as device tensors."""
    data = _image_f32(data)
    conv = _image_f32(conv, 'conv')
    if conv.shape != data.shape:
        raise ValueError('conv must have the image shape')
    kernel = _kernel_on(kernel, data.device)
    idx = idx.to(device=data.device, dtype=torch.int32).contiguous()
    n = idx.numel()
    rec = torch.empty((n, len(DAOFIND_RECORD)), dtype=torch.float64, device=data.device)
    keep = torch.empty(n, dtype=torch.uint8, device=data.device)
    if n == 0:
        return rec, keep
    cx, cy = kernel['consts']['x'], kernel['consts']['y']
    consts = [kernel['npixels'] - 1.0, float(threshold_eff), sharplo, sharphi, roundlo, roundhi, kernel['sigma'] * kernel['sigma'],
              kernel['p']]
    for c in (cx, cy):
        consts += [c['sumg'], c['sumgsq'], c['sdgd'], c['sdgds'], c['sgdgd']]
    cd = torch.tensor(consts, dtype=torch.float64).to(data.device)
    d = kernel['dev']
    check(_lib.load().apgpu_daofind_measure(_ptr(data), _ptr(conv), data.shape[0], data.shape[1], _ptr(idx), n, kernel['R'],
                                            float(np.float32(bg_median)), _ptr(d['tables']), _ptr(d['quad']), _ptr(cd), _ptr(rec),
                                            _ptr(keep), _stream()))
    return rec, keep


def aperture_radii(fwhm):
    """(aperture radius, annulus inner, annulus outer) of ApFindStars._make_apertures (:272-297)."""
    import math
    r = math.ceil(2.0 * float(fwhm))
    return float(r), float(r), float(math.ceil(1.5 * r))


def aperture_photometry(data, xc, yc, fwhm=None, radii=None, sigma=3.0, maxiters=5):
    """Circular-aperture sums with exact pixel overlaps and the sigma-clipped median of the background annulus
    (ApFindStars.aperture_photometry, :363-400) for sources at (xc, yc) (x = column; sequences or tensors).

    Returns dict(aperture_sum_raw float64, bkg_median float32, n_annulus int32, area float64, aperture_sum float64 =
    raw - bkg_median * pi r^2) of device tensors [n]."""
    import math
    data = _image_f32(data)
    dev = data.device
    r, r_in, r_out = aperture_radii(fwhm) if radii is None else (float(x) for x in radii)
    xc = torch.as_tensor(xc, dtype=torch.float64).reshape(-1).to(dev).contiguous()
    yc = torch.as_tensor(yc, dtype=torch.float64).reshape(-1).to(dev).contiguous()
    if xc.numel() != yc.numel():
        raise ValueError('xc and yc must have the same length')
    n = xc.numel()
    out = dict(aperture_sum_raw=torch.empty(n, dtype=torch.float64, device=dev), bkg_median=torch.empty(n, dtype=torch.float32, device=dev),
               n_annulus=torch.empty(n, dtype=torch.int32, device=dev), area=torch.empty(n, dtype=torch.float64, device=dev))
    check(_lib.load().apgpu_aperture_phot_f32(_ptr(data), data.shape[0], data.shape[1], _ptr(xc), _ptr(yc), n, r, r_in, r_out,
                                              float(sigma), -1 if maxiters is None else int(maxiters), _ptr(out['aperture_sum_raw']),
                                              _ptr(out['bkg_median']), _ptr(out['n_annulus']), _ptr(out['area']), _stream()))
    out['aperture_sum'] = out['aperture_sum_raw'] - out['bkg_median'].double() * (math.pi * r * r)
    return out


def find_stars(data, fwhm, threshold, bg_median=0.0, mask=None, capacity=4096):
    """DAOStarFinder(fwhm, threshold)(data - bg_median, mask) with photutils' defaults (ApFindStars.source_search, :299-340):
    convolution, peaks, measurement and the rejection rules on the device.  The mask only excludes peaks.

    Returns a dict of device tensors, one entry per kept source ordered by flat pixel index: the DAOFIND_RECORD columns
    (float64), idx (int32 flat index of the peak), plus n_candidates (python int) and conv (the convolved image).  If the
    image holds more peaks than `capacity` the peak search is repeated once with a list of the right size."""
    data = _image_f32(data)
    kernel = daofind_kernel(fwhm, device=data.device)
    if kernel['R'] > DAOFIND_MAX_RADIUS:
        raise ValueError('fwhm = %g needs a kernel radius of %d, the kernels hold %d' % (fwhm, kernel['R'], DAOFIND_MAX_RADIUS))
    thr_eff = float(threshold) * kernel['relerr']
    conv = daofind_convolve(data, kernel, bg_median)
    idx, n = local_peaks(conv, kernel['dev']['fp'], thr_eff, mask=mask, border=kernel['R'], capacity=capacity)
    if n > capacity:
        idx, n = local_peaks(conv, kernel['dev']['fp'], thr_eff, mask=mask, border=kernel['R'], capacity=n)
    rec, keep = daofind_measure(data, conv, idx, kernel, thr_eff, bg_median)
    sel = keep != 0
    rec = rec[sel]
    out = {name: rec[:, c].contiguous() for c, name in enumerate(DAOFIND_RECORD)}
    out.update(idx=idx[sel], n_candidates=n, conv=conv, threshold_eff=thr_eff, kernel=kernel)
    return out


# ------------------------------------------------------------------------------------------------------------------
# F7: ApMeasureStars - Gaussian PSF fits (csrc/measurestars.hip)
SIGMA_TO_FWHM = 2.35482                                     # the reference's constant (ApMeasureStars.py:245)
GAUSS2D_COLUMNS = ('xc_fit', 'xc_err', 'yc_fit', 'yc_err', 'ampl', 'ampl_err', 'fwhm_x', 'fwhm_x_err', 'fwhm_y', 'fwhm_y_err', 'theta',
                   'theta_err', 'axrat', 'axrat_err', 'circular', 'fit_ok', 'rchisq')


def fit_box_width(init_fwhm):
    """(box width, edge exclusion) of ApMeasureStars._fit_box_initialization (:526-534)."""
    import math
    box = max(2 * int(3.0 * init_fwhm), 12)
    return box, 2 * int(math.ceil(box / 4))


def gauss2d_fit(data, xcenter, ycenter, peak, bg, init_fwhm, box_width=None, max_iter=500):
    """The three-stage 2-D Gaussian + constant fits of ApMeasureStars._do_fitting (:223-430) for stars at (xcenter, ycenter)
    (x = column) with starting amplitudes `peak` and background levels `bg` (sequences, or one number for bg), one wavefront per
    star.  The box of a star is [rint(centre) - box_width / 2, + box_width / 2) per axis and must lie inside the image.

    Returns a dict of float64 NumPy columns named as the reference's table (GAUSS2D_COLUMNS; circular and fit_ok are bool) plus
    bg_fit, niter [n, 3] (int64) and xmin / xmax / ymin / ymax.  The reference's axes are kept: the model's x runs along the
    ROWS of the cut-out, yet xc_fit = x_mean + xmin.  Error columns, axrat_err and circular (True) stay at their defaults where
    fit_ok is False."""
    import math
    import numpy as np
    data = _image_f32(data)
    dev = data.device
    H, W = int(data.shape[0]), int(data.shape[1])
    xcenter = np.atleast_1d(np.asarray(xcenter, np.float64)).reshape(-1)
    ycenter = np.atleast_1d(np.asarray(ycenter, np.float64)).reshape(-1)
    n = xcenter.size
    peak = np.broadcast_to(np.asarray(peak, np.float64).reshape(-1), (n,)) if n else np.zeros(0)
    bg = np.broadcast_to(np.asarray(bg, np.float64).reshape(-1), (n,)) if n else np.zeros(0)
    if ycenter.size != n:
        raise ValueError('xcenter and ycenter must have the same length')
    Wb = fit_box_width(init_fwhm)[0] if box_width is None else int(box_width)
    half = Wb / 2
    nx, ny = np.rint(xcenter).astype(np.int64), np.rint(ycenter).astype(np.int64)
    out = {'xmin': nx - half, 'xmax': nx + half, 'ymin': ny - half, 'ymax': ny + half}
    if n and Wb % 2 == 0 and (out['xmin'].min() < 0 or out['ymin'].min() < 0 or out['xmax'].max() > W or out['ymax'].max() > H):
        raise ValueError('gauss2d_fit: a %d-pixel fit box lies outside the [%d, %d] image' % (Wb, H, W))
    sig_y = float(init_fwhm) * (1.0 / SIGMA_TO_FWHM)
    init = np.empty((n, 7))
    init[:, 0], init[:, 1], init[:, 2], init[:, 3], init[:, 4] = peak, 1.05 * sig_y, sig_y, 1.1, bg
    init[:, 5], init[:, 6] = xcenter - out['xmin'], ycenter - out['ymin']
    box_y = torch.from_numpy(out['ymin'].astype(np.int32)).to(dev)
    box_x = torch.from_numpy(out['xmin'].astype(np.int32)).to(dev)
    init_t = torch.from_numpy(init).to(dev).contiguous()
    rec_t = torch.zeros((n, _lib.GAUSS2D_REC), dtype=torch.float64, device=dev)
    ok_t = torch.zeros(n, dtype=torch.int32, device=dev)
    check(_lib.load().apgpu_gauss2d_fit_f32(_ptr(data), H, W, _ptr(box_y), _ptr(box_x), _ptr(init_t), n, Wb, int(max_iter), _ptr(rec_t),
                                            _ptr(ok_t), _stream()))
    rec, okf = rec_t.cpu().numpy(), ok_t.cpu().numpy()
    if (okf < 0).any():
        raise ValueError('gauss2d_fit: a fit box lies outside the image')
    ok = okf == 1
    fx, fy = SIGMA_TO_FWHM * rec[:, 1], SIGMA_TO_FWHM * rec[:, 2]
    fxe, fye = np.where(ok, SIGMA_TO_FWHM * rec[:, 8], 0.0), np.where(ok, SIGMA_TO_FWHM * rec[:, 9], 0.0)
    with np.errstate(all='ignore'):
        axrat = np.maximum(fx, fy) / np.minimum(fx, fy)
        axrat_err = np.where(ok, axrat * np.sqrt((fxe / fx) ** 2 + (fye / fy) ** 2), 0.0)
        circular = ~(ok & (np.abs(fy - fx) / fye > 3.0))                  # is_circular (:433-445): fwhm_yerr only
    out.update(xc_fit=rec[:, 5] + out['xmin'], xc_err=np.where(ok, rec[:, 12], 0.0), yc_fit=rec[:, 6] + out['ymin'],
               yc_err=np.where(ok, rec[:, 13], 0.0), ampl=rec[:, 0].copy(), ampl_err=np.where(ok, rec[:, 7], 0.0), fwhm_x=fx,
               fwhm_x_err=fxe, fwhm_y=fy, fwhm_y_err=fye, theta=rec[:, 3].copy(), theta_err=np.where(ok, rec[:, 10], 0.0), axrat=axrat,
               axrat_err=axrat_err, circular=circular, fit_ok=ok, rchisq=rec[:, 14].copy(), bg_fit=rec[:, 4].copy(),
               bg_err=np.where(ok, rec[:, 11], 0.0), niter=rec[:, 16:19].astype(np.int64))
    return out


# ------------------------------------------------------------------------------------------------------------------
# F8: ApRegister - star-list registration by triangle similarity (csrc/register.hip)
REGISTER_IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _star_lists(xy, count):
    xy = torch.as_tensor(xy, dtype=torch.float64)
    if xy.dim() != 3 or xy.shape[2] != 2 or xy.shape[1] < 1:
        raise ValueError('xy must be [frames, stars >= 1, 2], got %s' % (tuple(xy.shape),))
    count = torch.as_tensor(count, dtype=torch.int32).reshape(-1)
    if count.numel() != xy.shape[0]:
        raise ValueError('count must hold one entry per frame')
    dev = xy.device if xy.is_cuda else torch.device('cuda')
    return xy.to(dev).contiguous(), count.to(dev).contiguous()


def triangle_build(xy, count, K=40, min_side=5.0):
    """The similarity invariants of every triangle among the K brightest stars of each list (xy [F, M, 2] float64, x = column,
    brightest first; count [F]).  A triangle is kept iff its shortest side is >= min_side, y >= 0.1, x <= 0.98 and y <= 0.98 x.

    Returns dict(xy float64 [F, T, 2] = (sqrt(b2 / a2), sqrt(c2 / a2)), v int32 [F, T] = v0 | v1 << 8 | v2 << 16 | (orientation
    + 1) << 24, count int32 [F], K) of device tensors, T = K (K-1) (K-2) / 6; a frame's list is in no particular order
    (triangle_unpack sorts it)."""
    K = int(K)
    if not 3 <= K <= _lib.REGISTER_MAX_K:
        raise ValueError('K = %d is outside 3 .. %d' % (K, _lib.REGISTER_MAX_K))
    xy, count = _star_lists(xy, count)
    F, M = int(xy.shape[0]), int(xy.shape[1])
    T = K * (K - 1) * (K - 2) // 6
    out = dict(xy=torch.empty((F, T, 2), dtype=torch.float64, device=xy.device), v=torch.empty((F, T), dtype=torch.int32, device=xy.device),
               count=torch.empty(F, dtype=torch.int32, device=xy.device), K=K)
    check(_lib.load().apgpu_triangle_build(_ptr(xy), _ptr(count), F, M, K, float(min_side), T, _ptr(out['xy']), _ptr(out['v']),
                                           _ptr(out['count']), _stream()))
    return out


def triangle_unpack(tri):
    """triangle_build's lists on the host: per frame a dict(x, y float64 [n]; v int64 [n, 3] = v0, v1, v2; orient int64 [n]),
    sorted by (v0, v1, v2)."""
    xy, v, n = tri['xy'].cpu().numpy(), tri['v'].cpu().numpy().astype(np.int64), tri['count'].cpu().numpy()
    frames = []
    for f in range(len(n)):
        w = v[f, :n[f]]
        vv = np.stack([w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xff], axis=1)
        order = np.lexsort((vv[:, 2], vv[:, 1], vv[:, 0]))
        frames.append(dict(x=xy[f, :n[f], 0][order], y=xy[f, :n[f], 1][order], v=vv[order], orient=((w >> 24) - 1)[order]))
    return frames


def triangle_vote(tri, eps=0.002, allow_mirror=False):
    """votes int32 [F, K, K] (device): votes[f, i, j] = the matching (reference triangle, frame-f triangle) pairs - invariants
    within eps of each other, inclusive, and equal orientation unless allow_mirror - in which reference star i and star j of
    frame f are the same canonical vertex.  Exact integers, the same on every run."""
    F, T = int(tri['v'].shape[0]), int(tri['v'].shape[1])
    K = int(tri['K'])
    votes = torch.empty((F, K, K), dtype=torch.int32, device=tri['v'].device)
    check(_lib.load().apgpu_triangle_vote(_ptr(tri['xy']), _ptr(tri['v']), _ptr(tri['count']), F, T, K, float(eps), int(bool(allow_mirror)),
                                          _ptr(votes), _stream()))
    return votes


def _poly_maps(maps, n, what='maps'):
    """maps: a sequence of n distortion.PolyMap of one degree, origin and scale, or (coef [n, 2, ncoef], (x0, y0), L).
    -> (coef float64 numpy [n, 2, ncoef], degree, x0, y0, L), checked."""
    from . import distortion
    if isinstance(maps, tuple) and len(maps) == 3 and not isinstance(maps[0], distortion.PolyMap):
        coef = np.array(maps[0], dtype=np.float64)
        if coef.ndim != 3 or coef.shape[1] != 2:
            raise ValueError('%s: the coefficients must be [frames, 2, ncoef], got %s' % (what, coef.shape))
        maps = [distortion.PolyMap(c[0], c[1], maps[1], maps[2]) for c in coef]
    maps = list(maps)
    if len(maps) != n or not all(isinstance(m, distortion.PolyMap) for m in maps):
        raise ValueError('%s must hold one PolyMap per frame (%d)' % (what, n))
    return distortion.stack_coefficients(maps)


def nearest_match(xy, count, transforms, radius, maps=None):
    """Nearest neighbours under per-frame maps, reference -> frame: affines (transforms [F, 6]) or, with maps= (one
    distortion.PolyMap per frame, one degree, origin and scale; transforms is then not looked at), polynomials.  fwd_idx / fwd_d2
    [F, M] for every reference star the nearest star of frame f to its image and the squared distance, bwd_idx / bwd_d2 [F, M] for
    every star of frame f the reference star whose image is nearest.  Only neighbours with d2 <= radius^2 (inclusive) count; ties
    go to the lower index; no neighbour: -1 and inf.  Device tensors."""
    xy, count = _star_lists(xy, count)
    F, M = int(xy.shape[0]), int(xy.shape[1])
    if M > _lib.REGISTER_MAX_STARS:
        raise ValueError('lists of %d stars: at most %d' % (M, _lib.REGISTER_MAX_STARS))
    idx = torch.empty((2, F, M), dtype=torch.int32, device=xy.device)
    d2 = torch.empty((2, F, M), dtype=torch.float64, device=xy.device)
    if maps is None:
        T = torch.as_tensor(np.asarray(transforms, np.float64).reshape(F, 6)).to(xy.device).contiguous()
        check(_lib.load().apgpu_nearest_match(_ptr(xy), _ptr(count), _ptr(T), F, M, float(radius), _ptr(idx[0]), _ptr(d2[0]), _ptr(idx[1]),
                                              _ptr(d2[1]), _stream()))
    else:
        coef, degree, x0, y0, L = _poly_maps(maps, F)
        T = torch.from_numpy(np.ascontiguousarray(coef)).to(xy.device)
        check(_lib.load().apgpu_nearest_match_poly(_ptr(xy), _ptr(count), _ptr(T), degree, x0, y0, L, F, M, float(radius), _ptr(idx[0]),
                                                   _ptr(d2[0]), _ptr(idx[1]), _ptr(d2[1]), _stream()))
    return dict(fwd_idx=idx[0], fwd_d2=d2[0], bwd_idx=idx[1], bwd_d2=d2[1])


def _register_apply(A, pts):
    return np.stack([(A[0] * pts[:, 0] + A[1] * pts[:, 1]) + A[2], (A[3] * pts[:, 0] + A[4] * pts[:, 1]) + A[5]], axis=1)


def _register_fit(r, s, kind):
    """Least squares s ~ T(r), coordinates centred on r's mean: 'similarity' (4 parameters), 'mirror' (a similarity after a
    reflection) or 'affine' (6).  Returns (coefficients [6], 2-D rms of the residuals)."""
    m = r.mean(axis=0)
    xc, yc = r[:, 0] - m[0], r[:, 1] - m[1]
    one, zero = np.ones_like(xc), np.zeros_like(xc)
    if kind == 'affine':
        D = np.stack([xc, yc, one], axis=1)
        (a0, a1, tx), (a3, a4, ty) = np.linalg.lstsq(D, s[:, 0], rcond=None)[0], np.linalg.lstsq(D, s[:, 1], rcond=None)[0]
    else:
        sgn = 1.0 if kind == 'similarity' else -1.0
        D = np.concatenate([np.stack([xc, -sgn * yc, one, zero], axis=1), np.stack([sgn * yc, xc, zero, one], axis=1)])
        a, b, tx, ty = np.linalg.lstsq(D, np.concatenate([s[:, 0], s[:, 1]]), rcond=None)[0]
        a0, a1, a3, a4 = a, -sgn * b, b, sgn * a
    A = np.array([a0, a1, tx - (a0 * m[0] + a1 * m[1]), a3, a4, ty - (a3 * m[0] + a4 * m[1])])
    res = _register_apply(A, r) - s
    return A, float(np.sqrt(np.mean(res[:, 0] ** 2 + res[:, 1] ** 2)))


def _register_seeds(V):
    """Mutual arg-max pairs (lowest index on ties) of one frame's votes [K, K] that hold at least half the largest vote."""
    vmax = int(V.max()) if V.size else 0
    if vmax <= 0:
        return np.zeros((0, 2), np.int64)
    row_best, col_best = V.argmax(axis=1), V.argmax(axis=0)
    i = np.arange(V.shape[0])
    ok = (col_best[row_best] == i) & (V[i, row_best] > 0) & (2 * V[i, row_best].astype(np.int64) >= vmax)
    return np.stack([i[ok], row_best[ok]], axis=1).astype(np.int64)


REGISTER_POLY_MODELS = ('poly2', 'poly3', 'poly4', 'poly5')


def _register_polynomial(out, xy, count, degree, match_radius, max_rounds):
    """Step 7 of DESIGN 4.3e': `out` is register_lists' result with the affine model; adds the polynomial of `degree`."""
    from .distortion import PolyMap, ncoef
    xy, count = _star_lists(xy, count)
    F, M = int(xy.shape[0]), int(xy.shape[1])
    pts, cnt = xy.cpu().numpy(), np.clip(count.cpu().numpy(), 0, M)
    ref = pts[0, :cnt[0]]
    if cnt[0] > 0:
        lo, hi = ref.min(axis=0), ref.max(axis=0)
        origin, L = (float(0.5 * (lo[0] + hi[0])), float(0.5 * (lo[1] + hi[1]))), float(0.5 * np.hypot(hi[0] - lo[0], hi[1] - lo[1]))
    else:
        origin, L = (0.0, 0.0), 1.0
    L = L if L > 0.0 else 1.0
    ident = PolyMap.from_affine(REGISTER_IDENTITY, degree, origin, L)
    maps = [PolyMap.from_affine(out['coeffs'][f], degree, origin, L) if out['ok'][f] else ident for f in range(F)]
    out.update(order=np.ones(F, np.int64), origin=origin, scale=L, rms_affine=out['rms'].copy())
    rms, pairs = out['rms'].copy(), [None] * F
    live = [f for f in range(1, F) if out['ok'][f]]
    fitted = {}
    for rnd in range(max_rounds):
        if not live:
            break
        radius = {f: float(np.clip(3.0 * rms[f], 0.5, match_radius)) for f in live}
        found = {}
        for rad in sorted(set(radius.values())):
            nm = nearest_match(xy, count, None, rad, maps=maps)
            fwd, bwd = nm['fwd_idx'].cpu().numpy(), nm['bwd_idx'].cpu().numpy()
            for f in live:
                if radius[f] == rad:
                    i = np.nonzero(fwd[f] >= 0)[0]
                    i = i[bwd[f][fwd[f][i]] == i]
                    found[f] = np.stack([i, fwd[f][i]], axis=1).astype(np.int64)
        still = []
        for f in live:
            if pairs[f] is not None and np.array_equal(found[f], pairs[f]):
                continue
            pairs[f] = found[f]
            m = None
            if len(pairs[f]) >= 3 * ncoef(degree):
                m, _, r = PolyMap.fit(pts[0, pairs[f][:, 0]], pts[f, pairs[f][:, 1]], degree, origin, L)
            if m is None:                                    # too few pairs or a rank-deficient design: the frame keeps its affine
                fitted.pop(f, None)
                maps[f] = PolyMap.from_affine(out['coeffs'][f], degree, origin, L)
                continue
            maps[f], rms[f], fitted[f] = m, r, pairs[f]
            still.append(f)
        live = still
    for f, pr in fitted.items():
        out['order'][f], out['rms'][f], out['n_matched'][f], out['pairs'][f] = degree, rms[f], len(pr), pr
    out['maps'] = [maps[f] if out['ok'][f] else None for f in range(F)]
    return out


def register_lists(xy, count, K=40, eps=0.002, min_side=5.0, match_radius=3.0, model='affine', allow_mirror=False, max_rounds=4):
    """Registers frames 1 .. F-1 on frame 0 from their star lists (xy [F, M, 2] float64, x = column, 0-based pixel centres,
    brightest first, padded; count [F]): triangle votes among the K brightest stars -> seed pairs -> a similarity fit -> up to
    max_rounds rounds of (mutual nearest neighbours on the full lists, refit with `model`: 'affine' from 6 pairs on, else a
    similarity).  The rule is DESIGN 4.3e; the kernels do the triangle and neighbour searches, the fits are a few float64
    NumPy lines.

    Returns a dict over frames: coeffs [F, 6] (x_frame = a0 x + a1 y + a2, y_frame = a3 x + a4 y + a5 for x, y on the grid of
    frame 0: what resample_affine and ap_coadd take; NaN where not ok), ok [F] bool, n_seed, n_matched [F], rms [F] (the 2-D
    rms of the matched pairs about the fit, pixels), pairs (per frame [n, 2]: reference index, frame index) and votes (device).
    A frame that cannot be registered has ok = False: that is a status, not an error.  Frame 0 gets the identity.

    model 'poly2' .. 'poly5' (DESIGN 4.3e'): the steps above with the affine model, then for every ok frame a polynomial of that
    degree (distortion.PolyMap), refined from the affine by up to max_rounds rounds of (mutual nearest neighbours under the
    polynomial at clip(3 rms, 0.5, match_radius), refit) until the pair set repeats.  The result then also holds maps (a PolyMap
    per frame, None where not ok), order [F] (the degree; 1 where the frame keeps its affine - fewer than 3 ncoef pairs or a
    rank-deficient design, a status too - and for frame 0), origin (the midpoint of the bounding box of frame 0's stars), scale
    (half its diagonal) and rms_affine; rms, n_matched and pairs are the polynomial's where order > 1; coeffs stays the affine."""
    if model not in ('affine', 'similarity') + REGISTER_POLY_MODELS:
        raise ValueError("model must be 'affine', 'similarity' or 'poly2' .. 'poly5', got %r" % (model,))
    if model in REGISTER_POLY_MODELS:
        out = register_lists(xy, count, K, eps, min_side, match_radius, 'affine', allow_mirror, max_rounds)
        return _register_polynomial(out, xy, count, int(model[4:]), match_radius, max_rounds)
    xy, count = _star_lists(xy, count)
    F, M = int(xy.shape[0]), int(xy.shape[1])
    tri = triangle_build(xy, count, K, min_side)
    votes_t = triangle_vote(tri, eps, allow_mirror)
    votes = votes_t.cpu().numpy()
    pts, cnt = xy.cpu().numpy(), np.clip(count.cpu().numpy(), 0, M)
    out = dict(coeffs=np.full((F, 6), np.nan), ok=np.zeros(F, bool), n_seed=np.zeros(F, np.int64), n_matched=np.zeros(F, np.int64),
               rms=np.full(F, np.nan), pairs=[np.zeros((0, 2), np.int64) for _ in range(F)], votes=votes_t)
    out['coeffs'][0], out['ok'][0], out['rms'][0], out['n_matched'][0] = REGISTER_IDENTITY, True, 0.0, cnt[0]
    out['pairs'][0] = np.stack([np.arange(cnt[0]), np.arange(cnt[0])], axis=1)
    A = np.tile(np.asarray(REGISTER_IDENTITY), (F, 1))
    rms, kind, seeds, pairs = np.zeros(F), ['similarity'] * F, [None] * F, [None] * F
    live = []
    for f in range(1, F):
        seeds[f] = _register_seeds(votes[f])
        out['n_seed'][f] = len(seeds[f])
        if len(seeds[f]) < 3:
            continue
        r, s = pts[0, seeds[f][:, 0]], pts[f, seeds[f][:, 1]]
        A[f], rms[f] = _register_fit(r, s, 'similarity')
        if allow_mirror:
            Am, rmsm = _register_fit(r, s, 'mirror')
            if rmsm < rms[f]:
                A[f], rms[f], kind[f] = Am, rmsm, 'mirror'
        live.append(f)
    for rnd in range(max_rounds):
        if not live:
            break
        # one launch per radius: in the first round all frames share match_radius, later each has its own
        radius = {f: float(match_radius) if rnd == 0 else float(np.clip(3.0 * rms[f], 0.5, match_radius)) for f in live}
        found = {}
        for rad in sorted(set(radius.values())):
            nm = nearest_match(xy, count, A, rad)
            fwd, bwd = nm['fwd_idx'].cpu().numpy(), nm['bwd_idx'].cpu().numpy()
            for f in live:
                if radius[f] == rad:
                    i = np.nonzero(fwd[f] >= 0)[0]
                    i = i[bwd[f][fwd[f][i]] == i]
                    found[f] = np.stack([i, fwd[f][i]], axis=1).astype(np.int64)
        still = []
        for f in live:
            if pairs[f] is not None and np.array_equal(found[f], pairs[f]):
                continue
            pairs[f] = found[f]
            if len(pairs[f]) < 3:
                continue
            A[f], rms[f] = _register_fit(pts[0, pairs[f][:, 0]], pts[f, pairs[f][:, 1]],
                                         'affine' if model == 'affine' and len(pairs[f]) >= 6 else kind[f])
            still.append(f)
        live = still
    for f in range(1, F):
        if pairs[f] is None:
            continue
        out['n_matched'][f], out['pairs'][f] = len(pairs[f]), pairs[f]
        if len(pairs[f]) >= max(3, len(seeds[f])):
            out['coeffs'][f], out['ok'][f], out['rms'][f] = A[f], True, rms[f]
    return out


# ------------------------------------------------------------------------------------------------------------------
# F9: ApComposite - colour composites of three co-added planes (csrc/composite.hip; STIFF absent, parity unpinned)
TONE_OCTAVES, TONE_KNOTS = 40, 256


def _planes3(planes):
    _need_cuda(planes)
    if planes.dim() != 3 or planes.shape[0] != 3 or planes.shape[1] < 1 or planes.shape[2] < 1:
        raise ValueError('planes must be [3, H, W] (red, green, blue), got %s' % (tuple(planes.shape),))
    return _f32c(planes, 'planes')


def quantile_levels(planes, q, manual=None):
    """Exact order statistics of the finite values of each channel: planes [3, H, W] float32, q [3, 2] (min and max quantile per
    channel, 0 .. 1), manual [3, 2] or None (an entry that is not NaN replaces that level).  The level of q is
    v[floor(q (n - 1))] of the sorted finite values (np.quantile, method='lower'); no finite value: NaN.

    Returns (levels float32 [3, 2], n_finite int64 [3]), both on the device: nothing is read back."""
    planes = _planes3(planes)
    qa = np.array(np.broadcast_to(np.asarray(q, np.float64), (3, 2)))
    if not np.all((qa >= 0.0) & (qa <= 1.0)):
        raise ValueError('quantiles must lie in 0 .. 1, got %s' % (qa.tolist(),))
    dev = planes.device
    qd = torch.from_numpy(qa).to(dev)
    md = None
    if manual is not None:
        md = torch.from_numpy(np.array(np.broadcast_to(np.asarray(manual, np.float32), (3, 2)))).to(dev)
    H, W = int(planes.shape[1]), int(planes.shape[2])
    lib = _lib.load()
    ws_bytes = lib.apgpu_quantile_levels_ws_bytes(H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    levels = torch.empty((3, 2), dtype=torch.float32, device=dev)
    n_finite = torch.empty(3, dtype=torch.int64, device=dev)
    check(lib.apgpu_quantile_levels_f32(_ptr(planes), H, W, _ptr(qd), _ptr(md), _ptr(levels), _ptr(n_finite), _ptr(ws), ws_bytes,
                                        _stream()))
    return levels, n_finite


def tone_table(gamma=2.2, gamma_fac=1.0, gamma_type='POWER-LAW'):
    """The float32 table of G(Y) = T(Y) / Y for the luminance curve T(Y) = Y^(1 / (gamma gamma_fac)) (STIFF's POWER-LAW gamma
    type; any other raises ValueError): 256 knots per octave over 2^-40 .. 2^0 and one closing knot for Y = 1, each the float64
    value at the knot rounded once to float32.  Host array [10241]; composite_rgb looks it up by the bits of Y."""
    if str(gamma_type).upper() != 'POWER-LAW':
        raise ValueError('gamma type %r is not supported: POWER-LAW only' % (gamma_type,))
    g = float(gamma) * float(gamma_fac)
    if not (g > 0.0 and np.isfinite(g)):
        raise ValueError('gamma * gamma_fac must be positive and finite, got %r' % (g,))
    e = np.arange(-TONE_OCTAVES, 0, dtype=np.float64)[:, None]
    m = np.arange(TONE_KNOTS, dtype=np.float64)[None, :]
    y = np.concatenate([(np.exp2(e) * (1.0 + m / TONE_KNOTS)).ravel(), [1.0]])
    table = (np.power(y, 1.0 / g) / y).astype(np.float32)
    assert table.size == _lib.TONE_TABLE_LEN
    return table


def composite_rgb(planes, levels, tables, colour_sat, bits=8, flip=True, out=None):
    """V colour composites from one read of planes [3, H, W] float32: levels [3, 2] float32 (device: quantile_levels), tables
    [V, 10241] float32 (tone_table per variant; host or device), colour_sat [V].  Returns out [V, H, W, 3] uint8 (bits = 8) or
    uint16 (bits = 16), interleaved RGB; flip (STIFF's orientation): output row r is FITS row H - 1 - r.  V <= 16.  The
    per-pixel arithmetic is DESIGN 4.3f / include/apgpu.h."""
    planes = _planes3(planes)
    dev = planes.device
    if bits not in (8, 16):
        raise ValueError('bits must be 8 or 16, got %r' % (bits,))
    tables = torch.as_tensor(tables, dtype=torch.float32).to(dev).contiguous()
    if tables.dim() == 1:
        tables = tables[None]
    sat = np.ascontiguousarray(np.asarray(colour_sat, np.float32).reshape(-1))
    V = int(tables.shape[0])
    if tables.dim() != 2 or tables.shape[1] != _lib.TONE_TABLE_LEN:
        raise ValueError('tables must be [V, %d], got %s' % (_lib.TONE_TABLE_LEN, tuple(tables.shape)))
    if not 1 <= V <= _lib.COMPOSITE_MAX_VARIANTS or sat.size != V:
        raise ValueError('%d tables and %d saturations: 1 .. %d variants, one saturation each' % (V, sat.size, _lib.COMPOSITE_MAX_VARIANTS))
    levels = torch.as_tensor(levels, dtype=torch.float32).to(dev).contiguous()
    if tuple(levels.shape) != (3, 2):
        raise ValueError('levels must be [3, 2], got %s' % (tuple(levels.shape),))
    H, W = int(planes.shape[1]), int(planes.shape[2])
    dt = torch.uint8 if bits == 8 else torch.uint16
    if out is None:
        out = torch.empty((V, H, W, 3), dtype=dt, device=dev)
    elif out.dtype != dt or tuple(out.shape) != (V, H, W, 3) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError('out must be a contiguous device tensor [%d, %d, %d, 3] of %s' % (V, H, W, dt))
    check(_lib.load().apgpu_composite_rgb(_ptr(planes), H, W, _ptr(levels), _ptr(tables), sat.ctypes.data_as(C.POINTER(C.c_float)), V,
                                          int(bits), int(bool(flip)), _ptr(out), _stream()))
    return out


# ------------------------------------------------------------------------------------------------------------------
# F10: ApDebayer - Bayer demosaic, white-balance scaling and the sums behind the white balance (csrc/demosaic.hip, DESIGN 4.3g;
# LibRaw absent: the interpolation is this project's definition)
DEMOSAIC_METHODS = {'bilinear': 0, 'mhc': 1, 'superpixel': 2, 'rcd': 4}          # APGPU_DEMOSAIC_*; 3 is no method
DEMOSAIC_OUTPUTS = {'rgb': 0, 'rgb_u16': 1, 'grey': 2, 'direct': 3}


def bayer_pattern(pattern):
    """Four ints: the colour (R 0, G1 1, B 2, G2 3) of cell position (r & 1) 2 + (c & 1); ValueError unless it is a Bayer
    arrangement (a permutation of 0 .. 3 with red and blue on one diagonal)."""
    try:
        pat = [int(x) for x in pattern]
    except (TypeError, ValueError):
        pat = []
    if sorted(pat) != [0, 1, 2, 3] or pat.index(0) ^ pat.index(2) != 3:
        raise ValueError('pattern %r is not a Bayer arrangement: a permutation of 0 .. 3 (R, G1, B, G2) with red and blue on one '
                         'diagonal' % (pattern,))
    return pat


def _four_f32(x, name):
    if x is None:
        return None
    a = np.asarray(x, np.float64).reshape(-1)
    if a.size != 4:
        raise ValueError('%s takes four values (R, G1, B, G2), got %r' % (name, x))
    return np.ascontiguousarray(a.astype(np.float32))


def _f32p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _bayer_black(black, dtype):
    blk = _four_f32(black, 'black')
    if blk is not None and dtype == APGPU_U16 and not np.all((blk == np.floor(blk)) & (blk >= 0) & (blk <= 65535)):
        raise ValueError('the black levels of uint16 data must be integers 0 .. 65535, got %r' % (black,))
    return blk


def bayer_demosaic(mosaic, pattern=(0, 1, 3, 2), black=None, gain=None, method='mhc', output='rgb', out=None):
    """Colour planes of Bayer mosaics: mosaic [H, W] or [N, H, W], uint16 or float32; pattern as in bayer_split (a Bayer
    arrangement); black, gain: four values by colour (R, G1, B, G2) or None.  Every sample is float32(max(raw - black, 0)) gain.

    method  'bilinear', 'mhc' (Malvar-He-Cutler 2004), 'superpixel' (one pixel per 2 x 2 cell: H and W even, h = H / 2) or 'rcd'
            (ratio-corrected and edge-directed, modelled on RCD 2.x: follows edges and keeps stars round where the linear filters
            leave zippers and coloured rims; several times slower.  Its eps = 2^-10 is in sample units: bring a mosaic
            normalised to 0 .. 1 to ADU scale with gain)
    output  'rgb' float32 [3, h, w]; 'rgb_u16' the same clipped to 0 .. 65535 and truncated; 'grey' float32 [h, w], the CCIR 601
            luminance of the colours; 'direct' float32 [H, W], the scaled samples themselves (method is ignored)

    A slab gives [N, 3, h, w] or [N, h, w].  out: a contiguous device tensor of that shape and dtype.  The arithmetic is DESIGN
    4.3g / include/apgpu.h, restated in tests/demosaic_model.py and, for 'rcd', tests/demosaic_rcd_model.py."""
    _need_cuda(mosaic, out)
    dt = _raw_dtype(mosaic)
    if mosaic.dim() not in (2, 3):
        raise TypeError('mosaic must be [H, W] or [N, H, W], got %s' % (tuple(mosaic.shape),))
    pat = bayer_pattern(pattern)
    if method not in DEMOSAIC_METHODS:
        raise ValueError('method %r is not one of %s' % (method, sorted(DEMOSAIC_METHODS)))
    if output not in DEMOSAIC_OUTPUTS:
        raise ValueError('output %r is not one of %s' % (output, sorted(DEMOSAIC_OUTPUTS)))
    blk, gn = _bayer_black(black, dt), _four_f32(gain, 'gain')
    mosaic = mosaic.contiguous()
    single = mosaic.dim() == 2
    N = 1 if single else int(mosaic.shape[0])
    H, W = int(mosaic.shape[-2]), int(mosaic.shape[-1])
    if N < 1 or H < 2 or W < 2:
        raise ValueError('a mosaic needs at least 2 x 2 pixels and one frame, got %s' % (tuple(mosaic.shape),))
    h, w = H, W
    if method == 'superpixel' and output != 'direct':
        if H % 2 or W % 2:
            raise ValueError('superpixel needs an even number of rows and columns, got %d x %d' % (H, W))
        h, w = H // 2, W // 2
    shape = (3, h, w) if output in ('rgb', 'rgb_u16') else (h, w)
    shape = shape if single else (N,) + shape
    odt = torch.uint16 if output == 'rgb_u16' else torch.float32
    if out is None:
        out = torch.empty(shape, dtype=odt, device=mosaic.device)
    elif out.dtype != odt or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError('out must be a contiguous device tensor %s of %s' % (shape, odt))
    check(_lib.load().apgpu_bayer_demosaic(_ptr(mosaic), dt, N, H, W, (C.c_int32 * 4)(*pat), _f32p(blk), _f32p(gn),
                                           DEMOSAIC_METHODS[method], DEMOSAIC_OUTPUTS[output], _ptr(out), _stream()))
    return out


def bayer_channel_sums(mosaic, pattern, black=None, region=None):
    """The device half of RawConv._get_whitebalance_from_region (RawConv.py:291-366): for each colour (R, G1, B, G2) the sum of
    max(raw - black, 0) over its sites in region = (rowmin, rowmax, colmin, colmax), inclusive and clamped to the image (None: the
    whole image), and their number.  mosaic [H, W] uint16 gives exact uint64 sums; float32 gives float64 sums and counts of the
    finite samples.  Returns (sums [4], counts [4] int64) on the device."""
    _need_cuda(mosaic)
    dt = _raw_dtype(mosaic)
    if mosaic.dim() != 2 or mosaic.shape[0] < 2 or mosaic.shape[1] < 2:
        raise TypeError('mosaic must be [H, W] of at least 2 x 2, got %s' % (tuple(mosaic.shape),))
    pat = bayer_pattern(pattern)
    blk = _bayer_black(black, dt)
    mosaic = mosaic.contiguous()
    H, W = int(mosaic.shape[0]), int(mosaic.shape[1])
    rect = [0, H, 0, W] if region is None else [int(v) for v in region]
    if len(rect) != 4:
        raise ValueError('region takes rowmin, rowmax, colmin, colmax, got %r' % (region,))
    sums = torch.empty(4, dtype=torch.uint64 if dt == APGPU_U16 else torch.float64, device=mosaic.device)
    counts = torch.empty(4, dtype=torch.int64, device=mosaic.device)
    check(_lib.load().apgpu_bayer_channel_sums(_ptr(mosaic), dt, H, W, (C.c_int32 * 4)(*pat), _f32p(blk), (C.c_int64 * 4)(*rect),
                                               _ptr(sums), _ptr(counts), _stream()))
    return sums, counts


def whitebalance_from_sums(sums, counts):
    """Four float64 gains from the four sums and counts: avg = sum / count, gain = max(avg) / avg (RawConv.py:315-331).  A colour
    with no pixels or avg <= 0 raises ValueError (the reference divides by zero there)."""
    avg = []
    for name, s, n in zip(('R', 'G1', 'B', 'G2'), sums, counts):
        if int(n) < 1:
            raise ValueError('white balance: colour %s has no valid pixels in the region' % name)
        a = float(s) / float(int(n))
        if not a > 0.0:
            raise ValueError('white balance: colour %s has a mean of %r in the region' % (name, a))
        avg.append(a)
    top = max(avg)
    return np.array([top / a for a in avg], np.float64)


def bayer_whitebalance(mosaic, pattern, black=None, region=None):
    """RawConv.get_whitebalance('auto' | 'region[...]'): four float64 gains (R, G1, B, G2) from bayer_channel_sums; the eight
    numbers are read back and divided on the host."""
    sums, counts = bayer_channel_sums(mosaic, pattern, black, region)
    s = sums.cpu()
    s = [int(v) for v in s.view(torch.int64).tolist()] if s.dtype == torch.uint64 else s.tolist()
    return whitebalance_from_sums(s, counts.cpu().tolist())


# ------------------------------------------------------------------------------------------------------------------
# F11: ApContinuumSubtract - PSF matching, the scale and offset of the continuum, the subtraction (csrc/continuum.hip, DESIGN
# 4.3h; the reference lists the stage as not yet built: the arithmetic is this project's definition)
BLUR_MAX_RADIUS, BLUR_TILE_H, BLUR_TILE_W = _lib.BLUR_MAX_RADIUS, _lib.BLUR_TILE_H, _lib.BLUR_TILE_W
FWHM_TO_SIGMA = 0.42466090014400953                    # 1 / (2 sqrt(2 ln 2))


def gauss_taps(sigma, radius=None):
    """float64 taps w[0 .. 2R] of a Gaussian of `sigma` pixels, exp(-(k - R)^2 / (2 sigma^2)) normalised to sum 1, R = ceil(4 sigma)
    (at least 1) unless given.  sigma = 0 or radius = 0: the identity {1}.  R > 32 raises ValueError."""
    import math
    sigma = float(sigma)
    if not sigma >= 0.0 or not math.isfinite(sigma):
        raise ValueError('sigma must be finite and >= 0, got %r' % sigma)
    if radius is None:
        radius = 0 if sigma == 0.0 else max(1, int(math.ceil(4.0 * sigma)))
    radius = int(radius)
    if radius < 0 or radius > BLUR_MAX_RADIUS:
        raise ValueError('a blur of sigma = %g pixels needs a radius of %d, the kernel holds %d' % (sigma, radius, BLUR_MAX_RADIUS))
    if radius == 0 or sigma == 0.0:
        w = np.zeros(2 * radius + 1)
        w[radius] = 1.0
        return w
    k = np.arange(2 * radius + 1, dtype=np.float64) - radius
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum()


def gauss_blur(data, sigma, min_weight=0.5, out=None):
    """The normalised, separable Gaussian blur of a float32 image [H, W] whose NaN / inf pixels mean "no data": every output is
    the weighted mean of the valid pixels under the kernel, NaN where the pixel itself is missing or the valid weight is below
    min_weight.  sigma: pixels, or the float64 taps themselves (an odd number, at most 65).  float64 accumulation in a fixed
    order (include/apgpu.h F11; tests/continuum_model.py)."""
    data = _image_f32(data)
    _need_cuda(out)
    taps = gauss_taps(sigma) if np.ndim(sigma) == 0 else np.ascontiguousarray(np.asarray(sigma, np.float64).reshape(-1))
    if taps.size % 2 != 1:
        raise ValueError('the taps must be an odd number of weights, got %d' % taps.size)
    R = (taps.size - 1) // 2
    if R > BLUR_MAX_RADIUS:
        raise ValueError('a blur radius of %d, the kernel holds %d' % (R, BLUR_MAX_RADIUS))
    if not float(min_weight) >= 0.0:
        raise ValueError('min_weight must be >= 0, got %r' % (min_weight,))
    out = _out_f32(out, data, data)
    check(_lib.load().apgpu_gauss_blur_norm_f32(_ptr(data), data.shape[0], data.shape[1], taps.ctypes.data_as(C.POINTER(C.c_double)), R,
                                                float(min_weight), _ptr(out), _stream()))
    return out


def _pair(n, c, mask=None):
    n, c = _image_f32(n, 'n'), _image_f32(c, 'c')
    if tuple(n.shape) != tuple(c.shape):
        raise ValueError('the two images must have one shape, got %s and %s' % (tuple(n.shape), tuple(c.shape)))
    return n, c, _mask_u8(mask, n.shape, 'mask must have the image shape')


def pair_moments(n, c, s=0.0, b=0.0, lo=-float('inf'), hi=float('inf'), mask=None, ws=None):
    """float64 device tensor [6] = count, sum c, sum n, sum c c, sum c n, sum n n over the pixel pairs that are finite in both
    float32 images, unmasked (mask == 0) and whose residual r = n - (s c + b) lies in [lo, hi] (inclusive; float64).  The same
    input gives the same bits on every run.  ws: a uint8 workspace from an earlier call's size, or None."""
    n, c, mask = _pair(n, c, mask)
    lib = _lib.load()
    need = lib.apgpu_pair_moments_ws_bytes(n.numel())
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=n.device)
    out = torch.empty(6, dtype=torch.float64, device=n.device)
    check(lib.apgpu_pair_moments_f64(_ptr(n), _ptr(c), _ptr(mask), n.numel(), float(s), float(b), float(lo), float(hi), _ptr(out), _ptr(ws),
                                     ws.numel(), _stream()))
    return out


def linear_combine(x, y, ca, cb, c0, out=None):
    """out = (float32(ca x) + float32(cb y)) + c0 in float32, NaN where x or y is not finite; y None: float32(ca x) + c0.  Tensors
    of any one shape; out may be x or y."""
    _need_cuda(x, y, out)
    x = _f32c(x, 'x')
    y = _f32c(y, 'y')
    if x.numel() == 0 or (y is not None and tuple(y.shape) != tuple(x.shape)):
        raise ValueError('x and y must be non-empty tensors of one shape')
    out = _out_f32(out, x)
    check(_lib.load().apgpu_linear_combine_f32(_ptr(x), _ptr(y), float(np.float32(ca)), float(np.float32(cb)), float(np.float32(c0)), _ptr(out),
                                               x.numel(), _stream()))
    return out


def _line_from_moments(mom, fixed_scale=None):
    """The straight line n = s c + b from the six moments, in centred form (float64 on the host)."""
    import math
    cnt, sc, sy, scc, scy, syy = (float(v) for v in mom)
    if cnt < 3:
        raise RuntimeError('continuum fit: %d valid pixel pairs survive, at least 3 are needed' % int(cnt))
    cbar, ybar = sc / cnt, sy / cnt
    Scc, Scy, Syy = scc - sc * cbar, scy - sc * ybar, syy - sy * ybar
    if fixed_scale is None:
        if not Scc > 0.0:
            raise RuntimeError('continuum fit: the continuum image has zero variance over the valid pixels')
        s = Scy / Scc
        rss, dof = Syy - s * Scy, cnt - 2.0
    else:
        s = float(fixed_scale)
        rss, dof = (Syy - 2.0 * s * Scy) + s * s * Scc, cnt - 1.0
    rss = max(rss, 0.0)
    var = rss / dof
    se_s = math.sqrt(var / Scc) if fixed_scale is None else 0.0
    se_b = math.sqrt(var * (1.0 / cnt + cbar * cbar / Scc)) if fixed_scale is None else math.sqrt(var / cnt)
    return dict(s=s, b=ybar - s * cbar, sigma=math.sqrt(rss / cnt), n=int(cnt), se_s=se_s, se_b=se_b)


def _truncated_gauss(alpha, beta):
    """(mean, variance) of a unit Gaussian cut to [alpha, beta]."""
    import math
    phi = lambda x: math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi) if math.isfinite(x) else 0.0      # noqa: E731
    Phi = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))                                               # noqa: E731
    Z = Phi(beta) - Phi(alpha)
    pa, pb = phi(alpha), phi(beta)
    mean = (pa - pb) / Z
    return mean, 1.0 + ((alpha * pa if math.isfinite(alpha) else 0.0) - (beta * pb if math.isfinite(beta) else 0.0)) / Z - mean * mean


def truncation_shift(sigma_lower=3.0, sigma_upper=2.0):
    """The mean of a unit Gaussian cut to [-sigma_lower, sigma_upper]: -0.0508 for the defaults."""
    return _truncated_gauss(-float(sigma_lower), float(sigma_upper))[0]


def gaussian_truncation(lo, hi, mean_kept, sigma_kept):
    """(mu, sigma0) of the Gaussian whose part inside [lo, hi] has the mean mean_kept and the standard deviation sigma_kept: the
    truncated Gaussian's closed-form mean and variance, solved for the Gaussian by fixed-point rounds."""
    import math
    if not (math.isfinite(lo) or math.isfinite(hi)) or not sigma_kept > 0.0:
        return mean_kept, sigma_kept
    mu, s0 = mean_kept, sigma_kept
    for _ in range(200):
        m, var = _truncated_gauss((lo - mu) / s0, (hi - mu) / s0)
        ns0 = sigma_kept / math.sqrt(var)
        nmu = mean_kept - ns0 * m
        done = abs(ns0 - s0) <= 1e-13 * s0 and abs(nmu - mu) <= 1e-13 * s0
        mu, s0 = nmu, ns0
        if done:
            break
    return mu, s0


def continuum_scale_pixels(n, c, mask=None, sigma_lower=3.0, sigma_upper=2.0, maxiters=10, fixed_scale=None):
    """The iteratively clipped straight-line fit n = s c + b over the valid pixel pairs of two float32 device images: the unclipped
    fit first, then bounds [-sigma_lower sigma, +sigma_upper sigma] on the residuals about the last line (sigma the rms residual of
    the kept pixels) until the count stands still or maxiters fits were made; one launch and one 48-byte read-back per round.
    Emission only adds to n, hence the tighter upper bound; b is then corrected for the shift an asymmetric cut gives the mean of
    Gaussian noise (gaussian_truncation).  fixed_scale: s is held and only b is fitted.

    Returns dict(s, b, b_uncorrected, sigma, sigma0, shift, n, n_unclipped, iterations, se_s, se_b, lo, hi)."""
    n, c, mask = _pair(n, c, mask)
    ws = torch.empty(_lib.load().apgpu_pair_moments_ws_bytes(n.numel()), dtype=torch.uint8, device=n.device)
    lo, hi = -float('inf'), float('inf')
    fit = _line_from_moments(pair_moments(n, c, 0.0, 0.0, lo, hi, mask, ws).cpu().numpy(), fixed_scale)
    n_unclipped, prev_b, count, iters = fit['n'], fit['b'], fit['n'], 0
    for _ in range(int(maxiters)):
        nlo, nhi = -float(sigma_lower) * fit['sigma'], float(sigma_upper) * fit['sigma']
        mom = pair_moments(n, c, fit['s'], fit['b'], nlo, nhi, mask, ws).cpu().numpy()
        if int(mom[0]) == count:
            break
        prev_b = fit['b']
        fit = _line_from_moments(mom, fixed_scale)
        lo, hi, count = nlo, nhi, fit['n']
        iters += 1
    mu, sigma0 = gaussian_truncation(lo, hi, fit['b'] - prev_b, fit['sigma'])
    out = dict(fit)
    out.update(b=prev_b + mu, b_uncorrected=fit['b'], sigma0=sigma0, shift=fit['b'] - (prev_b + mu), iterations=iters, lo=lo, hi=hi,
               n_unclipped=n_unclipped)
    return out


def _clipped_median(x, sigma=3.0, maxiters=5):
    x = np.asarray(x, np.float64).ravel()
    x = x[np.isfinite(x)]
    for _ in range(int(maxiters)):
        if x.size == 0:
            break
        med, sd = np.median(x), np.std(x)
        y = x[(x >= med - sigma * sd) & (x <= med + sigma * sd)]
        if y.size == x.size:
            break
        x = y
    if x.size == 0:
        return float('nan'), float('nan'), 0
    return float(np.median(x)), float(np.std(x)), int(x.size)


def continuum_scale_stars(n, c, xy, fwhm, peak=None, satlevel=None, min_stars=5, mask=None, sigma_lower=3.0, sigma_upper=2.0,
                          maxiters=10):
    """s from the stars, b from the pixels.  Stars are continuum sources: aperture_photometry of both (PSF-matched) float32 device
    images at the positions xy [k, 2] (x = column, y = row), aperture and annulus from `fwhm` (the broader one; aperture_radii), the
    flux sky-subtracted by the annulus median.  Kept: both fluxes positive and finite, peak < satlevel where both are given.  s =
    the sigma-clipped median (3 sigma, 5 rounds, float64 on the host) of F_N / F_C; b from continuum_scale_pixels with s held.
    Fewer than min_stars kept stars raise RuntimeError.

    Returns the dict of continuum_scale_pixels plus n_stars, n_stars_used, ratio_spread, flux_n, flux_c (NumPy) and se_s =
    spread / sqrt(stars used)."""
    import math
    n, c, mask = _pair(n, c, mask)
    xy = np.asarray(xy.cpu() if torch.is_tensor(xy) else xy, np.float64).reshape(-1, 2)
    fn = aperture_photometry(n, xy[:, 0], xy[:, 1], fwhm=fwhm)['aperture_sum'].cpu().numpy()
    fc = aperture_photometry(c, xy[:, 0], xy[:, 1], fwhm=fwhm)['aperture_sum'].cpu().numpy()
    keep = np.isfinite(fn) & np.isfinite(fc) & (fn > 0) & (fc > 0)
    if peak is not None and satlevel is not None:
        keep &= np.asarray(peak, np.float64).reshape(-1) < float(satlevel)
    if int(keep.sum()) < int(min_stars):
        raise RuntimeError('continuum scale from stars: %d usable stars, at least %d are needed' % (int(keep.sum()), int(min_stars)))
    s, spread, used = _clipped_median(fn[keep] / fc[keep])
    out = continuum_scale_pixels(n, c, mask, sigma_lower, sigma_upper, maxiters, fixed_scale=s)
    out.update(se_s=spread / math.sqrt(max(used, 1)), n_stars=int(keep.sum()), n_stars_used=used, ratio_spread=spread, flux_n=fn, flux_c=fc,
               keep=keep)
    return out


def psf_match(n, c, fwhm_n, fwhm_c, threshold=0.05, min_weight=0.5):
    """Brings two float32 device images to one PSF: the sharper one is blurred with a Gaussian of sigma_k = sqrt(sigma_broad^2 -
    sigma_sharp^2), sigma = FWHM / (2 sqrt(2 ln 2)); |FWHM_n - FWHM_c| < threshold blurs nothing.  A sigma_k that needs a radius
    above 32 raises ValueError naming the FWHMs.  Returns (n', c', dict(blurred 'narrow' | 'continuum' | None, sigma_k, taps))."""
    import math
    n, c, _ = _pair(n, c)
    fwhm_n, fwhm_c = float(fwhm_n), float(fwhm_c)
    if not (fwhm_n > 0 and fwhm_c > 0 and math.isfinite(fwhm_n) and math.isfinite(fwhm_c)):
        raise ValueError('the FWHMs must be positive and finite, got %r and %r' % (fwhm_n, fwhm_c))
    if abs(fwhm_n - fwhm_c) < float(threshold):
        return n, c, dict(blurred=None, sigma_k=0.0, taps=None)
    sn, sc = fwhm_n * FWHM_TO_SIGMA, fwhm_c * FWHM_TO_SIGMA
    broad, sharp = max(sn, sc), min(sn, sc)
    sigma_k = math.sqrt(broad * broad - sharp * sharp)
    try:
        taps = gauss_taps(sigma_k)
    except ValueError as exc:
        raise ValueError('PSF matching FWHM %g to %g: %s' % (fwhm_n, fwhm_c, exc)) from None
    if sn < sc:
        return gauss_blur(n, taps, min_weight), c, dict(blurred='narrow', sigma_k=sigma_k, taps=taps)
    return n, gauss_blur(c, taps, min_weight), dict(blurred='continuum', sigma_k=sigma_k, taps=taps)


# ------------------------------------------------------------------------------------------------------------------
# F12: ApDeconvolve - damped Richardson-Lucy deconvolution with the image's own PSF (csrc/deconvolve.hip; the
# reference has no such stage: the arithmetic is this project's definition, include/apgpu.h F12, tests/deconvolve_model.py)
DECONV_MAX_RADIUS = _lib.DECONV_MAX_RADIUS


def _psf_sampled(profile, fwhm, radius, default_radius):
    import math
    fwhm = float(fwhm)
    if not (fwhm > 0.0 and math.isfinite(fwhm)):
        raise ValueError('the FWHM must be finite and > 0, got %r' % fwhm)
    R = int(default_radius if radius is None else radius)
    if R < 0 or R > DECONV_MAX_RADIUS:
        raise ValueError('a PSF of FWHM %g pixels needs a radius of %d, the kernels hold %d: bin the image' % (fwhm, R, DECONV_MAX_RADIUS))
    k = np.arange(2 * R + 1, dtype=np.float64) - R
    sub = (np.arange(5, dtype=np.float64) + 0.5) / 5.0 - 0.5             # 5 x 5 midpoints inside the pixel
    g = np.zeros((2 * R + 1, 2 * R + 1), np.float64)
    for dy in sub:
        for dx in sub:
            g += profile((k[:, None] + dy) ** 2 + (k[None, :] + dx) ** 2)
    return (g / g.sum()).astype(np.float32)


def psf_gaussian(fwhm, radius=None):
    """float32 [K][K], K = 2 radius + 1: a round Gaussian of the given FWHM (pixels), pixel-integrated by 5 x 5 midpoint sub-sampling
    in float64, normalised to sum 1, then cast.  radius: ceil(1.7 FWHM) unless given; above 12 raises ValueError."""
    import math
    s = float(fwhm) * FWHM_TO_SIGMA
    return _psf_sampled(lambda r2: np.exp(-r2 / (2.0 * s * s)), fwhm, radius, math.ceil(1.7 * float(fwhm)))


def psf_moffat(fwhm, beta=2.5, radius=None):
    """The same for a Moffat profile (1 + r^2 / alpha^2)^-beta with alpha = FWHM / (2 sqrt(2^(1/beta) - 1)).  radius: ceil(2.5 FWHM)
    unless given; above 12 raises ValueError."""
    import math
    beta = float(beta)
    if not (beta > 1.0 and math.isfinite(beta)):
        raise ValueError('the Moffat beta must be finite and > 1, got %r' % beta)
    alpha = float(fwhm) / (2.0 * math.sqrt(2.0 ** (1.0 / beta) - 1.0))
    return _psf_sampled(lambda r2: (1.0 + r2 / (alpha * alpha)) ** -beta, fwhm, radius, math.ceil(2.5 * float(fwhm)))


def psf_stamp(psf):
    """(contiguous float32 [K][K] host array, radius) of a PSF stamp given as an array or tensor; the weights are taken as they are.
    ValueError for a shape that is not odd and square, a radius above 12, a negative or non-finite weight or a sum <= 0."""
    p = np.ascontiguousarray(psf.cpu().numpy() if hasattr(psf, 'cpu') else psf, dtype=np.float32)
    if p.ndim != 2 or p.shape[0] != p.shape[1] or p.shape[0] % 2 != 1:
        raise ValueError('the PSF stamp must be square with an odd side, got shape %s' % (p.shape,))
    R = p.shape[0] // 2
    if R > DECONV_MAX_RADIUS:
        raise ValueError('a PSF stamp of radius %d, the kernels hold %d: bin the image' % (R, DECONV_MAX_RADIUS))
    if not np.all(np.isfinite(p)) or np.any(p < 0) or not p.astype(np.float64).sum() > 0:
        raise ValueError('the PSF weights must be finite and >= 0 with a sum > 0')
    return p, R


def _psf_arg(p):
    return p.ctypes.data_as(C.POINTER(C.c_float))


def deconv_norm(data, psf, min_weight=0.1, out=None):
    """Step 1 of F12: inv = 1 / n where n = sum p W >= min_weight (W = 1 at the finite pixels), else 0."""
    data = _image_f32(data)
    p, R = psf_stamp(psf)
    out = _out_f32(out, data, data)
    check(_lib.load().apgpu_deconv_norm_f32(_ptr(data), data.shape[0], data.shape[1], _psf_arg(p), R, float(min_weight), _ptr(out), _stream()))
    return out


def deconv_ratio(u, data, psf, sky, gain=1.0, readnoise=0.0, damp=0.0, out=None):
    """Step 3 of F12: the forward convolution of u (edges replicated) plus the sky, and the (damped) ratio against the data."""
    data = _image_f32(data)
    u = _plane_like(u, 'u', data)
    p, R = psf_stamp(psf)
    out = _out_f32(out, data, u)
    check(_lib.load().apgpu_deconv_ratio_f32(_ptr(u), _ptr(data), data.shape[0], data.shape[1], _psf_arg(p), R, float(sky), float(gain),
                                             float(readnoise), float(damp), _ptr(out), _stream()))
    return out


def deconv_update(u, ratio, inv, psf, out=None):
    """Step 4 of F12: u' = (u q) inv where inv != 0, else u, with q the back-projection (correlation) of the ratio plane."""
    u = _image_f32(u, 'u')
    ratio, inv = _plane_like(ratio, 'ratio', u), _plane_like(inv, 'inv', u)
    p, R = psf_stamp(psf)
    out = _out_f32(out, u, ratio)
    check(_lib.load().apgpu_deconv_update_f32(_ptr(u), _ptr(ratio), _ptr(inv), u.shape[0], u.shape[1], _psf_arg(p), R, _ptr(out), _stream()))
    return out


def deconv_workspace(shape, device):
    """A workspace for richardson_lucy on images of this shape (16 bytes per pixel: the ratio, the norm and two estimates)."""
    return torch.empty(_lib.load().apgpu_deconv_ws_bytes(int(shape[0]), int(shape[1])), dtype=torch.uint8, device=device)


def richardson_lucy(data, psf, sky, niter=30, damp=0.0, gain=1.0, readnoise=0.0, start=None, min_weight=0.1, ws=None, out=None):
    """Damped Richardson-Lucy deconvolution of a float32 image [H, W] whose non-finite pixels mean "no data" (include/apgpu.h F12;
    tests/deconvolve_model.py).  psf: an odd, square stamp of radius <= 12, its weights used as given.  sky: the level (ADU) that is
    not deconvolved.  damp: White's threshold T in sigma (0: plain RL); gain (e-/ADU) and readnoise (ADU) give the variance it is
    measured in.  start: a positive scalar, a plane of the image shape, or None: the float64 mean of data - sky over the valid
    pixels, at least 1e-6.  ws: a uint8 device workspace (deconv_workspace) or None; out: the output tensor or None.  1 + 2 niter
    launches on the current stream, nothing else inside the loop.

    Returns (image, report): the image is the estimate plus the sky, NaN where the input has no data; report['start'] is the start
    level that was used (a float32 value, None for a plane)."""
    import math
    data = _image_f32(data)
    p, R = psf_stamp(psf)
    niter = int(niter)
    if niter < 0:
        raise ValueError('niter must be >= 0, got %d' % niter)
    plane, level = None, None
    if start is not None and np.ndim(start) != 0:
        plane = _plane_like(start, 'start', data)
    else:
        if start is None:
            ok = torch.isfinite(data)
            cnt = int(ok.sum().item())
            mean = float(torch.where(ok, data.to(torch.float64) - float(np.float32(sky)), 0.0).sum().item()) / cnt if cnt else 0.0
            start = max(mean, 1e-6)
        level = float(np.float32(start))
        if not (level > 0.0 and math.isfinite(level)):
            raise ValueError('the start level must be finite and > 0, got %r' % (start,))
    out = _out_f32(out, data, data, *(() if plane is None else (plane,)))
    lib = _lib.load()
    ws = _workspace(ws, lib.apgpu_deconv_ws_bytes(data.shape[0], data.shape[1]), data.device, 'deconv_workspace')
    check(lib.apgpu_richardson_lucy_f32(_ptr(data), data.shape[0], data.shape[1], _psf_arg(p), R, float(sky), float(gain), float(readnoise),
                                        float(damp), niter, 0.0 if level is None else level, _ptr(plane), float(min_weight), _ptr(out),
                                        _ptr(ws), ws.numel(), _stream()))
    report = dict(start=level, niter=niter, radius=R, damp=float(damp), sky=float(np.float32(sky)), gain=float(gain), readnoise=float(readnoise),
                  min_weight=float(min_weight), launches=1 + 2 * niter)
    return out, report


# ------------------------------------------------------------------------------------------------------------------
# F13: ApMultiscale - starlet (B3-spline a trous) denoise and sharpen (csrc/multiscale.hip; the reference has no such
# stage: the arithmetic is this project's definition, include/apgpu.h F13, tests/multiscale_model.py)
STARLET_MAX_SCALES = _lib.STARLET_MAX_SCALES
STARLET_TAPS = np.array([1.0, 4.0, 6.0, 4.0, 1.0], np.float64) / 16.0


def starlet_noise_constants(J):
    """float64 [J]: the standard deviation of the planes w_1 .. w_J for unit white noise far from borders and holes, computed from
    the taps as the 2-norm of each plane's impulse response."""
    import math
    J = _starlet_scales(J)
    kern, out = np.ones(1), []
    for j in range(J):
        up = np.zeros(4 * (1 << j) + 1)
        up[::1 << j] = STARLET_TAPS
        nxt = np.convolve(kern, up)                                          # the impulse response of c_{j+1} along one axis
        prev = np.pad(kern, (nxt.size - kern.size) // 2)
        plane = np.outer(prev, prev) - np.outer(nxt, nxt)
        out.append(math.sqrt(float((plane * plane).sum())))
        kern = nxt
    return np.array(out)


def _starlet_scales(J):
    if int(J) != J or not 1 <= int(J) <= STARLET_MAX_SCALES:
        raise ValueError('the number of scales must be 1 .. %d, got %r' % (STARLET_MAX_SCALES, J))
    return int(J)


def _starlet_per_scale(v, J, name):
    v = np.asarray(v, np.float64).reshape(-1)
    if v.size == 1:
        v = np.repeat(v, J)
    if v.size != J:
        raise ValueError('%s needs one value or %d (one per scale), got %d' % (name, J, v.size))
    return v


def _starlet_mode(mode):
    if mode not in _lib.STARLET_MODE:
        raise ValueError('Unexpected mode %r. Allowed values are: %s' % (mode, sorted(_lib.STARLET_MODE)))
    return _lib.STARLET_MODE[mode]


def starlet_workspace(shape, device):
    """A workspace for starlet_planes and multiscale on images of this shape (8 bytes per pixel: the two ping-pong planes)."""
    return torch.empty(_lib.load().apgpu_starlet_ws_bytes(int(shape[0]), int(shape[1])), dtype=torch.uint8, device=device)


def starlet_step(c, spacing, out=None, plane=None, acc=None, threshold=0.0, gain=1.0, g_res=1.0, mode='hard', first=True, last=False,
                 form='auto'):
    """One launch of F13: c_j -> c_{j+1} at `spacing` = 2^j (1 .. 32) by normalised convolution with the B3 taps, NaN / inf pixels
    being holes that stay NaN.  out: the tensor for c_{j+1} (None: a new one; False: not wanted).  plane: a tensor that receives
    w_{j+1} = c_j - c_{j+1}.  acc: the accumulator of the reconstruction: written as +0 + gain T(w) when `first`, else added to;
    `last` adds g_res c_{j+1} on top.  form: 'auto', 'tile' (spacing <= 8) or 'direct': the same bits either way.
    Returns c_{j+1} (None with out=False)."""
    c = _image_f32(c, 'c')
    if form not in _lib.STARLET_FORM:
        raise ValueError('Unexpected form %r. Allowed values are: %s' % (form, sorted(_lib.STARLET_FORM)))
    if out is None:
        out = torch.empty_like(c)
    elif out is False:
        out = None
    for t in (out, plane, acc):
        if t is not None:
            _out_f32(t, c, name='out, plane and acc each')
    flags = (_lib.STARLET_FIRST if first else 0) | (_lib.STARLET_LAST if last else 0)
    check(_lib.load().apgpu_starlet_step_f32(_ptr(c), c.shape[0], c.shape[1], int(spacing), _ptr(out), _ptr(plane), _ptr(acc),
                                             float(threshold), float(gain), float(g_res), _starlet_mode(mode), flags, _lib.STARLET_FORM[form],
                                             _stream()))
    return out


def starlet_plane1(image, out=None):
    """w_1 = c_0 - c_1 alone (one launch): the plane the image noise is measured in."""
    image = _image_f32(image, 'image')
    out = _out_f32(out, image, image)
    check(_lib.load().apgpu_starlet_plane1_f32(_ptr(image), image.shape[0], image.shape[1], _ptr(out), _stream()))
    return out


def starlet_planes(image, J=4, ws=None, out=None):
    """The transform itself: a float32 tensor [J + 1, H, W] holding w_1 .. w_J and the smooth residual c_J; their float32 sum in
    this order is the image to within rounding.  Holes (NaN / inf pixels) are NaN in every plane.  J launches."""
    image = _image_f32(image, 'image')
    J = _starlet_scales(J)
    out = _out_f32(out, image, shape=(J + 1,) + tuple(image.shape))
    ws = _workspace(ws, _lib.load().apgpu_starlet_ws_bytes(image.shape[0], image.shape[1]), image.device, 'starlet_workspace')
    check(_lib.load().apgpu_starlet_planes_f32(_ptr(image), image.shape[0], image.shape[1], J, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def starlet_sigma(image):
    """The image noise: the clipped standard deviation (sigma 3, 5 iterations) of plane 1 over the noise constant of plane 1.
    NaN when plane 1 has no finite pixel."""
    std = float(sigclip_global(starlet_plane1(image), 3.0, maxiters=5).cpu().numpy()[2])
    return std / float(starlet_noise_constants(1)[0])


def multiscale(image, J=4, k=(3.0, 3.0, 2.0, 1.0), gains=1.0, g_res=1.0, mode='hard', sigma=None, ws=None, out=None):
    """Noise reduction and sharpening by scale of a float32 image [H, W] whose NaN / inf pixels are holes (include/apgpu.h F13;
    tests/multiscale_model.py): plane j of the starlet transform is cut at t_j = float32(k_j sigma sigma_e[j-1]) ('hard': smaller
    coefficients become 0; 'soft': all shrink by t_j; k_j = 0: untouched), weighted by gains[j-1] and summed with g_res times the
    smooth residual.  k, gains: one value per scale, or one for all.  sigma: the image noise; None measures it (starlet_sigma) and
    raises RuntimeError when that gives no finite value.  ws: a uint8 device workspace (starlet_workspace) or None; out: the output
    tensor or None.  J launches on the current stream, nothing else inside the loop.

    Returns (image, report): report has sigma, t (float32 [J]), J, mode, k, gains, g_res."""
    import math
    image = _image_f32(image, 'image')
    J = _starlet_scales(J)
    k, gains = _starlet_per_scale(k, J, 'k'), _starlet_per_scale(gains, J, 'gains')
    if not np.all(k >= 0.0) or not np.all(np.isfinite(k)):
        raise ValueError('the thresholds k must be finite and >= 0, got %s' % (k.tolist(),))
    g = gains.astype(np.float32)
    gr = np.float32(g_res)
    if not np.all(np.isfinite(g)) or not np.isfinite(gr):
        raise ValueError('the gains must be finite, got %s and %r' % (gains.tolist(), g_res))
    m = _starlet_mode(mode)
    if sigma is None:
        sigma = starlet_sigma(image)
        if not math.isfinite(sigma):
            raise RuntimeError('Could not measure the noise of the image (plane 1 has no finite standard deviation): pass sigma.')
    sigma = float(sigma)
    if not (sigma >= 0.0 and math.isfinite(sigma)):
        raise ValueError('sigma must be finite and >= 0, got %r' % sigma)
    se = starlet_noise_constants(J)
    t = np.array([np.float32(float(k[j]) * sigma * float(se[j])) for j in range(J)], np.float32)
    if not np.all(np.isfinite(t)):
        raise ValueError('the thresholds overflow float32: %s' % (t.tolist(),))
    out = _out_f32(out, image, image)
    ws = _workspace(ws, _lib.load().apgpu_starlet_ws_bytes(image.shape[0], image.shape[1]), image.device, 'starlet_workspace')
    check(_lib.load().apgpu_multiscale_f32(_ptr(image), image.shape[0], image.shape[1], J, t.ctypes.data_as(C.POINTER(C.c_float)),
                                           g.ctypes.data_as(C.POINTER(C.c_float)), float(gr), m, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out, dict(sigma=sigma, t=t, J=J, mode=mode, k=k, gains=g.astype(np.float64), g_res=float(gr))


# ------------------------------------------------------------------------------------------------------------------
# F14: ApDrizzle - drizzle co-add of dithered frames and its blot-and-compare rejection (csrc/drizzle.hip; the reference
# has no such stage: the arithmetic is this project's definition, include/apgpu.h F14, tests/drizzle_model.py)
DRIZZLE_TILE_H, DRIZZLE_TILE_W = _lib.DRIZZLE_TILE_H, _lib.DRIZZLE_TILE_W


def _drizzle_frames(frames):
    _need_cuda(frames)
    frames = _f32c(frames, 'frames')
    if frames.dim() == 2:
        frames = frames[None]
    if frames.dim() != 3 or frames.numel() == 0:
        raise ValueError('frames must be [N,H,W] or [H,W]')
    return frames


def _drizzle_tile_shape(shape):
    """The grid of 16 x 64 pixel tiles over an image: the per-tile transforms of drizzle (output tiles) and drizzle_reject (input)."""
    return -(-int(shape[0]) // 16), -(-int(shape[1]) // 64)


def _drizzle_affines(affines, N, tile_shape=None):
    """float64 numpy [N, 6]: one transform per frame - or, when `affines` is [N, ty, tx, 6], [N ty tx, 6]: one per frame and tile of
    the grid `tile_shape` (checked).  -> (transforms, per_tile)."""
    a = np.array(torch.as_tensor(affines, dtype=torch.float64).cpu().numpy(), dtype=np.float64)
    if a.ndim == 4:
        if tile_shape is None or tuple(a.shape) != (N,) + tuple(tile_shape) + (6,):
            raise ValueError('per-tile transforms must be [N, %s, %s, 6] (tiles of 16 x 64 pixels), got %s'
                             % (tile_shape[0] if tile_shape else '?', tile_shape[1] if tile_shape else '?', a.shape))
        if not np.all(np.isfinite(a)):
            raise ValueError('the transforms must be finite')
        return a.reshape(-1, 6), True
    return _drizzle_frame_affines(a, N), False


def _drizzle_frame_affines(a, N):
    a = a.reshape(-1, 6)
    if a.shape[0] == 1 and N > 1:
        a = np.repeat(a, N, 0)
    if a.shape[0] != N:
        raise ValueError('affines must hold one 2x3 transform per frame')
    if not np.all(np.isfinite(a)):
        raise ValueError('the transforms must be finite')
    return a


def _drizzle_f32n(x, N, name, default):
    """One float32 value per frame (float64 -> float32 as numpy casts), on the host."""
    if x is None:
        return np.full(N, default, np.float32)
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    x = np.asarray(x, np.float64).reshape(-1)
    if x.size == 1 and N > 1:
        x = np.repeat(x, N)
    if x.size != N:
        raise ValueError('%s must hold one value per frame' % name)
    return x.astype(np.float32)


def drizzle_out_shape(in_shape, scale):
    """The default output grid: ceil(scale H) x ceil(scale W), the reference grid at `scale` pixels per pixel."""
    import math
    return int(math.ceil(int(in_shape[0]) * float(scale))), int(math.ceil(int(in_shape[1]) * float(scale)))


def drizzle_affines(affines, scale):
    """float64 numpy [N, 6]: the transforms of the grid with `scale` output pixels per reference pixel, output pixel (u, v) at
    reference coordinate ((u + 0.5) / s - 0.5, (v + 0.5) / s - 0.5): oversampled_affines for any s > 0."""
    import math
    s = float(scale)
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError('scale must be a positive number, got %r' % (scale,))
    a = np.array(affines, dtype=np.float64).reshape(-1, 6)
    off = 0.5 / s - 0.5
    fine = a.copy()
    fine[:, 0] = a[:, 0] / s
    fine[:, 1] = a[:, 1] / s
    fine[:, 2] = a[:, 2] + (a[:, 0] + a[:, 1]) * off
    fine[:, 3] = a[:, 3] / s
    fine[:, 4] = a[:, 4] / s
    fine[:, 5] = a[:, 5] + (a[:, 3] + a[:, 4]) * off
    return fine


def drizzle(frames, affines, scale=2.0, pixfrac=0.5, fscale=None, weights=None, mask=None, frame_masks=None, out_shape=None,
            conserve_flux=False, cfa=None):
    """Drizzle co-add (variable-pixel linear reconstruction, "turbo" footprint, gather form) of [N,H,W] float32 frames onto a grid of
    `scale` output pixels per reference pixel, in one launch (include/apgpu.h F14).

    affines: one 2x3 float64 transform per frame, reference pixel -> input pixel, as resample_affine takes them (ap_register writes
    them); or [N, ty, tx, 6], one per frame and 16 x 64 tile of the OUTPUT, reference pixel -> input pixel about that tile
    (poly_tile_affines(..., composed=False): a lens distortion): footprint, weight and flux factor are then the tile's own.  pixfrac: the side of a drop in input pixels, (0, 1].  fscale: per-frame flux scale; conserve_flux also multiplies by
    |det| of the composed transform (surface brightness otherwise).  weights: one finite, positive weight per frame (None: 1).
    mask [H,W] / frame_masks [N,H,W]: non-zero = bad pixel.  out_shape: (h, w) of the output, default drizzle_out_shape.  cfa:
    (pattern, channel) - only pixels of that colour feed the plane: pattern as bayer_pattern gives it, channel 0 (R), 1 (G, both
    greens) or 2 (B).  The footprint of an output pixel must be within (0, 2] input pixels per axis (ValueError).

    Returns dict(image, weight): float32 [h, w]; image NaN and weight 0 where no drop reaches."""
    import math
    frames = _drizzle_frames(frames)
    N, H, W = frames.shape
    dev = frames.device
    p = np.float32(pixfrac)
    if not (p > 0 and p <= 1):
        raise ValueError('pixfrac must be in (0, 1], got %r' % (pixfrac,))
    h, wo = drizzle_out_shape((H, W), scale) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
    if h < 1 or wo < 1:
        raise ValueError('out_shape must be positive, got %r' % (out_shape,))
    A, per_tile = _drizzle_affines(affines, N, _drizzle_tile_shape((h, wo)))
    A = drizzle_affines(A, scale)
    if not np.all(np.isfinite(A)):
        raise ValueError('the transforms must be finite')
    hx, hy = 0.5 * np.hypot(A[:, 0], A[:, 3]), 0.5 * np.hypot(A[:, 1], A[:, 4])
    lx, ly = 2.0 * hx, 2.0 * hy
    if not (np.all(lx > 0.0) and np.all(lx <= 2.0) and np.all(ly > 0.0) and np.all(ly <= 2.0)):
        raise ValueError('the footprint of an output pixel must be within (0, 2] input pixels per axis, got %s x %s: '
                         'use a larger scale' % ((lx.tolist(), ly.tolist()) if not per_tile else
                                                 ('%g .. %g' % (lx.min(), lx.max()), '%g .. %g over the tiles' % (ly.min(), ly.max()))))
    fs = _drizzle_f32n(fscale, N, 'fscale', 1.0)
    w = _drizzle_f32n(weights, N, 'weights', 1.0)
    if not np.all(np.isfinite(fs)):
        raise ValueError('fscale must be finite')
    if not (np.all(np.isfinite(w)) and np.all(w > 0)):
        raise ValueError('weights must be finite and positive')
    if per_tile:                                                         # a frame's values, once per tile of the frame
        fs, w = np.repeat(fs, A.shape[0] // N), np.repeat(w, A.shape[0] // N)
    g = fs
    if conserve_flux:
        g = (fs.astype(np.float64) * np.abs(A[:, 0] * A[:, 4] - A[:, 1] * A[:, 3])).astype(np.float32)
    if not np.all(np.isfinite(g)):
        raise ValueError('the flux factors overflow float32')
    mk = _mask_u8(mask, (H, W), 'mask must be [H,W]')
    fm = _mask_u8(frame_masks, (N, H, W), 'frame_masks must be [N,H,W]')
    pat, channel = None, 0
    if cfa is not None:
        pattern, channel = cfa
        pat = (C.c_int32 * 4)(*bayer_pattern(pattern))
        if isinstance(channel, bool) or int(channel) != channel or int(channel) not in (0, 1, 2):
            raise ValueError('the cfa channel must be 0 (R), 1 (G) or 2 (B), got %r' % (channel,))
    prm = np.concatenate([A, hx[:, None], hy[:, None], w.astype(np.float64)[:, None], g.astype(np.float64)[:, None]], 1)
    prm = torch.from_numpy(np.ascontiguousarray(prm)).to(dev)
    image = torch.empty((h, wo), dtype=torch.float32, device=dev)
    weight = torch.empty((h, wo), dtype=torch.float32, device=dev)
    lib = _lib.load()
    entry = lib.apgpu_drizzle_tiles_f32 if per_tile else lib.apgpu_drizzle_f32
    check(entry(_ptr(frames), N, H, W, _ptr(mk), _ptr(fm), _ptr(prm), float(p), pat, int(channel), _ptr(image), _ptr(weight), h, wo, _stream()))
    return dict(image=image, weight=weight)


def drizzle_reject(frames, affines, ref, ref_scale=1.0, fscale=None, sigmas=None, k=3.5, grow=1.2):
    """Blot-and-compare outlier flags for drizzle (the driz_cr step): every pixel of every frame is compared with the bilinear value
    b of the reference image `ref` under it; flagged when |g v - b| > k sigma_i + grow d, d being the spread of the four reference
    pixels b comes from (it keeps undersampled star cores from being flagged).  ref: float32 [hr, wr] on the grid with `ref_scale`
    pixels per reference pixel (a median co-add at 1, a first drizzle at its scale), in flux-scaled units.  sigmas: per-frame noise in
    those units (fscale_i times the frame's clipped standard deviation).  Pixels under which the reference is missing or not finite are not
    flagged.  affines: as drizzle's, or [N, ty, tx, 6], one per frame and 16 x 64 tile of the INPUT frame, reference pixel -> input
    pixel about the point that maps to that tile (poly_input_tile_affines).  Returns uint8 [N, H, W], 1 = outlier: drizzle's
    frame_masks."""
    import math
    frames = _drizzle_frames(frames)
    N, H, W = frames.shape
    dev = frames.device
    _need_cuda(ref)
    ref = _f32c(ref, 'ref')
    if ref.dim() != 2 or ref.numel() == 0:
        raise ValueError('ref must be [hr,wr]')
    rs = float(ref_scale)
    if not (math.isfinite(rs) and rs > 0.0):
        raise ValueError('ref_scale must be a positive number, got %r' % (ref_scale,))
    kf, gf = np.float32(k), np.float32(grow)
    if not (np.isfinite(kf) and np.isfinite(gf) and kf >= 0 and gf >= 0):
        raise ValueError('k and grow must be finite and >= 0, got %r and %r' % (k, grow))
    a, per_tile = _drizzle_affines(affines, N, _drizzle_tile_shape((H, W)))
    det = a[:, 0] * a[:, 4] - a[:, 1] * a[:, 3]
    if not np.all(np.isfinite(det)) or np.any(det == 0.0):
        raise ValueError('a transform is singular')
    inv = np.empty_like(a)
    inv[:, 0], inv[:, 1] = a[:, 4] / det, -a[:, 1] / det
    inv[:, 3], inv[:, 4] = -a[:, 3] / det, a[:, 0] / det
    inv[:, 2] = -(inv[:, 0] * a[:, 2] + inv[:, 1] * a[:, 5])
    inv[:, 5] = -(inv[:, 3] * a[:, 2] + inv[:, 4] * a[:, 5])
    B = inv * rs                                                          # reference coordinate x -> pixel (x + 0.5) rs - 0.5
    B[:, 2] += 0.5 * rs - 0.5
    B[:, 5] += 0.5 * rs - 0.5
    fs = _drizzle_f32n(fscale, N, 'fscale', 1.0)
    sg = _drizzle_f32n(sigmas, N, 'sigmas', 0.0)
    if not (np.all(np.isfinite(fs)) and np.all(np.isfinite(sg)) and np.all(sg >= 0)):
        raise ValueError('fscale must be finite and sigmas finite and >= 0')
    if per_tile:
        fs, sg = np.repeat(fs, a.shape[0] // N), np.repeat(sg, a.shape[0] // N)
    prm = np.concatenate([B, fs.astype(np.float64)[:, None], sg.astype(np.float64)[:, None]], 1)
    prm = torch.from_numpy(np.ascontiguousarray(prm)).to(dev)
    out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    entry = lib.apgpu_drizzle_reject_tiles_u8 if per_tile else lib.apgpu_drizzle_reject_u8
    check(entry(_ptr(frames), N, H, W, _ptr(prm), _ptr(ref), ref.shape[0], ref.shape[1], float(kf), float(gf), _ptr(out), _stream()))
    return out


# ------------------------------------------------------------------------------------------------------------------
# F19: lens distortion - polynomial maps (distortion.py) as the per-tile transforms the resample and drizzle kernels take
# (csrc/distortion.hip, DESIGN 4.3e')
def poly_tile_affines(maps, out_shape, tile_scale=1, scale=1.0, max_tile_error=0.01, composed=True, device='cuda'):
    """The linearisation of per-frame distortion maps (distortion.PolyMap, reference pixel -> input pixel; one degree, origin and
    scale) over the tiles of 16 tile_scale x 64 tile_scale pixels of an out_shape grid with `scale` pixels per reference pixel (grid
    pixel (u, v) at reference coordinate ((u + 0.5) / scale - 0.5, (v + 0.5) / scale - 0.5)): the map and its analytic Jacobian at
    the tile centre, written on the device.  scale 1: the co-add's grid, for resample_affine / coadd; OVERSAMPLING n: scale = n,
    tile_scale = n, for resample_oversampled(fine_affines=).  composed=False: transforms of REFERENCE pixels instead of grid pixels,
    what drizzle takes (it composes with its grid itself).

    Returns (float64 device tensor [N, tiles_y, tiles_x, 6], the largest PolyMap.tile_error estimate in input pixels); ValueError
    when the estimate exceeds max_tile_error."""
    import math
    maps = list(maps) if not isinstance(maps, tuple) else maps
    h, w = int(out_shape[0]), int(out_shape[1])
    ts, s = int(tile_scale), float(scale)
    if h < 1 or w < 1:
        raise ValueError('out_shape must be positive, got %r' % (out_shape,))
    if ts != tile_scale or not 1 <= ts <= 16:
        raise ValueError('tile_scale must be 1 .. 16, got %r' % (tile_scale,))
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError('scale must be a positive number, got %r' % (scale,))
    coef, degree, x0, y0, L = _poly_maps(maps, len(maps[0]) if isinstance(maps, tuple) else len(maps))
    from .distortion import PolyMap
    est = max(PolyMap(c[0], c[1], (x0, y0), L).tile_error((h, w), ts, s) for c in coef)
    if not est <= float(max_tile_error):
        raise ValueError('the tiles of %d x %d pixels linearise this map to %.3g input pixels, more than max_tile_error = %g'
                         % (64 * ts, 16 * ts, est, max_tile_error))
    N = coef.shape[0]
    ty, tx = -(-h // (16 * ts)), -(-w // (64 * ts))
    dev = torch.device(device)
    c = torch.from_numpy(np.ascontiguousarray(coef)).to(dev)
    out = torch.empty((N, ty, tx, 6), dtype=torch.float64, device=c.device)
    check(_lib.load().apgpu_poly_tile_affines(_ptr(c), N, degree, x0, y0, L, h, w, ts, s, int(bool(composed)), _ptr(out), _stream()))
    return out, est


def poly_input_tile_affines(maps, in_shape):
    """For drizzle_reject under distortion maps: float64 numpy [N, ty, tx, 6], per frame and 16 x 64 tile of the INPUT frame the
    transform reference pixel -> input pixel about the reference point p that maps to the tile centre c (PolyMap.inverse, host):
    the Jacobian at p, and the offset that takes p to c.  NaN where the inverse does not converge (drizzle_reject refuses it)."""
    maps = list(maps)
    ty, tx = _drizzle_tile_shape(in_shape)
    yc = np.arange(ty, dtype=np.float64)[:, None] * 16.0 + 7.5 + np.zeros((1, tx))
    xc = np.arange(tx, dtype=np.float64)[None, :] * 64.0 + 31.5 + np.zeros((ty, 1))
    out = np.empty((len(maps), ty, tx, 6))
    for m, o in zip(maps, out):
        px, py = m.inverse(xc, yc)
        a0, a1, a3, a4 = m.jacobian(px, py)
        o[...] = np.stack([a0, a1, (xc - a0 * px) - a1 * py, a3, a4, (yc - a3 * px) - a4 * py], axis=-1)
    return out


# ------------------------------------------------------------------------------------------------------------------
# F20: removal of the large-scale sky gradient (csrc/gradient.hip; the rule restated in tests/gradient_model.py).
# Device: the clipped statistics of the sample boxes, the surface on a lattice, the pass over the image.  Host: where the samples
# lie and the robust fit of the surface to them (float64, numpy).
GRADIENT_MODELS = tuple(_lib.SURFACE_MODEL)
GRADIENT_MODES = tuple(_lib.GRADIENT_MODE)
GRADIENT_MAX_SAMPLES, GRADIENT_MAX_RADIUS, GRADIENT_MAX_DEGREE = _lib.GRADIENT_MAX_SAMPLES, _lib.GRADIENT_MAX_RADIUS, _lib.GRADIENT_MAX_DEGREE
GRADIENT_MIN_STEP, GRADIENT_MAX_STEP = _lib.GRADIENT_MIN_STEP, _lib.GRADIENT_MAX_STEP


def _image_shape(shape):
    H, W = (int(s) for s in shape)
    if H < 1 or W < 1:
        raise ValueError('the image shape must be positive, got %r' % (tuple(shape),))
    return H, W


def surface_frame(shape):
    """(x0, y0, L) of the normalised coordinates u = (x - x0) / L, v = (y - y0) / L of an image [H, W]."""
    H, W = _image_shape(shape)
    return (W - 1) / 2.0, (H - 1) / 2.0, max(W, H) / 2.0


def _centres(centres):
    c = centres.cpu().numpy() if torch.is_tensor(centres) else np.asarray(centres)
    if c.size == 0:
        c = c.reshape(0, 2)
    if c.ndim != 2 or c.shape[1] != 2:
        raise ValueError('centres must be [K, 2] (x, y), got shape %s' % (c.shape,))
    if c.shape[0] > GRADIENT_MAX_SAMPLES:
        raise ValueError('%d samples, at most %d' % (c.shape[0], GRADIENT_MAX_SAMPLES))
    ci = np.rint(c).astype(np.int64)
    if not np.array_equal(ci, c) or (ci.size and (ci.min() < -2 ** 31 or ci.max() >= 2 ** 31)):
        raise ValueError('the centres must be whole pixels')
    return np.ascontiguousarray(ci, np.int32)


def _radius(radius):
    r = int(radius)
    if r != radius or not 0 <= r <= GRADIENT_MAX_RADIUS:
        raise ValueError('the box radius must be a whole number in 0 .. %d, got %r' % (GRADIENT_MAX_RADIUS, radius))
    return r


def _step(step):
    s = int(step)
    if s != step or not GRADIENT_MIN_STEP <= s <= GRADIENT_MAX_STEP:
        raise ValueError('the lattice step must be a whole number in %d .. %d, got %r' % (GRADIENT_MIN_STEP, GRADIENT_MAX_STEP, step))
    return s


def exclude_samples(xy, exclude=()):
    """bool [K]: the centres xy [K, 2] (x, y) that lie in none of the `exclude` rectangles (x0, y0, x1, y1), bounds inclusive."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    keep = np.ones(len(xy), bool)
    for rect in exclude:
        if len(rect) != 4:
            raise ValueError('an excluded rectangle is x0, y0, x1, y1, got %r' % (rect,))
        x0, y0, x1, y1 = (float(t) for t in rect)
        keep &= ~((xy[:, 0] >= min(x0, x1)) & (xy[:, 0] <= max(x0, x1)) & (xy[:, 1] >= min(y0, y1)) & (xy[:, 1] <= max(y0, y1)))
    return keep


def gradient_samples(shape, samples_per_row=16, exclude=()):
    """Where the samples of an image [H, W] lie: int32 [K, 2] (x, y), a regular grid of samples_per_row columns with the same pitch
    W / samples_per_row in y, centred in the image, row by row; without the centres inside one of the `exclude` rectangles
    (x0, y0, x1, y1), bounds inclusive."""
    H, W = _image_shape(shape)
    n = int(samples_per_row)
    if n != samples_per_row or n < 1:
        raise ValueError('samples_per_row must be a whole number >= 1, got %r' % (samples_per_row,))
    pitch = W / float(n)
    rows = max(1, int(math.floor(H / pitch)))
    if n * rows > GRADIENT_MAX_SAMPLES:
        raise ValueError('%d x %d samples, at most %d' % (rows, n, GRADIENT_MAX_SAMPLES))
    xs = np.floor((W - 1) / 2.0 + (np.arange(n) - (n - 1) / 2.0) * pitch + 0.5)
    ys = np.floor((H - 1) / 2.0 + (np.arange(rows) - (rows - 1) / 2.0) * pitch + 0.5)
    xy = np.stack([np.tile(xs, rows), np.repeat(ys, n)], axis=1)
    return np.ascontiguousarray(xy[exclude_samples(xy, exclude)], np.int32)


def sample_pixels(shape, centres, radius):
    """int64 [K]: the pixels of each sample box that lie inside an image [H, W]."""
    H, W = _image_shape(shape)
    c, r = _centres(centres).astype(np.int64), _radius(radius)
    nx = np.clip(np.minimum(c[:, 0] + r, W - 1) - np.maximum(c[:, 0] - r, 0) + 1, 0, None)
    ny = np.clip(np.minimum(c[:, 1] + r, H - 1) - np.maximum(c[:, 1] - r, 0) + 1, 0, None)
    return nx * ny


def sample_clipped_stats(data, mask, centres, radius, sigma=3.0, maxiters=5):
    """astropy's SigmaClip(sigma, maxiters) median / std of the square boxes of half-size `radius` (0 .. 32) about `centres` [K, 2]
    (x, y; whole pixels, K <= 4096, anywhere - a box is clipped at the image edge): float64 device tensor [K, 4] = median, std,
    survivors, pixels of the (2 radius + 1)^2 that were outside the image, masked (mask != 0) or not finite.  A box without a
    survivor: NaN, NaN, 0.  The contract of box_clipped_stats, the boxes taken from a list; the std is np.nanstd of the survivors in the
    box's row-major order, bit for bit."""
    c, r = _centres(centres), _radius(radius)
    if not float(sigma) >= 0.0 or int(maxiters) < 0:
        raise ValueError('sigma must be >= 0 and maxiters >= 0, got %r, %r' % (sigma, maxiters))
    data = _image_f32(data)
    mask = _mask_u8(mask, data.shape, 'mask must have the image shape')
    K = c.shape[0]
    out = torch.empty((K, 4), dtype=torch.float64, device=data.device)
    cd = torch.from_numpy(c).to(data.device)
    check(_lib.load().apgpu_sample_clipped_stats_f32(_ptr(data), _ptr(mask), data.shape[0], data.shape[1], _ptr(cd) if K else None, K, r,
                                                     float(sigma), int(maxiters), _ptr(out) if K else None, _stream()))
    return out


def _poly_terms(degree):
    return [(t - j, j) for t in range(degree + 1) for j in range(t + 1)]


def _poly_design(u, v, degree):
    """[n, P]: u^i v^j in the coefficient order of the kernels (by total degree t, within t by j, i = t - j), the powers by repeated
    multiplication."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    pu, pv = [np.ones_like(u)], [np.ones_like(v)]
    for _ in range(degree):
        pu.append(pu[-1] * u)
        pv.append(pv[-1] * v)
    return np.stack([pu[i] * pv[j] for i, j in _poly_terms(degree)], axis=-1)


def _tps_phi(q):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(q == 0.0, 0.0, 0.5 * q * np.log(q))


def _surface_arg(surface):
    if not isinstance(surface, dict) or surface.get('model') not in GRADIENT_MODELS:
        raise ValueError('Unexpected surface model %r. Allowed models are: %s' % (surface.get('model') if isinstance(surface, dict) else surface,
                                                                               list(GRADIENT_MODELS)))
    x0, y0, L = (float(t) for t in surface['frame'])
    if not (math.isfinite(x0) and math.isfinite(y0) and math.isfinite(L) and L > 0.0):
        raise ValueError('the frame of a surface is finite x0, y0 and L > 0, got %r' % (surface['frame'],))
    if surface['model'] == 'poly':
        d = int(surface['degree'])
        coef = np.ascontiguousarray(surface['coef'], np.float64).reshape(-1)
        if not 1 <= d <= GRADIENT_MAX_DEGREE or coef.size != (d + 1) * (d + 2) // 2:
            raise ValueError('a polynomial surface has a degree in 1 .. %d and (d + 1)(d + 2) / 2 coefficients, got degree %r and %d'
                             % (GRADIENT_MAX_DEGREE, surface['degree'], coef.size))
        return 'poly', (x0, y0, L), d, coef, None
    a = np.asarray(surface['a'], np.float64).reshape(-1)
    w = np.asarray(surface['w'], np.float64).reshape(-1)
    uv = np.ascontiguousarray(surface['uv'], np.float64).reshape(-1, 2)
    if a.size != 3 or uv.shape[0] != w.size or w.size > GRADIENT_MAX_SAMPLES:
        raise ValueError('a thin-plate surface has a [3], w [K] and uv [K, 2] with K <= %d, got %d, %d and %s'
                         % (GRADIENT_MAX_SAMPLES, a.size, w.size, uv.shape))
    return 'tps', (x0, y0, L), w.size, np.ascontiguousarray(np.concatenate([a, w])), uv


def surface_eval(surface, x, y):
    """The surface itself (not its lattice interpolant) at pixel coordinates x, y, on the host in float64."""
    kind, (x0, y0, L), n, params, uv = _surface_arg(surface)
    u, v = (np.asarray(x, np.float64) - x0) / L, (np.asarray(y, np.float64) - y0) / L
    if kind == 'poly':
        return _poly_design(u, v, n) @ params
    q = (u[..., None] - uv[:, 0]) ** 2 + (v[..., None] - uv[:, 1]) ** 2
    return ((_tps_phi(q) @ params[3:] + params[0]) + params[1] * u) + params[2] * v


def surface_lattice(surface, shape, step=16, device='cuda'):
    """The surface at the nodes of the lattice of an image [H, W]: float64 device tensor [(H - 1) // step + 4, (W - 1) // step + 4],
    node (iy, ix) at pixel ((ix - 1) step, (iy - 1) step) - every pixel has its 4 x 4 nodes, the model is analytic outside the
    image.  surface: dict(model='poly', degree, coef, frame) or dict(model='tps', a, w, uv, frame), as fit_surface returns it."""
    kind, (x0, y0, L), n, params, uv = _surface_arg(surface)
    H, W = _image_shape(shape)
    s = _step(step)
    ny, nx = (H - 1) // s + 4, (W - 1) // s + 4
    dev = torch.device(device)
    p = torch.from_numpy(params).to(dev)
    c = torch.from_numpy(uv).to(dev) if uv is not None and n else None
    out = torch.empty((ny, nx), dtype=torch.float64, device=p.device)
    check(_lib.load().apgpu_surface_lattice_f64(_lib.SURFACE_MODEL[kind], _ptr(p), _ptr(c), n, x0, y0, L, s, ny, nx, _ptr(out), _stream()))
    return out


def surface_apply(data, lattice, step=16, mode='subtract', pedestal=0.0, out=None, surface_out=None):
    """One pass over a float32 image [H, W] with S the cubic-convolution interpolant (Keys, a = -1/2, float64) of `lattice` (float64
    device tensor, from surface_lattice): 'subtract' out = float32(d - S + pedestal), 'divide' out = float32(d / S pedestal) and NaN
    where S is not finite or <= 0; a pixel that is not finite stays NaN.  out may be data.  surface_out: None, True (a new plane) or a
    float32 plane of its own for float32(S).  Returns out, or (out, surface) with surface_out."""
    if mode not in GRADIENT_MODES:
        raise ValueError('Unexpected mode %r. Allowed modes are: %s' % (mode, list(GRADIENT_MODES)))
    s = _step(step)
    data = _image_f32(data)
    _need_cuda(lattice)
    H, W = data.shape
    ny, nx = (H - 1) // s + 4, (W - 1) // s + 4
    if lattice.dtype != torch.float64 or tuple(lattice.shape) != (ny, nx):
        raise ValueError('lattice must be a float64 tensor of shape %s for an image of %s at step %d, got %s %s'
                         % ((ny, nx), (H, W), s, lattice.dtype, tuple(lattice.shape)))
    if not math.isfinite(float(pedestal)):
        raise ValueError('the pedestal must be finite, got %r' % (pedestal,))
    lattice = lattice.contiguous()
    out = _out_f32(out, data)
    surf = None
    if surface_out is not None and surface_out is not False:
        surf = _out_f32(None if surface_out is True else surface_out, data, data, out, name='surface_out')
    check(_lib.load().apgpu_surface_apply_f32(_ptr(data), _ptr(lattice), H, W, ny, nx, s, _lib.GRADIENT_MODE[mode], float(pedestal), _ptr(out),
                                              _ptr(surf), _stream()))
    return out if surf is None else (out, surf)


def sample_sigmas(std, n):
    """sigma_k = 1.2533 std / sqrt(n), the standard error of a median; a sample whose std is 0 (a single pixel, a constant box) takes
    the smallest positive sigma of the others, 1 if there is none: its weight stays finite."""
    std, n = np.asarray(std, np.float64), np.asarray(n, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        sg = 1.2533 * std / np.sqrt(n)
    pos = np.isfinite(sg) & (sg > 0.0)
    floor = sg[pos].min() if pos.any() else 1.0
    return np.where(pos, sg, floor)


def _fit_poly(u, v, z, om, degree):
    A = _poly_design(u, v, degree)
    sw = np.sqrt(om)
    coef = np.linalg.lstsq(A * sw[:, None], z * sw, rcond=None)[0]
    return coef, A @ coef


def _fit_tps(u, v, z, om, smoothing):
    n = u.size
    Phi = _tps_phi((u[:, None] - u[None, :]) ** 2 + (v[:, None] - v[None, :]) ** 2)
    T = np.stack([np.ones(n), u, v], axis=1)
    M = np.zeros((n + 3, n + 3))
    M[:n, :n] = Phi + np.diag(smoothing * n * om.mean() / om)
    M[:n, n:] = T
    M[n:, :n] = T.T
    try:
        sol = np.linalg.solve(M, np.concatenate([z, np.zeros(3)]))
    except np.linalg.LinAlgError as exc:
        raise ValueError('the thin-plate system is singular (samples on one line?): %s' % exc) from None
    w, a = sol[:n], sol[n:]
    return w, a, Phi @ w + T @ a


def fit_surface(xy, values, sigmas, shape, model='poly', degree=3, smoothing=0.1, k_high=2.0, k_low=3.0, max_rounds=5, use=None):
    """The robust fit of a surface to samples, on the host in float64.  xy [K, 2] pixel coordinates, values [K], sigmas [K] (> 0; the
    weights are 1 / sigma^2), shape the image's, use [K] bool (None: every finite sample).
      'poly'  total degree 1 .. 6 in u, v by weighted least squares
      'tps'   S = a0 + a1 u + a2 v + sum w_k phi(q_k), phi = r^2 log r, with sum w = sum w u = sum w v = 0 and
              smoothing n mean(omega) / omega_k on the diagonal (0 interpolates, a large value tends to the weighted plane)
    After a fit sigma_r = 1.4826 median |r - median r| of the kept samples' residuals r = value - S; samples with r > k_high sigma_r
    or r < -k_low sigma_r are dropped for good and the rest is fitted again, at most max_rounds times.  ValueError when fewer than
    P + 3 samples (poly, P parameters) or 8 (tps) are left.
    Returns (surface: a dict for surface_lattice / surface_eval, kept [K] bool, sigma_r of the last fit)."""
    if model not in GRADIENT_MODELS:
        raise ValueError('Unexpected model %r. Allowed models are: %s' % (model, list(GRADIENT_MODELS)))
    frame = surface_frame(shape)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    z, sg = np.asarray(values, np.float64).reshape(-1), np.asarray(sigmas, np.float64).reshape(-1)
    if not (xy.shape[0] == z.size == sg.size):
        raise ValueError('xy [K, 2], values [K] and sigmas [K] must agree, got %s, %d and %d' % (xy.shape, z.size, sg.size))
    if model == 'poly':
        d = int(degree)
        if d != degree or not 1 <= d <= GRADIENT_MAX_DEGREE:
            raise ValueError('the degree must be a whole number in 1 .. %d, got %r' % (GRADIENT_MAX_DEGREE, degree))
        need = (d + 1) * (d + 2) // 2 + 3
    else:
        need = 8
        if not float(smoothing) >= 0.0:
            raise ValueError('the smoothing must be >= 0, got %r' % (smoothing,))
    if not (float(k_high) > 0.0 and float(k_low) > 0.0) or int(max_rounds) < 0:
        raise ValueError('k_high and k_low must be > 0 and max_rounds >= 0, got %r, %r, %r' % (k_high, k_low, max_rounds))
    ok = np.isfinite(z) & np.isfinite(sg) & (sg > 0.0) & np.isfinite(xy).all(axis=1)
    kept = ok if use is None else ok & np.asarray(use, bool).reshape(-1)
    kept = kept.copy()
    u, v = (xy[:, 0] - frame[0]) / frame[2], (xy[:, 1] - frame[1]) / frame[2]
    om = np.zeros(z.size)
    om[ok] = 1.0 / sg[ok] ** 2
    for rnd in range(int(max_rounds) + 1):
        idx = np.flatnonzero(kept)
        if idx.size < need:
            raise ValueError('%d samples are left, the %s surface needs at least %d' % (idx.size, model, need))
        if model == 'poly':
            coef, fit = _fit_poly(u[idx], v[idx], z[idx], om[idx], d)
            surface = dict(model='poly', degree=d, coef=coef, frame=frame)
        else:
            w, a, fit = _fit_tps(u[idx], v[idx], z[idx], om[idx], float(smoothing))
            surface = dict(model='tps', a=a, w=w, uv=np.stack([u[idx], v[idx]], axis=1), frame=frame, smoothing=float(smoothing))
        res = z[idx] - fit
        sigma_r = 1.4826 * float(np.median(np.abs(res - np.median(res))))
        drop = (res > float(k_high) * sigma_r) | (res < -float(k_low) * sigma_r)
        if rnd == int(max_rounds) or not sigma_r > 0.0 or not drop.any():
            break
        kept[idx[drop]] = False
    return surface, kept, sigma_r


# ------------------------------------------------------------------------------------------------------------------
# F21: ApAstrometry - offline plate solving against a catalogue (csrc/astrometry.hip; astrometry.net absent, parity unpinned)
SOLVE_NOMINAL, SOLVE_NO_SOLUTION = 0, 2


def _f64_dev(a, name):
    t = torch.as_tensor(a)
    if t.dim() != 1:
        raise ValueError('%s must be one-dimensional, got shape %s' % (name, tuple(t.shape)))
    return t.to(device=t.device if t.is_cuda else 'cuda', dtype=torch.float64).contiguous()


def sky_project(ra, dec, centre, cos_rc=-1.0):
    """The standard coordinates (xi, eta: degrees, xi towards east; NaN behind the tangent plane) of stars (ra, dec: degrees, float64
    [n]) about centre = (ra0, dec0), with wcs.TanWcs.sky2pix's expressions in its order, and keep (uint8): 1 where ra and dec are
    finite, the star is in front of the plane and cos(its distance from the centre) >= cos_rc.  Device tensors."""
    ra, dec = _f64_dev(ra, 'ra'), _f64_dev(dec, 'dec')
    if ra.shape != dec.shape:
        raise ValueError('ra and dec must have one length, got %d and %d' % (ra.numel(), dec.numel()))
    n = int(ra.numel())
    xi, eta = torch.empty(n, dtype=torch.float64, device=ra.device), torch.empty(n, dtype=torch.float64, device=ra.device)
    keep = torch.empty(n, dtype=torch.uint8, device=ra.device)
    check(_lib.load().apgpu_sky_project(_ptr(ra), _ptr(dec), n, float(centre[0]), float(centre[1]), float(cos_rc), _ptr(xi), _ptr(eta),
                                        _ptr(keep), _stream()))
    return xi, eta, keep


def cell_select(x, y, cells, capacity=512):
    """Per cell (cells [C, 3] = centre x, centre y, half side) the first `capacity` stars of the list (x, y float64 [n], brightest
    first) inside the closed square |x - cx| <= half, |y - cy| <= half.  Returns (idx int32 [C, capacity]: ascending star indices,
    -1 in the unused slots; count int32 [C]; inside int32 [C]: the number of stars in the square where that is <= capacity, else
    some value above it).  Exact and the same on every run.  Device tensors."""
    x, y = _f64_dev(x, 'x'), _f64_dev(y, 'y')
    if x.shape != y.shape:
        raise ValueError('x and y must have one length, got %d and %d' % (x.numel(), y.numel()))
    cells = torch.as_tensor(np.asarray(cells.cpu() if torch.is_tensor(cells) else cells, np.float64).reshape(-1, 3)).to(x.device).contiguous()
    capacity = int(capacity)
    if not 1 <= capacity <= _lib.CELL_MAX_CAPACITY:
        raise ValueError('capacity = %d is outside 1 .. %d' % (capacity, _lib.CELL_MAX_CAPACITY))
    C_ = int(cells.shape[0])
    idx = torch.empty((C_, capacity), dtype=torch.int32, device=x.device)
    count, inside = torch.empty(C_, dtype=torch.int32, device=x.device), torch.empty(C_, dtype=torch.int32, device=x.device)
    check(_lib.load().apgpu_cell_select(_ptr(x), _ptr(y), int(x.numel()), _ptr(cells), C_, capacity, _ptr(idx), _ptr(count), _ptr(inside),
                                        _stream()))
    return idx, count, inside


def scale_levels(ratio):
    """The cell sides of the plate solver relative to min(nx, ny): geometric from 1 / ratio to ratio, 1 + 2 ceil(ln ratio / ln 1.3) of them."""
    m = int(math.ceil(math.log(ratio) / math.log(1.3) - 1e-9)) if ratio > 1.0 else 0
    return [float(ratio) ** ((k - m) / m) if m else 1.0 for k in range(2 * m + 1)]


def astrometry_cells(shape, scale, ratio, radius):
    """The search cells [C, 3] = (cx, cy, half side) in nominal pixels, and cos(Rc) of the catalogue cut."""
    ny, nx = shape
    r_px = radius * 3600.0 / scale
    out = []
    levels = scale_levels(ratio)
    for f in levels:
        L = f * min(nx, ny)
        stride = L / 2.0
        m = int(math.ceil(r_px / stride))
        out += [(ix * stride, iy * stride, L / 2.0) for iy in range(-m, m + 1) for ix in range(-m, m + 1)]
    rc = radius * math.sqrt(2.0) + (max(levels) * min(nx, ny) / 2.0) * math.sqrt(2.0) * scale / 3600.0
    return np.array(out, np.float64).reshape(-1, 3), math.cos(min(rc, 89.0) * math.pi / 180.0)


def _std_coords(ra, dec, crval):
    """Standard coordinates (degrees) about crval on the host: wcs.TanWcs.sky2pix's expressions."""
    r = math.pi / 180.0
    a, d, a0, d0 = ra * r, dec * r, np.float64(crval[0]) * r, np.float64(crval[1]) * r
    with np.errstate(divide='ignore', invalid='ignore'):
        cosc = np.sin(d0) * np.sin(d) + np.cos(d0) * np.cos(d) * np.cos(a - a0)
        xi = np.where(cosc > 0, np.cos(d) * np.sin(a - a0) / cosc, np.nan) / r
        eta = np.where(cosc > 0, (np.cos(d0) * np.sin(d) - np.sin(d0) * np.cos(d) * np.cos(a - a0)) / cosc, np.nan) / r
    return xi, eta


def _std_sky(xi, eta, crval):
    """... and back: wcs.TanWcs.pix2sky's."""
    r = math.pi / 180.0
    x, e, a0, d0 = np.float64(xi) * r, np.float64(eta) * r, np.float64(crval[0]) * r, np.float64(crval[1]) * r
    den = np.cos(d0) - e * np.sin(d0)
    ra = a0 + np.arctan2(x, den)
    dec = np.arctan2((e * np.cos(d0) + np.sin(d0)) * np.cos(ra - a0), den)
    return float(np.mod(ra / r, 360.0)), float(dec / r)


def _pair_rms(w, xy, ra, dec):
    px, py = w.sky2pix(ra, dec)
    return float(np.sqrt(np.mean((px - xy[:, 0]) ** 2 + (py - xy[:, 1]) ** 2)))


def tan_fit(xy, ra, dec, crpix, crval, max_iter=10, tol=1e-11):
    """The least-squares TAN WCS with the given CRPIX (FITS, 1-based) through pairs (pixel xy [n, 2], 0-based; ra, dec degrees),
    from the start CRVAL: project about CRVAL, fit xi and eta as affine functions of the offset from CRPIX, move CRVAL to the sky
    position of the constant terms, until they are below `tol` degrees.  Host float64.  -> (wcs.TanWcs, 2-D rms in pixels)."""
    from .wcs import TanWcs
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ra, dec = np.asarray(ra, np.float64), np.asarray(dec, np.float64)
    u, v = xy[:, 0] + 1.0 - crpix[0], xy[:, 1] + 1.0 - crpix[1]
    D = np.stack([u, v, np.ones_like(u)], axis=1)
    crval = (float(crval[0]), float(crval[1]))
    for _ in range(max_iter):
        xi, eta = _std_coords(ra, dec, crval)
        cx, cy = np.linalg.lstsq(D, xi, rcond=None)[0], np.linalg.lstsq(D, eta, rcond=None)[0]
        crval = _std_sky(cx[2], cy[2], crval)
        if math.hypot(cx[2], cy[2]) < tol:
            break
    w = TanWcs(crpix, crval, [[cx[0], cx[1]], [cy[0], cy[1]]])
    return w, _pair_rms(w, xy, ra, dec)


_SIP2, _SIP_INV = ((2, 0), (1, 1), (0, 2)), ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))


def _sip_fit(xy, ra, dec, tan, shape, rounds=2):
    """A, B of order 2 on top of `tan`, alternated with the TAN fit; AP, BP from a 16 x 16 grid."""
    from .wcs import SipWcs
    design = lambda p, q, terms: np.stack([p ** i * q ** j for i, j in terms], axis=1)
    crpix = (float(tan.crpix[0]), float(tan.crpix[1]))
    u, v = xy[:, 0] + 1.0 - crpix[0], xy[:, 1] + 1.0 - crpix[1]
    D, Dall = design(u, v, _SIP2), design(u, v, _SIP_INV)
    for _ in range(rounds):
        xi, eta = _std_coords(ra, dec, tan.crval)
        U = tan.cdinv[0, 0] * xi + tan.cdinv[0, 1] * eta
        V = tan.cdinv[1, 0] * xi + tan.cdinv[1, 1] * eta
        a = np.linalg.lstsq(Dall, U - u, rcond=None)[0][3:]                 # the constant and linear terms are the next TAN fit's
        b = np.linalg.lstsq(Dall, V - v, rcond=None)[0][3:]
        tan, _ = tan_fit(np.stack([xy[:, 0] + D @ a, xy[:, 1] + D @ b], axis=1), ra, dec, crpix, tan.crval)
    ny, nx = shape
    gx, gy = np.meshgrid(np.linspace(0.0, nx - 1.0, 16), np.linspace(0.0, ny - 1.0, 16))
    gu, gv = gx.ravel() + 1.0 - crpix[0], gy.ravel() + 1.0 - crpix[1]
    G = design(gu, gv, _SIP2)
    fu, fv = gu + G @ a, gv + G @ b
    Di = design(fu, fv, _SIP_INV)
    ap, bp = np.linalg.lstsq(Di, gu - fu, rcond=None)[0], np.linalg.lstsq(Di, gv - fv, rcond=None)[0]
    w = SipWcs(crpix, tan.crval, tan.cd, dict(zip(_SIP2, a)), dict(zip(_SIP2, b)), dict(zip(_SIP_INV, ap)), dict(zip(_SIP_INV, bp)))
    return w, _pair_rms(w, xy, ra, dec)


def _solve_rematch(w, xy, ra, dec, shape, match_radius, rms, fit, max_rounds=4):
    """mutual nearest neighbours of the image's stars and the catalogue's stars under the current WCS."""
    ny, nx = shape
    M = _lib.REGISTER_MAX_STARS
    pairs = None
    for rnd in range(max_rounds):
        radius = float(match_radius) if rnd == 0 else float(np.clip(3.0 * rms, 0.5, match_radius))
        px, py = w.sky2pix(ra, dec)
        with np.errstate(invalid='ignore'):
            near = np.flatnonzero((px >= -3.0) & (px <= nx - 1.0 + 3.0) & (py >= -3.0) & (py <= ny - 1.0 + 3.0))[:M]
        lists = [xy[:M], np.stack([px[near], py[near]], axis=1)]
        both = np.zeros((2, max(1, len(lists[0]), len(lists[1])), 2))
        for f, a in enumerate(lists):
            both[f, :len(a)] = a
        nm = nearest_match(both, [len(a) for a in lists], np.tile(np.asarray(REGISTER_IDENTITY), (2, 1)), radius)
        fwd, bwd = nm['fwd_idx'][1].cpu().numpy(), nm['bwd_idx'][1].cpu().numpy()
        i = np.nonzero(fwd >= 0)[0]
        i = i[bwd[fwd[i]] == i]
        new = np.stack([i, near[fwd[i]]], axis=1).astype(np.int64)
        if pairs is not None and np.array_equal(new, pairs):
            break
        pairs = new
        if len(pairs) < 3:
            break
        w, rms = fit(xy[pairs[:, 0]], ra[pairs[:, 1]], dec[pairs[:, 1]], w)
    return w, rms, pairs


def solve_field(xy, shape, catalogue, centre, scale, scale_err_ratio=1.3, radius=1.0, K=40, cell_stars=512, n_cand=5, match_radius=3.0,
                min_matched=10, use_sip=False):
    """Plate-solves one frame against a catalogue, given a hint.  xy [n, 2]: the image's stars, 0-based pixels, brightest
    first; shape (ny, nx); catalogue: a mapping with 'ra', 'dec' (degrees) and 'mag' (arrays or tensors of one length; rows with a
    non-finite value are dropped); centre (ra0, dec0): the hint; scale: the nominal arcsec per pixel, good to the factor
    scale_err_ratio; radius: how far (degrees) the true centre may be from the hint.

    The catalogue is projected about the hint (sky_project), put in brightness order and cut into overlapping square cells of a few
    sizes (cell_select); every cell's brightest K stars vote against the image's (triangle_build / triangle_vote with mirrored
    triangles allowed); the n_cand cells with the most votes are registered (register_lists); from the best candidate a TAN WCS is
    fitted on the sphere, refined by rematching all of the image's stars with all of the catalogue's (nearest_match), with SIP terms of
    order 2 when use_sip.  The fits are host float64.

    Returns a dict: status (SOLVE_NOMINAL or SOLVE_NO_SOLUTION: a status, not an error), wcs (wcs.TanWcs / wcs.SipWcs or None), pairs
    [n, 2] (image star, catalogue row), n_matched, rms (pixels), scale (arcsec / pixel), cell (the winning cell), cell_scale (true /
    nominal scale of its registration), parity (+1: east left of north as on the sky, -1 mirrored; 0 unsolved), n_seed, peak_votes
    [C], cells [C, 3] and candidates (a dict per registered cell)."""
    xy = np.asarray(xy.cpu() if torch.is_tensor(xy) else xy, np.float64).reshape(-1, 2)
    ny, nx = int(shape[0]), int(shape[1])
    scale, ratio = float(scale), float(scale_err_ratio)
    if not (scale > 0.0 and ratio >= 1.0 and radius > 0.0 and nx > 0 and ny > 0):
        raise ValueError('solve_field: scale and radius must be positive and scale_err_ratio >= 1')
    cells, cos_rc = astrometry_cells((ny, nx), scale, ratio, float(radius))
    ra, dec, mag = (_f64_dev(catalogue[k], k) for k in ('ra', 'dec', 'mag'))
    if not ra.shape == dec.shape == mag.shape:
        raise ValueError('solve_field: the catalogue columns must have one length')
    rows = torch.nonzero(torch.isfinite(ra) & torch.isfinite(dec) & torch.isfinite(mag)).reshape(-1)
    xi, eta, keep = sky_project(ra[rows], dec[rows], centre, cos_rc)
    kept = torch.nonzero(keep).reshape(-1)
    order = torch.sort(mag[rows][kept], stable=True)[1]
    kept = kept[order]
    rows = rows[kept]
    X, Y = (-xi[kept]) * 3600.0 / scale, eta[kept] * 3600.0 / scale
    idx, count, _ = cell_select(X, Y, cells, cell_stars)
    half = min(nx, ny) / 2.0
    with np.errstate(invalid='ignore'):
        f0 = np.flatnonzero((np.abs(xy[:, 0] - (nx - 1) / 2.0) <= half) & (np.abs(xy[:, 1] - (ny - 1) / 2.0) <= half))[:cell_stars]
    C_ = len(cells)
    fxy = torch.zeros((1 + C_, int(cell_stars), 2), dtype=torch.float64, device=X.device)
    fxy[0, :len(f0)] = torch.from_numpy(xy[f0]).to(X.device)
    if C_ and X.numel():
        g = idx.clamp(min=0).long()
        fxy[1:] = torch.where((idx >= 0)[..., None], torch.stack([X[g], Y[g]], dim=-1), fxy[1:])
    fcount = torch.cat([torch.tensor([len(f0)], dtype=torch.int32, device=X.device), count])
    votes = triangle_vote(triangle_build(fxy, fcount, K, 5.0), 0.002, True)
    peak = votes[1:].reshape(C_, -1).amax(dim=1).cpu().numpy() if C_ else np.zeros(0, np.int32)
    out = dict(status=SOLVE_NO_SOLUTION, wcs=None, pairs=np.zeros((0, 2), np.int64), n_matched=0, rms=np.nan, scale=np.nan, cell=-1,
               cell_scale=np.nan, parity=0, n_seed=0, peak_votes=peak, cells=cells, candidates=[])
    best = None
    lo, hi = 1.0 / (1.02 * ratio), 1.02 * ratio
    for c in np.argsort(-peak.astype(np.int64), kind='stable')[:n_cand]:
        if peak[c] <= 0:
            continue
        sel = torch.tensor([0, 1 + int(c)], device=X.device)
        r = register_lists(fxy[sel], fcount[sel], K, 0.002, 5.0, match_radius, 'affine', True)
        cand = dict(cell=int(c), ok=bool(r['ok'][1]), n_matched=int(r['n_matched'][1]), n_seed=int(r['n_seed'][1]), coeffs=r['coeffs'][1],
                    pairs=r['pairs'][1], scale=np.nan, counted=False)
        if cand['ok']:
            A = cand['coeffs']
            cand['scale'] = float(np.sqrt(abs(A[0] * A[4] - A[1] * A[3])))
            cand['counted'] = bool(lo <= cand['scale'] <= hi)
        out['candidates'].append(cand)
        if cand['counted'] and (best is None or (cand['n_matched'], -cand['cell']) > (best['n_matched'], -best['cell'])):
            best = cand
    if best is None:
        return out
    A = best['coeffs']
    out.update(cell=best['cell'], cell_scale=best['scale'], n_seed=best['n_seed'], parity=1 if A[0] * A[4] - A[1] * A[3] > 0 else -1)
    crpix = ((nx + 1) / 2.0, (ny + 1) / 2.0)
    c0 = _register_apply(A, np.array([[(nx - 1) / 2.0, (ny - 1) / 2.0]]))[0]
    crval = _std_sky(-c0[0] * scale / 3600.0, c0[1] * scale / 3600.0, (float(centre[0]), float(centre[1])))
    ra_k, dec_k = ra[rows].cpu().numpy(), dec[rows].cpu().numpy()
    cat = idx[best['cell']].cpu().numpy()[best['pairs'][:, 1]]
    w, rms = tan_fit(xy[f0[best['pairs'][:, 0]]], ra_k[cat], dec_k[cat], crpix, crval)
    fit = lambda p, a, d, w0: tan_fit(p, a, d, crpix, w0.crval)
    w, rms, pairs = _solve_rematch(w, xy, ra_k, dec_k, (ny, nx), match_radius, rms, fit)
    if use_sip and len(pairs) >= 12:
        sfit = lambda p, a, d, w0: _sip_fit(p, a, d, w0.tan(), (ny, nx))
        w, rms = sfit(xy[pairs[:, 0]], ra_k[pairs[:, 1]], dec_k[pairs[:, 1]], w)
        w, rms, pairs = _solve_rematch(w, xy, ra_k, dec_k, (ny, nx), match_radius, rms, sfit, max_rounds=1)
    fitted = 3600.0 * float(np.sqrt(abs(np.linalg.det(w.cd))))
    rows_h = rows.cpu().numpy()
    out.update(wcs=w, rms=rms, n_matched=len(pairs), scale=fitted,
               pairs=np.stack([pairs[:, 0], rows_h[pairs[:, 1]]], axis=1) if len(pairs) else out['pairs'])
    if len(pairs) >= min_matched and scale / (1.02 * ratio) <= fitted <= scale * 1.02 * ratio and len(pairs) >= best['n_seed']:
        out['status'] = SOLVE_NOMINAL
    return out


# ------------------------------------------------------------------------------------------------------------------
# F22: ApEmpiricalPsf - the effective PSF of the stars, PSF-fitting photometry, star removal (csrc/epsf.hip, DESIGN 4.3n;
# photutils absent, parity unpinned; the definition is restated in tests/epsf_model.py)
EPSF_SMOOTHING = {'quartic': 4, 'quadratic': 2, 'none': None}
EPSF_REC_COLUMNS = ('flux_fit', 'x_fit', 'y_fit', 'sky_fit', 'chi2', 'npix', 'niter', 'fit_ok')


def epsf_grid_size(o, R):
    """G = 2 o R + 1 for oversampling o in 1 .. 4 and stamp radius R in 2 .. 32 pixels (ValueError otherwise)."""
    if isinstance(o, bool) or isinstance(R, bool) or int(o) != o or int(R) != R:
        raise ValueError('oversampling and radius must be integers, got %r and %r' % (o, R))
    o, R = int(o), int(R)
    if not 1 <= o <= _lib.EPSF_MAX_OVERSAMPLING:
        raise ValueError('oversampling = %d is outside 1 .. %d' % (o, _lib.EPSF_MAX_OVERSAMPLING))
    if not 2 <= R <= _lib.EPSF_MAX_RADIUS:
        raise ValueError('radius = %d is outside 2 .. %d' % (R, _lib.EPSF_MAX_RADIUS))
    return 2 * o * R + 1


def _epsf_grid(E, o):
    """(E, o, R) of a grid argument: a square float32 device tensor [G, G] with G = 2 o R + 1."""
    if not torch.is_tensor(E) or E.dtype != torch.float32 or E.dim() != 2 or E.shape[0] != E.shape[1]:
        raise ValueError('the ePSF grid must be a square float32 tensor, got %s' % (
            '%s %s' % (E.dtype, tuple(E.shape)) if torch.is_tensor(E) else type(E).__name__))
    _need_cuda(E)
    if isinstance(o, bool) or int(o) != o or int(o) < 1:
        raise ValueError('oversampling = %r is not a positive integer' % (o,))
    G, o = int(E.shape[0]), int(o)
    if (G - 1) % (2 * o):
        raise ValueError('a grid of %d nodes per axis is not 2 o R + 1 for oversampling %d' % (G, o))
    R = (G - 1) // (2 * o)
    epsf_grid_size(o, R)
    return E.contiguous(), o, R


def _epsf_rows(a, cols, name, device):
    """A star table argument: [n, cols] float64 on the device (a NumPy array, a sequence or a tensor)."""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, cols)))
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError('%s must have the shape [n, %d], got %s' % (name, cols, tuple(t.shape)))
    if t.shape[0] >= 2 ** 31:
        raise ValueError('%s has too many rows' % name)
    return t.to(device=device, dtype=torch.float64).contiguous()


def epsf_smoothing_taps(kind='quartic'):
    """The 5 x 5 smoothing taps (float64 [5, 5], row-major) of the update: the weights with which the least-squares fit of the
    full bivariate polynomial of degree 4 ('quartic') or 2 ('quadratic') to a 5 x 5 neighbourhood gives its value at the centre
    - the centre row of the fit's pseudo-inverse, computed here with numpy.linalg.  'none': the identity."""
    if kind not in EPSF_SMOOTHING:
        raise ValueError('smoothing = %r; allowed: %s' % (kind, list(EPSF_SMOOTHING)))
    deg = EPSF_SMOOTHING[kind]
    taps = np.zeros((5, 5))
    if deg is None:
        taps[2, 2] = 1.0
        return taps
    yy, xx = np.mgrid[-2:3, -2:3].astype(np.float64)
    terms = [(a, b) for a in range(deg + 1) for b in range(deg + 1 - a)]                 # x^a y^b, a + b <= deg; (0, 0) first
    A = np.stack([xx.ravel() ** a * yy.ravel() ** b for a, b in terms], axis=1)           # [25, terms]
    return np.linalg.pinv(A)[0].reshape(5, 5)                                            # the constant term = the value at (0, 0)


def epsf_accumulate(image, stars, E, o, sigma=2.5, maxiters=5):
    """The sigma-clipped mean residual of the stars' pixels about the ePSF E at every node (apgpu_epsf_accumulate_f32).  stars:
    [n, 4] = flux, x, y, sky.  Returns (mean float64 [G, G], count int32 [G, G]) on the device."""
    image = _image_f32(image, 'image')
    E, o, R = _epsf_grid(E, o)
    stars = _epsf_rows(stars, 4, 'stars', image.device)
    if not float(sigma) > 0 or int(maxiters) < 0:
        raise ValueError('sigma (%r) must be > 0 and maxiters (%r) >= 0' % (sigma, maxiters))
    G = int(E.shape[0])
    mean = torch.empty((G, G), dtype=torch.float64, device=image.device)
    count = torch.empty((G, G), dtype=torch.int32, device=image.device)
    check(_lib.load().apgpu_epsf_accumulate_f32(_ptr(image), int(image.shape[0]), int(image.shape[1]), _ptr(stars), int(stars.shape[0]),
                                                _ptr(E), o, R, float(sigma), int(maxiters), _ptr(mean), _ptr(count), _stream()))
    return mean, count


def epsf_shift(E, o, dx, dy, scale=1.0):
    """The grid of E(u + (dx, dy)) scale at its own nodes u (apgpu_epsf_shift_f32): a new float32 device tensor."""
    E, o, R = _epsf_grid(E, o)
    if not all(math.isfinite(float(v)) for v in (dx, dy, scale)):
        raise ValueError('the offset (%r, %r) and the scale %r must be finite' % (dx, dy, scale))
    out = torch.empty(tuple(E.shape), dtype=torch.float32, device=E.device)
    check(_lib.load().apgpu_epsf_shift_f32(_ptr(E), o, R, float(dx), float(dy), float(scale), _ptr(out), _stream()))
    return out


def epsf_centroid(E, o, r_fit=None):
    """(dx, dy) pixels: the centre of mass of max(E, 0) over the nodes within r_fit of the centre (None: all), in float64 on the
    host from a NumPy copy of the grid.  (0, 0) for a grid without positive weight."""
    E = np.asarray(E, np.float64)
    G = E.shape[0]
    half = (G - 1) // 2
    off = (np.arange(G) - half) / float(o)
    w = np.maximum(E, 0.0)
    if r_fit is not None:
        w = np.where(off[:, None] ** 2 + off[None, :] ** 2 <= float(r_fit) ** 2, w, 0.0)
    tot = w.sum()
    if not (tot > 0 and np.isfinite(tot)):
        return 0.0, 0.0
    return float((w.sum(axis=0) * off).sum() / tot), float((w.sum(axis=1) * off).sum() / tot)


def epsf_update(E, mean, count, o, taps='quartic', min_count=1, r_fit=None, recentre=True, normalise=True):
    """One update of the ePSF: E + mean where count >= min_count, the 5 x 5 smoothing with `taps` (a name of
    epsf_smoothing_taps or 25 numbers) - one kernel (apgpu_epsf_update_f32) -, then the recentring by the centre of mass
    (epsf_centroid; a shift of at least 1e-6 px goes through epsf_shift) and the normalisation sum(E) / o^2 = 1.
    Returns (the new grid, (dx, dy) of the recentring)."""
    E, o, R = _epsf_grid(E, o)
    G = int(E.shape[0])
    _need_cuda(mean, count)
    if mean.dtype != torch.float64 or count.dtype != torch.int32 or tuple(mean.shape) != (G, G) or tuple(count.shape) != (G, G):
        raise ValueError('mean (float64) and count (int32) must have the grid\'s shape %s' % ((G, G),))
    taps = np.ascontiguousarray(epsf_smoothing_taps(taps) if isinstance(taps, str) else np.asarray(taps, np.float64))
    if taps.size != 25 or not np.all(np.isfinite(taps)):
        raise ValueError('taps must be 25 finite numbers')
    out = torch.empty((G, G), dtype=torch.float32, device=E.device)
    check(_lib.load().apgpu_epsf_update_f32(_ptr(E), _ptr(mean.contiguous()), _ptr(count.contiguous()), o, R, int(min_count),
                                            taps.ctypes.data_as(C.POINTER(C.c_double)), _ptr(out), _stream()))
    delta = (0.0, 0.0)
    if recentre:
        delta = epsf_centroid(out.cpu().numpy(), o, r_fit)
        if math.hypot(*delta) >= 1e-6:
            out = epsf_shift(out, o, delta[0], delta[1])
    if normalise:
        tot = float(out.cpu().numpy().astype(np.float64).sum()) / (o * o)
        if tot > 0 and math.isfinite(tot):
            out = epsf_shift(out, o, 0.0, 0.0, 1.0 / tot)
    return out, delta


def epsf_fit(image, init, E, o, r_fit, fit_sky=False, gain=0.0, readnoise=0.0, max_iter=50, prev=None):
    """PSF-fitting photometry (apgpu_epsf_fit_f32): flux and centre, and the sky with fit_sky, of every star of init ([n, 4] =
    flux, x, y, sky) from the pixels within r_fit of its rounded centre.  gain > 0: weights 1 / (readnoise^2 + max(model, 0) /
    gain), else uniform.  prev ([n, 3] = f0, x0, y0): `image` is a residual image and each star's own previous model is added back.
    Returns the records, float64 [n, 8] on the device: EPSF_REC_COLUMNS."""
    image = _image_f32(image, 'image')
    E, o, R = _epsf_grid(E, o)
    init = _epsf_rows(init, 4, 'init', image.device)
    n = int(init.shape[0])
    if prev is not None:
        prev = _epsf_rows(prev, 3, 'prev', image.device)
        if int(prev.shape[0]) != n:
            raise ValueError('prev has %d rows for %d stars' % (prev.shape[0], n))
    if not 1.0 <= float(r_fit) <= _lib.EPSF_MAX_RADIUS:
        raise ValueError('r_fit = %r is outside 1 .. %d' % (r_fit, _lib.EPSF_MAX_RADIUS))
    if not float(gain) >= 0 or not float(readnoise) >= 0 or int(max_iter) < 1:
        raise ValueError('gain (%r) and readnoise (%r) must be >= 0 and max_iter (%r) >= 1' % (gain, readnoise, max_iter))
    rec = torch.empty((n, _lib.EPSF_REC), dtype=torch.float64, device=image.device)
    check(_lib.load().apgpu_epsf_fit_f32(_ptr(image), int(image.shape[0]), int(image.shape[1]), _ptr(init), _ptr(prev), n, _ptr(E), o, R,
                                         float(r_fit), int(bool(fit_sky)), float(gain), float(readnoise), int(max_iter), _ptr(rec),
                                         _stream()))
    return rec


def epsf_tile_lists(x, y, R, shape, device='cuda'):
    """The stars of every 32 x 32-pixel tile of an image of `shape` in CSR form: (offsets int32 [tiles + 1], stars int32 [entries]),
    tiles row-major, ascending star index within a tile.  A star is listed in the tiles its stamp's bounding box
    [x - R, x + R] x [y - R, y + R] touches; one with a non-finite centre in none.  Built on the host."""
    H, W = _image_shape(shape)
    T = _lib.EPSF_TILE
    ty, tx = -(-H // T), -(-W // T)
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    if x.shape != y.shape:
        raise ValueError('x and y must have one length, got %d and %d' % (x.size, y.size))
    R = float(R)
    tiles, stars = [], []
    ok = np.isfinite(x) & np.isfinite(y) & (x + R >= 0) & (x - R <= W - 1) & (y + R >= 0) & (y - R <= H - 1)
    for s in np.flatnonzero(ok):
        x0, x1 = max(int(math.ceil(x[s] - R)), 0) // T, min(int(math.floor(x[s] + R)), W - 1) // T
        y0, y1 = max(int(math.ceil(y[s] - R)), 0) // T, min(int(math.floor(y[s] + R)), H - 1) // T
        for b in range(y0, y1 + 1):
            for a in range(x0, x1 + 1):
                tiles.append(b * tx + a)
                stars.append(s)
    tiles, stars = np.asarray(tiles, np.int64), np.asarray(stars, np.int64)
    if tiles.size >= 2 ** 31:
        raise ValueError('too many tile entries')
    order = np.argsort(tiles, kind='stable')
    offsets = np.zeros(ty * tx + 1, np.int64)
    np.cumsum(np.bincount(tiles, minlength=ty * tx), out=offsets[1:])
    return (torch.from_numpy(offsets.astype(np.int32)).to(device), torch.from_numpy(stars[order].astype(np.int32)).to(device))


def epsf_render(image, stars, E, o, lists=None, shape=None, model=True, residual=True):
    """The image of the stars ([n, 3] = flux, x, y) under the ePSF and / or image minus it (apgpu_epsf_render_f32): (model, residual)
    float32 device planes, None for the one not asked for.  image may be None with shape = (H, W) when only the model is
    wanted.  lists: epsf_tile_lists of these stars (built here when None).  NaN pixels stay NaN in the residual."""
    E, o, R = _epsf_grid(E, o)
    if image is None:
        if residual or shape is None:
            raise ValueError('without an image only the model can be rendered, and shape is needed')
        H, W = _image_shape(shape)
    else:
        image = _image_f32(image, 'image')
        H, W = int(image.shape[0]), int(image.shape[1])
    if not (model or residual):
        raise ValueError('neither the model nor the residual is asked for')
    stars = _epsf_rows(stars, 3, 'stars', E.device)
    n = int(stars.shape[0])
    if lists is None:
        sh = stars.cpu().numpy()
        lists = epsf_tile_lists(sh[:, 1], sh[:, 2], R, (H, W), E.device)
    offsets, idx = lists
    _need_cuda(offsets, idx)
    n_tiles = -(-H // _lib.EPSF_TILE) * -(-W // _lib.EPSF_TILE)
    if offsets.dtype != torch.int32 or idx.dtype != torch.int32 or offsets.numel() != n_tiles + 1 or offsets.dim() != 1 or idx.dim() != 1:
        raise ValueError('lists must be (offsets int32 [%d], stars int32 [entries]) of epsf_tile_lists for this shape' % (n_tiles + 1))
    offsets, idx = offsets.contiguous(), idx.contiguous()
    m = torch.empty((H, W), dtype=torch.float32, device=E.device) if model else None
    r = torch.empty((H, W), dtype=torch.float32, device=E.device) if residual else None
    check(_lib.load().apgpu_epsf_render_f32(_ptr(image), H, W, _ptr(stars) if n else None, n, _ptr(offsets), _ptr(idx) if idx.numel() else None,
                                            int(idx.numel()), _ptr(E), o, R, _ptr(m), _ptr(r), _stream()))
    return m, r


def epsf_select_stars(x, y, flux, shape, R, r_fit, psbl_sat=None, max_stars=500):
    """The indices of the stars an ePSF is built from, brightest first: not flagged in psbl_sat, finite x, y and flux > 0, at least
    R + 2 pixels from every edge, no other star of the whole list (flagged ones too) within R + r_fit, the max_stars brightest."""
    H, W = _image_shape(shape)
    x, y, flux = (np.asarray(v, np.float64).reshape(-1) for v in (x, y, flux))
    n = x.size
    sat = np.zeros(n, bool) if psbl_sat is None else np.asarray(psbl_sat).astype(bool).reshape(-1)
    pos = np.isfinite(x) & np.isfinite(y)
    with np.errstate(invalid='ignore'):
        ok = pos & ~sat & np.isfinite(flux) & (flux > 0) & (x >= R + 2) & (x <= W - 1 - (R + 2)) & (y >= R + 2) & (y <= H - 1 - (R + 2))
    cand, others = np.flatnonzero(ok), np.flatnonzero(pos)
    lim2 = float(R + r_fit) ** 2
    keep = []
    for s in cand:
        d2 = (x[others] - x[s]) ** 2 + (y[others] - y[s]) ** 2
        if np.count_nonzero(d2 < lim2) <= 1:                                     # itself
            keep.append(s)
    keep = np.asarray(keep, np.int64)
    order = np.argsort(-flux[keep], kind='stable')
    return keep[order][:int(max_stars)]


def epsf_build(image, x, y, flux, sky, o=4, R=12, r_fit=None, psbl_sat=None, max_stars=500, n_iter=8, tol=1e-4, sigma=2.5, maxiters=5,
               smoothing='quartic', min_count=1, fit_sky=False, gain=0.0, readnoise=0.0, max_iter=50, min_stars=1):
    """The empirical PSF of an image from a star list (x, y: centres, x = column; flux: the aperture sums; sky: per pixel): from
    E = 0, rounds of epsf_accumulate -> epsf_update -> epsf_fit over the stars of epsf_select_stars, until the grid changes by at
    most tol max(E) or n_iter rounds are done (none with fewer than min_stars stars).  r_fit: None = 2.  Returns dict(epsf: float32 device grid [G, G]; o, R, r_fit;
    index: the chosen stars' rows in the list; stars: their fitted records, float64 NumPy [n, 8] (EPSF_REC_COLUMNS); change: the
    relative change of every round; count: the last round's int32 NumPy counts [G, G]; niter)."""
    image = _image_f32(image, 'image')
    G = epsf_grid_size(o, R)
    o, R = int(o), int(R)
    r_fit = 2.0 if r_fit is None else float(r_fit)
    x, y, flux = (np.asarray(v, np.float64).reshape(-1) for v in (x, y, flux))
    sky = np.broadcast_to(np.asarray(sky, np.float64).reshape(-1), x.shape) if x.size else np.zeros(0)
    if not (x.shape == y.shape == flux.shape):
        raise ValueError('x, y and flux must have one length')
    index = epsf_select_stars(x, y, flux, image.shape, R, r_fit, psbl_sat, max_stars)
    cur = np.stack([flux[index], x[index], y[index], sky[index]], axis=1) if index.size else np.zeros((0, 4))
    taps = epsf_smoothing_taps(smoothing)
    E = torch.zeros((G, G), dtype=torch.float32, device=image.device)
    rec = np.zeros((0, _lib.EPSF_REC))
    change, count, done = [], np.zeros((G, G), np.int32), 0
    for _ in range(int(n_iter) if index.size >= max(int(min_stars), 1) else 0):
        mean, cnt = epsf_accumulate(image, cur, E, o, sigma, maxiters)
        E_new, _delta = epsf_update(E, mean, cnt, o, taps, min_count, r_fit)
        new_h, old_h = E_new.cpu().numpy().astype(np.float64), E.cpu().numpy().astype(np.float64)
        peak = float(new_h.max())
        change.append(float(np.abs(new_h - old_h).max()) / peak if peak > 0 else float('inf'))
        E, count, done = E_new, cnt.cpu().numpy(), done + 1
        rec = epsf_fit(image, cur, E, o, r_fit, fit_sky, gain, readnoise, max_iter).cpu().numpy()
        cur = rec[:, :4].copy()                                                     # (a star whose fit failed kept its values)
        if change[-1] <= tol:
            break
    return dict(epsf=E, o=o, R=R, r_fit=r_fit, index=index, stars=rec, change=change, count=count, niter=done)


def epsf_stamp(E, o):
    """The ePSF at integer pixel offsets: every o-th node of the grid, [2R + 1, 2R + 1], negative values set to 0, normalised to
    sum 1 in float64, as float32 NumPy - what ApDeconvolve.normalise_stamp accepts."""
    E = np.asarray(E.cpu() if torch.is_tensor(E) else E, np.float64)
    if E.ndim != 2 or E.shape[0] != E.shape[1] or isinstance(o, bool) or int(o) != o or int(o) < 1 or (E.shape[0] - 1) % (2 * int(o)):
        raise ValueError('a grid of shape %s is not [2 o R + 1] squared for oversampling %r' % (E.shape, o))
    epsf_grid_size(int(o), (E.shape[0] - 1) // (2 * int(o)))
    p = np.maximum(E[::int(o), ::int(o)], 0.0)
    tot = p.sum()
    if not (np.all(np.isfinite(p)) and tot > 0):
        raise ValueError('the ePSF has no positive finite weight at the pixel offsets')
    return (p / tot).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# F23: ApSubtract - optimal image subtraction with a spatially varying kernel (csrc/subtract.hip; Alard & Lupton
# 1998, Alard 2000; the reference has no such stage, parity unpinned; the definition is restated in tests/subtract_model.py)
SUBTRACT_SIGMAS, SUBTRACT_DEGREES, SUBTRACT_RADIUS = (0.7, 1.5, 3.0), (6, 4, 2), 10
SUBTRACT_STATUS = {1: 'the footprint leaves the image', 2: 'non-finite template pixel', 4: 'non-finite image pixel', 8: 'masked pixel'}


class SubtractNoFit(ArithmeticError):
    """Fewer usable stamps than the spatial terms need, or normal equations that cannot be solved."""


def _poly_count(d):
    return (d + 1) * (d + 2) // 2


def _sub_degree(d, name):
    if isinstance(d, bool) or int(d) != d or not 0 <= int(d) <= _lib.SUBTRACT_MAX_DEGREE:
        raise ValueError('%s = %r is outside 0 .. %d' % (name, d, _lib.SUBTRACT_MAX_DEGREE))
    return int(d)


def _sub_ipow(x, k):
    p = np.ones_like(np.asarray(x, np.float64))
    for _ in range(k):
        p = p * x
    return p


def subtract_poly_terms(degree, X, Y):
    """[terms, ...] float64: X^i Y^j for i + j <= degree, i then j ascending, the powers by repeated multiplication."""
    return np.stack([_sub_ipow(X, i) * _sub_ipow(Y, j) for i in range(degree + 1) for j in range(degree + 1 - i)])


def subtract_norm_coord(p, n):
    """(2 p - (n - 1)) / max(n - 1, 1): -1 .. 1 over an axis of n pixels."""
    return (2 * np.asarray(p, np.int64) - (n - 1)) / float(max(n - 1, 1))


def kernel_basis(sigmas=SUBTRACT_SIGMAS, degrees=SUBTRACT_DEGREES, radius=SUBTRACT_RADIUS):
    """The kernel basis of Gaussians times polynomials (apgpu_subtract_basis_f64; host only): a dict of the separable form - filters
    float64 [NF, 2 r + 1], row, col, even int32 [Nb], scale float64 [Nb] - the dense functions B float64 [Nb, 2 r + 1, 2 r + 1] (B_n(u, v)
    at [n, v + r, u + r]; every function but the first sums to 0, the first to 1), radius, nb, sigmas and degrees."""
    sig = np.ascontiguousarray(np.asarray(sigmas, np.float64).ravel())
    deg = np.asarray(degrees).ravel()
    if sig.size == 0 or sig.size != deg.size or np.any(deg != deg.astype(np.int64)):
        raise ValueError('sigmas %r and degrees %r must be as many numbers, the degrees integers' % (sigmas, degrees))
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= _lib.SUBTRACT_MAX_RADIUS:
        raise ValueError('radius = %r is outside 1 .. %d' % (radius, _lib.SUBTRACT_MAX_RADIUS))
    if not np.all(np.isfinite(sig) & (sig > 0)) or np.any(deg < 0):
        raise ValueError('sigmas must be > 0 and degrees >= 0, got %r and %r' % (sigmas, degrees))
    if sum(_poly_count(int(d)) for d in deg) > _lib.SUBTRACT_MAX_BASIS:
        raise ValueError('the degrees %r make more than %d basis functions' % (list(deg), _lib.SUBTRACT_MAX_BASIS))
    deg = np.ascontiguousarray(deg.astype(np.int32))
    r, M = int(radius), _lib.SUBTRACT_MAX_BASIS
    kw = 2 * r + 1
    filters = np.zeros((M, kw), np.float64)
    row, col, even = (np.zeros(M, np.int32) for _ in range(3))
    scale = np.zeros(M, np.float64)
    nf, nb = C.c_int32(0), C.c_int32(0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    check(_lib.load().apgpu_subtract_basis_f64(sig.ctypes.data_as(dp), deg.ctypes.data_as(ip), int(sig.size), r, filters.ctypes.data_as(dp),
                                               row.ctypes.data_as(ip), col.ctypes.data_as(ip), scale.ctypes.data_as(dp),
                                               even.ctypes.data_as(ip), C.byref(nf), C.byref(nb)))
    nf, nb = nf.value, nb.value
    filters, row, col, even, scale = filters[:nf].copy(), row[:nb].copy(), col[:nb].copy(), even[:nb].copy(), scale[:nb].copy()
    B = np.empty((nb, kw, kw))
    for n in range(nb):
        B[n] = scale[n] * (filters[col[n]][:, None] * filters[row[n]][None, :])
        if n > 0 and even[n]:
            B[n] = B[n] - B[0]
    return dict(filters=filters, row=row, col=col, even=even, scale=scale, B=B, radius=r, nb=nb, sigmas=[float(s) for s in sig],
                degrees=[int(d) for d in deg])


def _sub_centers(centers, device):
    c = centers.cpu().numpy() if torch.is_tensor(centers) else np.asarray(centers)
    c = c.reshape(-1, 2)
    if c.size and (np.any(c != np.rint(c)) or np.abs(c).max() >= 2 ** 31):
        raise ValueError('stamp centres must be integer pixels (x, y)')
    return torch.from_numpy(np.ascontiguousarray(c.astype(np.int32))).to(device)


def subtract_stamps(template, image, centers, half, basis, mask=None, gain=0.0, readnoise=0.0):
    """The normal equations of every stamp (apgpu_subtract_stamps_f32): `template` is the image that the kernel convolves, `image` the one
    it is matched to; centers [S, 2] integer (x, y); half the stamp's half-size (1 .. 15); basis a dict of kernel_basis.  mask: non-zero
    pixels refuse the stamps they fall in.  gain > 0 (then readnoise > 0): weights 1 / (readnoise^2 / gain^2 + max(image, 0) / gain).
    Returns device tensors (gram float64 [S, Nb + 2, Nb + 2], status int32 [S], count int32 [S]): gram[s, :Nb + 1, :Nb + 1] is the Gram
    matrix of the stamp's fit vectors T (x) B_0 .., 1, gram[s, :Nb + 1, Nb + 1] their products with the image, gram[s, Nb + 1, Nb + 1]
    sum w I^2; status is 0 or a sum of SUBTRACT_STATUS' bits (the stamp then has zeros and count 0)."""
    template = _image_f32(template, 'template')
    image = _plane_like(image, 'image', template)
    mask = _mask_u8(mask, template.shape, 'mask must have the image shape %s' % (tuple(template.shape),))
    if isinstance(half, bool) or int(half) != half or not 1 <= int(half) <= _lib.SUBTRACT_MAX_HALF:
        raise ValueError('half = %r is outside 1 .. %d' % (half, _lib.SUBTRACT_MAX_HALF))
    if not float(gain) >= 0 or not float(readnoise) >= 0 or not math.isfinite(float(gain)) or not math.isfinite(float(readnoise)) or \
            (float(gain) > 0 and not float(readnoise) > 0):
        raise ValueError('gain (%r) and readnoise (%r) must be finite and >= 0, and a gain needs a read noise above 0' % (gain, readnoise))
    dev = template.device
    cen = _sub_centers(centers, dev)
    S, nb = int(cen.shape[0]), int(basis['nb'])
    filters = torch.from_numpy(np.ascontiguousarray(basis['filters'], np.float64)).to(dev)
    row, col, even = (np.ascontiguousarray(basis[k], np.int32) for k in ('row', 'col', 'even'))
    scale = np.ascontiguousarray(basis['scale'], np.float64)
    gram = torch.empty((S, nb + 2, nb + 2), dtype=torch.float64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    count = torch.empty(S, dtype=torch.int32, device=dev)
    ip = C.POINTER(C.c_int32)
    check(_lib.load().apgpu_subtract_stamps_f32(_ptr(template), _ptr(image), _ptr(mask), int(template.shape[0]), int(template.shape[1]),
                                                _ptr(cen), S, int(half), int(basis['radius']), _ptr(filters), int(filters.shape[0]),
                                                row.ctypes.data_as(ip), col.ctypes.data_as(ip), scale.ctypes.data_as(C.POINTER(C.c_double)),
                                                even.ctypes.data_as(ip), nb, float(gain), float(readnoise), _ptr(gram), _ptr(status),
                                                _ptr(count), _stream()))
    return gram, status, count


def _sub_design(nb, kdeg, bdeg, X, Y):
    """P [unknowns, Nb + 1] of a stamp at the normalised centre (X, Y): the unknowns are a_0, then a_{n,t} (n = 1 .. Nb - 1 outside, t
    inside), then c_t; column m belongs to the fit vector V_m (V_Nb = 1)."""
    pk, pb = subtract_poly_terms(kdeg, X, Y), subtract_poly_terms(bdeg, X, Y)
    ntk = len(pk)
    P = np.zeros((1 + (nb - 1) * ntk + len(pb), nb + 1))
    P[0, 0] = 1.0
    for n in range(1, nb):
        P[1 + (n - 1) * ntk:1 + n * ntk, n] = pk
    P[1 + (nb - 1) * ntk:, nb] = pb
    return P


def subtract_fit(gram, status, count, centers, shape, basis, kernel_degree=2, bg_degree=1, k=3.0, rounds=3):
    """The host side of the fit, float64: the normal equations M = sum_s P_s G_s P_s^T of the kept stamps (the spatial terms taken at the
    stamps' centres), scaled by their diagonal and solved; every stamp's chi^2 per pixel from its own G_s, g_s and sum w I^2; stamps
    above median + k 1.4826 MAD dropped and the fit made again, at most `rounds` times.  gram, status, count: what subtract_stamps
    returned (tensors or arrays).  Returns a dict: a0 (the photometric scale), akt [Nb, ntk] (a_{n,t}; row 0 holds a_0 in column 0), bg
    [ntb], kernels (the composite kernels A_t, float32 [ntk, 2 r + 1, 2 r + 1]), kept (bool [S]), chi2 [S] (NaN for a refused stamp),
    cond (of the scaled normal matrix), rounds (fits made), margin (the smallest relative distance of a chi^2 to the last cut).
    Raises SubtractNoFit when fewer stamps are usable than the spatial terms need."""
    kdeg, bdeg = _sub_degree(kernel_degree, 'kernel_degree'), _sub_degree(bg_degree, 'bg_degree')
    gram, status, count = (np.asarray(a.cpu().numpy() if torch.is_tensor(a) else a) for a in (gram, status, count))
    centers = (centers.cpu().numpy() if torch.is_tensor(centers) else np.asarray(centers)).reshape(-1, 2).astype(np.int64)
    H, W = int(shape[0]), int(shape[1])
    nb, S = int(basis['nb']), gram.shape[0]
    if gram.shape[1:] != (nb + 2, nb + 2) or len(centers) != S or len(status) != S or len(count) != S:
        raise ValueError('gram %s, status, count and centers do not belong to %d stamps of %d basis functions' % (gram.shape, S, nb))
    if not float(k) > 0 or int(rounds) < 0:
        raise ValueError('k (%r) must be > 0 and rounds (%r) >= 0' % (k, rounds))
    ntk, ntb = _poly_count(kdeg), _poly_count(bdeg)
    Ps = [_sub_design(nb, kdeg, bdeg, float(subtract_norm_coord(cx, W)), float(subtract_norm_coord(cy, H))) for cx, cy in centers]
    usable = status == 0
    kept = usable.copy()
    chi2 = np.full(S, np.nan)
    margin, made = float('inf'), 0
    nun = 1 + (nb - 1) * ntk + ntb
    while True:
        if kept.sum() < max(ntk, ntb):
            raise SubtractNoFit('%d usable stamps for %d spatial terms' % (kept.sum(), max(ntk, ntb)))
        M, rhs = np.zeros((nun, nun)), np.zeros(nun)
        for s in np.flatnonzero(kept):
            M = M + Ps[s] @ gram[s, :nb + 1, :nb + 1] @ Ps[s].T
            rhs = rhs + Ps[s] @ gram[s, :nb + 1, nb + 1]
        d = np.sqrt(np.diag(M))
        if not np.all(d > 0) or not np.all(np.isfinite(M)):
            raise SubtractNoFit('the normal matrix has an empty or non-finite row')
        Ms = M / d[:, None] / d[None, :]
        try:
            theta = np.linalg.solve(Ms, rhs / d) / d
        except np.linalg.LinAlgError as exc:
            raise SubtractNoFit('the normal equations are singular') from exc
        made += 1
        for s in np.flatnonzero(usable):
            q = Ps[s].T @ theta
            chi2[s] = (gram[s, nb + 1, nb + 1] - 2.0 * (q @ gram[s, :nb + 1, nb + 1]) + q @ gram[s, :nb + 1, :nb + 1] @ q) / count[s]
        if made > int(rounds):
            break
        c = chi2[kept]
        med = np.median(c)
        cut = med + float(k) * 1.4826 * np.median(np.abs(c - med))
        drop = kept & (chi2 > cut)
        margin = float(np.min(np.abs(c - cut)) / cut)
        if not drop.any():
            break
        kept = kept & ~drop
    akt = np.zeros((nb, ntk))
    akt[0, 0] = theta[0]
    akt[1:] = theta[1:1 + (nb - 1) * ntk].reshape(nb - 1, ntk)
    kernels = np.zeros((ntk,) + basis['B'].shape[1:])
    for t in range(ntk):
        for n in range(nb):
            kernels[t] = kernels[t] + akt[n, t] * basis['B'][n]
    return dict(a0=float(theta[0]), akt=akt, bg=theta[1 + (nb - 1) * ntk:].copy(), kernels=kernels.astype(np.float32), kept=kept, chi2=chi2,
                cond=float(np.linalg.cond(Ms)), rounds=made, margin=margin, kernel_degree=kdeg, bg_degree=bdeg)


def subtract_kernel_at(fit, x, y, shape):
    """The fitted kernel at pixel (x, y) of an image of `shape`: float64 [2 r + 1, 2 r + 1], K(u, v) at [v + r, u + r]."""
    phi = subtract_poly_terms(fit['kernel_degree'], float(subtract_norm_coord(int(x), int(shape[1]))), float(subtract_norm_coord(int(y), int(shape[0]))))
    return np.tensordot(phi, fit['kernels'].astype(np.float64), 1)


def subtract_apply(convolved, other, kernels, kernel_degree, bg, bg_degree, convolved_image=False, a0=1.0, matched=False):
    """Applies a fitted kernel (apgpu_subtract_apply_f32).  `convolved` is the image the kernel convolves (the template, or with
    convolved_image=True the image), `other` the one it is compared with; kernels float32 [ntk, 2 r + 1, 2 r + 1] (subtract_fit's
    'kernels'), bg the background coefficients.  Returns the difference other - (convolved (x) K + B), or with convolved_image
    ((convolved (x) K + B) - other) / a0; with matched=True (diff, convolved (x) K + B).  NaN where `other` is not finite or the
    kernel's footprint meets a non-finite pixel of `convolved` or the image's edge."""
    convolved = _image_f32(convolved, 'convolved')
    other = _plane_like(other, 'other', convolved)
    kdeg, bdeg = _sub_degree(kernel_degree, 'kernel_degree'), _sub_degree(bg_degree, 'bg_degree')
    kn = np.ascontiguousarray(kernels.cpu().numpy() if torch.is_tensor(kernels) else kernels, np.float32)
    if kn.ndim != 3 or kn.shape[0] != _poly_count(kdeg) or kn.shape[1] != kn.shape[2] or kn.shape[1] % 2 == 0 or \
            not 1 <= (kn.shape[1] - 1) // 2 <= _lib.SUBTRACT_MAX_RADIUS:
        raise ValueError('kernels of shape %s are not [%d, 2 r + 1, 2 r + 1] with r in 1 .. %d' % (kn.shape, _poly_count(kdeg), _lib.SUBTRACT_MAX_RADIUS))
    bgc = np.ascontiguousarray(np.asarray(bg, np.float64).ravel())
    if bgc.size != _poly_count(bdeg) or not np.all(np.isfinite(bgc)):
        raise ValueError('bg must be %d finite coefficients' % _poly_count(bdeg))
    if convolved_image and (not math.isfinite(float(a0)) or float(np.float32(a0)) == 0.0):
        raise ValueError('a0 = %r must be finite and not 0' % (a0,))
    kd = torch.from_numpy(kn).to(convolved.device)
    diff = torch.empty_like(convolved)
    mt = torch.empty_like(convolved) if matched else None
    check(_lib.load().apgpu_subtract_apply_f32(_ptr(convolved), _ptr(other), int(convolved.shape[0]), int(convolved.shape[1]), _ptr(kd),
                                               (kn.shape[1] - 1) // 2, kdeg, bgc.ctypes.data_as(C.POINTER(C.c_double)), bdeg,
                                               _lib.SUBTRACT_CONVOLVED_IMAGE if convolved_image else 0, float(a0), _ptr(diff), _ptr(mt),
                                               _stream()))
    return (diff, mt) if matched else diff


def subtract_select_stamps(x, y, flux, shape, half, radius, peak=None, satlevel=None, nx=4, ny=4, per_region=5):
    """The stamp centres [S, 2] int64 (x, y) from a star list, on the host: stars with a peak at satlevel are dropped; of two stars
    closer than 2 half the fainter is dropped; stamps whose footprint half + radius leaves the image are dropped; the brightest
    per_region of every cell of an nx x ny grid are kept.  In the order of falling flux."""
    H, W = int(shape[0]), int(shape[1])
    x, y, flux = (np.asarray(a, np.float64).ravel() for a in (x, y, flux))
    if not (x.size == y.size == flux.size) or int(nx) < 1 or int(ny) < 1 or int(per_region) < 1:
        raise ValueError('x, y and flux must be as many numbers; nx, ny and per_region at least 1')
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(flux)
    if peak is not None and satlevel is not None:
        ok &= ~(np.asarray(peak, np.float64).ravel() >= float(satlevel))
    order = [i for i in np.argsort(-np.where(ok, flux, -np.inf), kind='stable') if ok[i]]
    taken, cells, out = [], {}, []
    F = int(half) + int(radius)
    for i in order:
        if any(math.hypot(x[i] - x[j], y[i] - y[j]) < 2 * half for j in taken):
            continue
        taken.append(i)
        cx, cy = int(np.rint(x[i])), int(np.rint(y[i]))
        if cx - F < 0 or cx + F >= W or cy - F < 0 or cy + F >= H:
            continue
        cell = (min(cx * int(nx) // W, int(nx) - 1), min(cy * int(ny) // H, int(ny) - 1))
        if cells.get(cell, 0) >= int(per_region):
            continue
        cells[cell] = cells.get(cell, 0) + 1
        out.append((cx, cy))
    return np.array(out, np.int64).reshape(-1, 2)


def optimal_subtract(image, template, stars=None, centers=None, mask=None, sigmas=SUBTRACT_SIGMAS, degrees=SUBTRACT_DEGREES,
                     radius=SUBTRACT_RADIUS, kernel_degree=2, bg_degree=1, half=15, regions=(4, 4), per_region=5, satlevel=None, gain=0.0,
                     readnoise=0.0, k=3.0, rounds=3, convolve='template', fwhm=None, matched=False):
    """Optimal image subtraction end to end: D = image - (template (x) K + B) with the kernel K(u, v; x, y) and the background B(x, y)
    fitted on stamps around stars.  stars: [n, 3] or [n, 4] = x, y, flux[, peak] (an array or a tensor), from which
    subtract_select_stamps chooses; or centers [S, 2] as they are.  convolve: 'template', 'image' (D = (image (x) K + B - template) /
    a0, still on the image's flux scale) or 'auto' (the one with the smaller of fwhm = (image, template)).
    Returns a dict: diff, matched (with matched=True), centers, status, convolve and the entries of subtract_fit."""
    image = _image_f32(image, 'image')
    template = _plane_like(template, 'template', image)
    if convolve not in ('template', 'image', 'auto'):
        raise ValueError("convolve = %r; allowed: 'template', 'image', 'auto'" % (convolve,))
    if convolve == 'auto':
        if fwhm is None or not all(math.isfinite(float(f)) and float(f) > 0 for f in fwhm):
            raise ValueError("convolve='auto' needs fwhm = (image, template) in pixels")
        convolve = 'image' if float(fwhm[0]) < float(fwhm[1]) else 'template'
    basis = kernel_basis(sigmas, degrees, radius)
    if centers is None:
        if stars is None:
            raise ValueError('give stars (x, y, flux[, peak]) or stamp centers')
        st = np.asarray(stars.cpu().numpy() if torch.is_tensor(stars) else stars, np.float64)
        if st.ndim != 2 or st.shape[1] not in (3, 4):
            raise ValueError('stars must be [n, 3] (x, y, flux) or [n, 4] (x, y, flux, peak), got shape %s' % (st.shape,))
        centers = subtract_select_stamps(st[:, 0], st[:, 1], st[:, 2], image.shape, half, basis['radius'],
                                         st[:, 3] if st.shape[1] == 4 else None, satlevel, regions[0], regions[1], per_region)
    centers = (centers.cpu().numpy() if torch.is_tensor(centers) else np.asarray(centers)).reshape(-1, 2).astype(np.int64)
    src, oth = (template, image) if convolve == 'template' else (image, template)
    gram, status, count = subtract_stamps(src, oth, centers, half, basis, mask, gain, readnoise)
    status = status.cpu().numpy()
    fit = subtract_fit(gram, status, count, centers, image.shape, basis, kernel_degree, bg_degree, k, rounds)
    res = subtract_apply(src, oth, fit['kernels'], fit['kernel_degree'], fit['bg'], fit['bg_degree'], convolve == 'image', fit['a0'], matched)
    out = dict(fit, diff=res[0] if matched else res, centers=centers, status=status, convolve=convolve, basis=basis)
    if matched:
        out['matched'] = res[1]
    return out
