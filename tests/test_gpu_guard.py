"""Every kernel-launching entry point of libapgpu.so under the guard of tests/guard.py: stores outside an output or a workspace,
loads outside an input, stores into an input, and the stream that reaches the library.

One table of cases, one parametrised test.  A case places its inputs (and the outputs / workspaces a caller may own) inside
poisoned slabs, calls a few `ops` functions and hands every result to `io.out` together with the family's existing reference and
the bound the family's own GPU test uses.  The test runs a case three times inside `guarded(...)`:

  A  poison 0xFF (NaN as float32 / float64, 255 as a mask, 65535 as uint16), on the default stream;
  B  poison 0x00;
  C  poison 0xFF under torch.cuda.stream(s) of a side stream: inputs placed on s just before the call, no synchronisation in
     between, results fetched on s.

A equals the reference to the family's bound; B and C equal A bit for bit (a load outside an input that reaches a result makes A and B
differ; a call on another stream than the current one makes C differ when the race is lost); every stream argument recorded in C is
s and in A the default stream (this half is deterministic); every input is unchanged, every surround and every canary intact.

Results held to their family's bound instead of bit equality between the runs (ORDER_DEPENDENT below): those whose value depends on
the order in which atomic operations land.

What the catalogue found when it was written: ops.calibrate and ops.flat_normalize handed a plane one element past a 16-byte
boundary to kernels that take aligned planes, and the library refused it; the wrappers now copy such a plane once (`_aligned16`),
same bits.  Nothing else: no canary, input, surround, A / B / C or stream difference.  On one MI355X the module ran in 1.9 s next
to 100.0 s for the rest of `-m gpu` (1.9 %).

What the guard cannot reach:
  * scratch the library takes itself with hipMallocAsync (csrc/stack_chunks.hip, csrc/stack_kernels.h, csrc/resample.hip): the stack's
    per-call temporaries when no workspace is attached, the resample's tile lists;
  * the copies `.contiguous()` / `.clone()` / `.to()` make inside ops.py (an unaligned frame through `_aligned16`, masks of another
    dtype, per-frame scalars, the Lanczos table): they are torch's own allocations.  The kernel then reads the copy; the placed
    original is still checked for writes.
"""
import ctypes as C
import math
import time

import numpy as np
import pytest

from tests import composite_model as cpm
from tests import continuum_model as ctm
from tests import deconvolve_model as dcm
from tests import demosaic_model as dmm
from tests import drizzle_model as drm
from tests import findstars_model as fm
from tests import measurestars_model as msm
from tests import multiscale_model as mlm
from tests import register_model as rm
from astrophotography_amd._lib import TONE_TABLE_LEN
from tests.guard import guard_width, guarded, intact, place, unchanged
from tests.util import assert_biteq, assert_ulp, synth_cube, synth_masters

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
F = np.float32

# labels of the results that depend on the order of atomic operations, with the reason; they are compared with the reference to the
# family's own bound in every run instead of bit for bit with run A.  Exact labels: the test fails if one of them is never produced.
_SHORT_LIST = ('apgpu_local_peaks_f32 appends with an atomic counter: WHICH 64 of the 200 peaks a short list holds depends on scheduling '
               '(tests/test_gpu_findstars.py::test_capacity_is_respected_and_the_true_count_returned checks membership)')
_CHANNEL_SUMS = ('apgpu_bayer_channel_sums adds float64 partial sums with atomics: any order of n additions, bound n 2^-53 sum|v| '
                 '(tests/test_gpu_demosaic.py::test_channel_sums_f32_within_the_bound_of_any_order)')
ORDER_DEPENDENT = {'peaks_short_list': _SHORT_LIST, 'peaks_short_list_own': _SHORT_LIST,
                   'channel_sums_f32_6_float32': _CHANNEL_SUMS, 'channel_sums_f32_7_float32': _CHANNEL_SUMS}
ORDER_DEPENDENT_SEEN = set()

# entry points that launch nothing and take no device pointer (include/apgpu.h); everything else must have been called under the guard
EXCLUDED = {
    'apgpu_last_error': 'returns the thread-local message of the last failure: a host string',
    'apgpu_version': 'returns a constant',
    'apgpu_stack_kernel_name': 'names the kernel a stack call would dispatch: reads the argument struct on the host, never its pointers',
    'apgpu_flat_normalize_ws_bytes': 'size query: arithmetic on n',
    'apgpu_flat_normalize_f64_ws_bytes': 'size query: arithmetic on n',
    'apgpu_stack_ws_bytes': 'size query: arithmetic on n_pixels, writes one host size_t',
    'apgpu_resample_stack_ws_bytes': 'size query: arithmetic on the shapes',
    'apgpu_combine_ccdproc_f64_ws_bytes': 'size query: arithmetic on n_frames, n_pixels',
    'apgpu_sigclip_global_ws_bytes': 'size query: arithmetic on n',
    'apgpu_sigclip_global_f64_ws_bytes': 'size query: arithmetic on n',
    'apgpu_sliding_clipped_stats_ws_bytes': 'size query: arithmetic on the batch shape and the window',
    'apgpu_source_mask_ws_bytes': 'size query: arithmetic on H, W',
    'apgpu_lacosmic_ws_bytes': 'size query: arithmetic on H, W',
    'apgpu_quantile_levels_ws_bytes': 'size query: arithmetic on H, W',
    'apgpu_pair_moments_ws_bytes': 'size query: arithmetic on n',
    'apgpu_deconv_ws_bytes': 'size query: arithmetic on H, W',
    'apgpu_starlet_ws_bytes': 'size query: arithmetic on H, W',
}

CASES = []
SEEN = set()                        # names of the apgpu_* functions called under the guard, over all cases
RAN = set()
TIMES = {}


def case(name, row_bytes=0):
    def deco(fn):
        CASES.append((name, fn, row_bytes))
        return fn
    return deco


def both_shifts(name, row_bytes=0):
    """Registers fn(io, shift) twice: inputs on a 16-byte boundary, and one element past it."""
    def deco(fn):
        for s in (0, 1):
            CASES.append(('%s[shift%d]' % (name, s), (lambda io, s=s: fn(io, s)), row_bytes))
        return fn
    return deco


def host(t):
    if t.dtype == torch.uint16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    if t.dtype == torch.uint64:
        return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)
    return t.cpu().numpy()


class IO:
    """A case's side of one run: placed inputs, caller-owned outputs, results and their references."""

    def __init__(self, poison, guard, memo):
        self.poison, self.guard, self.memo = poison, guard, memo
        self.inputs, self.owned, self.results = [], [], []

    def dev(self, a, shift=0):
        """The array on the device inside a poisoned slab, `shift` elements (0 or 1) past a 16-byte boundary: an input."""
        a = np.ascontiguousarray(a)
        t, tok = place(a, self.poison, shift * a.dtype.itemsize, self.guard, what='input %d %s%s' % (len(self.inputs), a.dtype, list(a.shape)))
        self.inputs.append(tok)
        return t

    def own(self, shape, dtype=F, init=None):
        """A tensor the caller owns and the call may write (out=, ws=, an accumulator): exactly this many bytes inside a poisoned
        slab, filled with the poison (or `init`)."""
        shape = (int(shape),) if np.ndim(shape) == 0 else tuple(int(s) for s in shape)
        if init is None:
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            a = np.full(n, self.poison, np.uint8).view(dtype).reshape(shape)
        else:
            a = np.ascontiguousarray(init, dtype=dtype).reshape(shape)
        t, tok = place(a, self.poison, 0, self.guard, what='caller-owned %d %s%s' % (len(self.owned), np.dtype(dtype), list(shape)))
        self.owned.append(tok)
        return t

    def once(self, key, make):
        """A reference (or an input set) computed once and shared by the three runs."""
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def out(self, label, got, ref=None, tol='bit'):
        got = host(got) if torch.is_tensor(got) else np.asarray(got)
        self.results.append((label, got, None if ref is None else (host(ref) if torch.is_tensor(ref) else np.asarray(ref)), tol))


def compare(got, ref, tol, what):
    if callable(tol):
        tol(got, ref, what)
    elif tol == 'bit':
        if got.dtype == bool or ref.dtype == bool:
            got, ref = got.astype(np.uint8), ref.astype(np.uint8)
        assert_biteq(got, ref.astype(got.dtype) if ref.dtype != got.dtype and got.dtype.kind in 'iu' and ref.dtype.kind in 'iu' else ref, what)
    elif tol[0] == 'ulp':
        assert_ulp(got, ref.astype(F), tol[1], what)
    elif tol[0] == 'rel':
        np.testing.assert_allclose(got, ref, rtol=tol[1], atol=tol[2] if len(tol) > 2 else 0, equal_nan=True, err_msg=what)
    elif tol[0] == 'abs':
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        gn, rn = np.isnan(got), np.isnan(ref)
        assert np.array_equal(gn, rn), what + ': NaN positions differ'
        with np.errstate(invalid='ignore'):
            d = np.abs(np.where(gn, 0, got) - np.where(rn, 0, ref))
            same_inf = np.isinf(got) & (got == ref)
        d[same_inf] = 0
        assert np.all(d <= tol[1]), (what, float(np.max(d - tol[1])))
    else:
        raise AssertionError('unknown tolerance %r' % (tol,))


@pytest.fixture(scope='module')
def side_stream():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.cuda.Stream()


def run(fn, row_bytes, poison, memo, monkeypatch):
    G = guard_width(row_bytes)
    with guarded(monkeypatch, G) as g:
        io = IO(poison, G, memo)
        fn(io)
        for tok in io.inputs:
            unchanged(tok)
        for tok in io.owned:
            intact(tok)
    SEEN.update(g.lib.names())
    return io.results, g.lib.streams()


# ===========================================================================================================================
# the catalogue
def _ops():
    from astrophotography_amd import ops
    return ops


def _apref():
    from oracle import apref
    return apref


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


# ---- elementwise -----------------------------------------------------------------------------------------------------------
def _elementwise(io, shape, shift):
    ops, apref = _ops(), _apref()
    from astrophotography_amd import _lib

    def make():
        rng = np.random.default_rng(shape[0] * 100 + shape[1])
        bias, dark, flat = synth_masters(rng, shape)
        flat.flat[1] = 0.0
        flat.flat[3] = np.nan
        d = dict(bias=bias, dark=dark, flat=flat, raw=synth_cube(rng, 3, shape), rawu=synth_cube(rng, 2, shape, dtype=np.uint16),
                 e=rng.uniform(0.2, 2.0, 3), ped=[0.0, -100.0, 12.5])
        d['nflat'], d['norm'] = apref.flat_normalize(flat)
        d['nflat64'], d['norm64'] = apref.flat_normalize(flat.astype(np.float64))
        d['cal'] = apref.calibrate(d['raw'], bias, dark, d['nflat'], d['e'], d['ped'], True)
        d['calu'] = apref.calibrate(d['rawu'], bias, dark, None, d['e'][:2], None, False)
        d['bias64'] = bias.astype(np.float64) + 1e-9
        d['cal_b64'] = apref.calibrate_mixed(d['raw'], d['bias64'], dark, d['nflat'], d['e'], d['ped'], False)
        d['raw64'] = d['raw'][0].astype(np.float64) + 1e-7
        d['cal_r64'] = apref.calibrate_mixed(d['raw64'], bias, dark, d['nflat64'], d['e'][:1], None, True)
        d['calu_d64'] = apref.calibrate_mixed(d['rawu'], bias, dark.astype(np.float64), None, d['e'][:2], d['ped'][:2], False)
        a, b = d['raw'][0], (d['raw'][1] - 480).astype(F)
        b.flat[2] = 0.0
        d['a'], d['b'] = a, b
        d['arith'] = {(op, k): apref.imarith(a, op, y) for op in ('ADD', 'SUB', 'MUL', 'DIV') for k, y in (('arr', b), ('scl', 3.25))}
        d['arith_u16'] = apref.imarith(d['rawu'][0], 'SUB', d['rawu'][1])
        a64, b64 = a.astype(np.float64) + 1e-9, b.astype(np.float64)
        d['a64'], d['b64'] = a64, b64
        d['arith64'] = {}
        with np.errstate(divide='ignore', invalid='ignore'):
            for op, f in (('ADD', np.add), ('DIV', np.divide)):
                for k, x, y in (('64_64', a64, b64), ('64_32', a64, b), ('32_64', a, b64), ('64_scl', a64, 2.5)):
                    r = np.zeros(x.shape, x.dtype)
                    f(x, y, out=r, casting='same_kind')                    # what core/ApImArith.py:321-333 executes
                    d['arith64'][(op, k)] = r
        d['lo'], d['hi'] = 470.0, 540.0
        d['tmask'], d['nbad'] = apref.threshold_mask(a, d['lo'], d['hi'])
        H, W = shape
        d['rects'] = [[0, H, W - 1, W], [0, 1, 0, 1], [H - 1, H, 0, W], [1, H - 1, 2, W - 2]]
        d['rmask'] = apref.mask_add_rects(d['tmask'], d['rects'], 2)
        d['split'] = apref.bayer_split(d['rawu'][0], (2, 3, 1, 0), (100, 0, 50, 7))
        m1 = (rng.random(shape) < 0.1).astype(np.uint8)
        m2 = (rng.random(shape) < 0.1).astype(np.uint8)
        d['m1'], d['m2'] = m1, m2
        for k, x, y in (('f32', a, b), ('u16', d['rawu'][0], d['rawu'][1])):
            d['diff_' + k] = np.where((m1 | m2) != 0, np.nan, x.astype(np.float64) - y.astype(np.float64))
        return d
    d = io.once('data', make)
    s = shift
    # A1
    for tag, flat, nf, norm in (('f32', d['flat'], d['nflat'], d['norm']), ('f64', d['flat'].astype(np.float64), d['nflat64'], d['norm64'])):
        nflat, n = ops.flat_normalize(io.dev(flat, s))
        io.out('nflat_' + tag, nflat, nf)
        io.out('norm_' + tag, n, np.array([norm], flat.dtype))
    # A2: float32, uint16 raw, the float64 mixes; the output left to ops and given
    bias, dark, nflat = io.dev(d['bias'], s), io.dev(d['dark'], s), io.dev(d['nflat'], s)
    raw, rawu = io.dev(d['raw'], s), io.dev(d['rawu'], s)
    io.out('calibrate_f32', ops.calibrate(raw, bias, dark, nflat, d['e'], d['ped'], True), d['cal'])
    o = io.own(d['raw'].shape)
    ops.calibrate(raw, bias, dark, nflat, d['e'], d['ped'], True, out=o)
    io.out('calibrate_f32_out', o, d['cal'])
    io.out('calibrate_u16', ops.calibrate(rawu, bias, dark, None, d['e'][:2], None, False), d['calu'])
    o = io.own(d['rawu'].shape)
    ops.calibrate(rawu, bias, dark, None, d['e'][:2], None, False, out=o)
    io.out('calibrate_u16_out', o, d['calu'])
    io.out('calibrate_bias64', ops.calibrate(raw, io.dev(d['bias64'], s), dark, nflat, d['e'], d['ped'], False), d['cal_b64'])
    o = io.own(d['raw64'].shape, np.float64)
    ops.calibrate(io.dev(d['raw64'], s), bias, dark, io.dev(d['nflat64'], s), d['e'][:1], None, True, out=o)
    io.out('calibrate_raw64_out', o, d['cal_r64'])
    io.out('calibrate_u16_dark64', ops.calibrate(rawu, bias, io.dev(d['dark'].astype(np.float64), s), None, d['e'][:2], d['ped'][:2], False),
           d['calu_d64'])
    # A8
    a, b = io.dev(d['a'], s), io.dev(d['b'], s)
    for (op, k), ref in d['arith'].items():
        io.out('imarith_%s_%s' % (op, k), ops.imarith(a, op, b if k == 'arr' else 3.25), ref)
    io.out('imarith_u16', ops.imarith(rawu[0], 'SUB', rawu[1]), d['arith_u16'])
    a64, b64 = io.dev(d['a64'], s), io.dev(d['b64'], s)
    for (op, k), ref in d['arith64'].items():
        x, y = {'64_64': (a64, b64), '64_32': (a64, b), '32_64': (a, b64), '64_scl': (a64, 2.5)}[k]
        io.out('imarith_f64_%s_%s' % (op, k), ops.imarith(x, op, y), ref)
    # A4
    mask, nbad = ops.threshold_mask(a, d['lo'], d['hi'])
    io.out('threshold_mask', mask, d['tmask'])
    io.out('threshold_nbad', nbad, np.array([d['nbad']], np.int64))
    mask2, _ = ops.threshold_mask(a, thresholds=io.dev(np.array([d['lo'], d['hi']]), s))
    io.out('threshold_mask_device_thresholds', mask2, d['tmask'])
    m = io.own(d['tmask'].shape, np.uint8, init=d['tmask'])                    # written in place: the caller's
    ops.mask_add_rects(m, d['rects'], 2)
    io.out('mask_add_rects', m, d['rmask'])
    # A9, F2
    io.out('bayer_split', ops.bayer_split(rawu[0], (2, 3, 1, 0), (100, 0, 50, 7)), d['split'])
    m1, m2 = io.dev(d['m1'], s), io.dev(d['m2'], s)
    io.out('image_difference_f32', ops.image_difference(a, b, m1, m2), d['diff_f32'])
    io.out('image_difference_u16', ops.image_difference(rawu[0], rawu[1], m1, m2), d['diff_u16'])
    # FITS payloads: the byte-swapped forms of the arrays, both ways (the round trip of tests/test_gpu_f64.py, without the file)
    lib = _lib.load()
    n = d['a'].size
    u = d['rawu'][0]
    for tag, payload, bitpix, u16, ref in (('u16', (u.astype(np.int32) - 32768).astype('>i2'), 16, 1, u),
                                           ('i16', (u.astype(np.int32) - 32768).astype('>i2'), 16, 0, (u.astype(np.int32) - 32768).astype(F)),
                                           ('f32', d['a'].astype('>f4'), -32, 0, d['a']), ('f64', d['a64'].astype('>f8'), -64, 0, d['a64'])):
        src = io.dev(np.frombuffer(payload.tobytes(), np.uint8))              # a file's payload: torch's own allocation, aligned
        o = io.own(ref.shape, ref.dtype)
        _lib.check(lib.apgpu_fits_decode(_p(src), bitpix, u16, _p(o), n, _stream()))
        io.out('fits_decode_' + tag, o, ref)
    # (the ABI takes 16-byte aligned buffers here and refuses others: no shift)
    for tag, x, fn, be in (('f32', io.dev(d['a']), lib.apgpu_fits_encode_f32, '>f4'), ('f64', io.dev(d['a64']), lib.apgpu_fits_encode_f64, '>f8')):
        o = io.own(n * int(be[2]), np.uint8)
        _lib.check(fn(_p(x), _p(o), n, _stream()))
        io.out('fits_encode_' + tag, o, np.frombuffer((d['a'] if tag == 'f32' else d['a64']).astype(be).tobytes(), np.uint8))


for _shape in ((7, 9), (61, 47), (5, 6), (5, 5)):                # pixel counts 63, 2867 (3 mod 4), 30 (2 mod 4), 25 (1 mod 4)
    both_shifts('elementwise %dx%d' % _shape)(lambda io, s, shape=_shape: _elementwise(io, shape, s))


# ---- sigclip_global ---------------------------------------------------------------------------------------------------------
def _sigclip_global(io, n, shift):
    ops, apref = _ops(), _apref()

    def make():
        rng = np.random.default_rng(n)
        x = rng.normal(20, 3, n).astype(F)
        hot = rng.random(n) < 0.002
        x[hot] = rng.uniform(2000, 6000, hot.sum())
        x[[5, n // 2]] = np.nan
        x[n - 1] = np.inf
        xd = rng.normal(0, 3, n)
        xd[rng.random(n) < 0.002] += 100
        xd[3] = np.nan
        return dict(x=x, xd=xd, r32=apref.sigclip_global(x, sigma=3.0, maxiters=5), r64=apref.sigclip_global(xd, sigma=3.0, maxiters=5))
    d = io.once('data', make)
    for tag, x, r, cast in (('f32', d['x'], d['r32'], F), ('f64', d['xd'], d['r64'], np.float64)):
        s = host(ops.sigclip_global(io.dev(x, shift), sigma=3.0, maxiters=5))
        io.out('stats_' + tag, s[:3].astype(cast), np.array([r['mean'], r['median'], r['std']], cast))
        io.out('bounds_' + tag, s[3:5], np.array([r['lo'], r['hi']]))
        io.out('counts_' + tag, s[5:7].astype(np.int64), np.array([r['niter'], r['nkeep']], np.int64))
        io.out('all_' + tag, s)


for _n in (2047, 2049, 8191, 8193):                              # tile 2048, piece 8192
    both_shifts('sigclip_global n=%d' % _n, row_bytes=8 * _n)(lambda io, s, n=_n: _sigclip_global(io, n, s))


# ---- fix_badpix -------------------------------------------------------------------------------------------------------------
@both_shifts('fix_badpix 61x47')
def _fix_badpix(io, shift):
    ops, apref = _ops(), _apref()
    H, W = 61, 47

    def make():
        rng = np.random.default_rng(11)
        img = rng.normal(1000, 30, (H, W)).astype(F)
        img[5, 7] = np.nan
        mask = (rng.random((H, W)) < 0.03).astype(np.uint8)
        mask[20:27, 10:17] = 1
        mask[0, 0] = mask[0, W - 1] = mask[H - 1, 0] = mask[H - 1, W - 1] = 1      # all four corners
        mask[H - 1, W - 3:] = 1                                                    # the last three pixels of the plane
        d = dict(img=img, mask=mask)
        for dp in (1, 2, 3, 4):
            d['f32', dp] = apref.fix_badpix(img, mask, dp)
            d['f64', dp] = apref.fix_badpix(img.astype(np.float64), mask, dp)
        return d
    d = io.once('data', make)
    x, x64, m = io.dev(d['img'], shift), io.dev(d['img'].astype(np.float64), shift), io.dev(d['mask'], shift)
    for dp in (1, 2, 3, 4):
        for tag, t in (('f32', x), ('f64', x64)):
            out, st = ops.fix_badpix(t, m, dp)
            ref, rs = d[tag, dp]
            io.out('fixed_%s_dp%d' % (tag, dp), out, ref)
            io.out('stats_%s_dp%d' % (tag, dp), st, np.array([rs['nbad'], rs['nfix'], rs['nrem']], np.int64))


# ---- stack ------------------------------------------------------------------------------------------------------------------
def _median_tol(N):
    return ('ulp', 0 if N % 2 else 1)                            # tests/test_gpu_parity.py::test_stack_median_vs_oracle


def _stack(io, N, P, dt, shift):
    ops, apref = _ops(), _apref()

    def make():
        rng = np.random.default_rng(1000 * N + P)
        cube = synth_cube(rng, N, (P,), dtype=dt)
        if dt == F:
            cube[:, 0] = 7.0
            cube[N // 2, 5] = np.nan
        ref = apref.stack_sigclip(cube, sigma=3.0, maxiters=5)
        clean = np.where(np.isfinite(cube), cube, F(500)) if dt == F else cube
        return dict(cube=cube, ref=ref, clean=clean, med=apref.stack_median(clean))
    d = io.once('data', make)
    r = ops.stack_sigclip(io.dev(d['cube'], shift), sigma=3.0, maxiters=5, outputs=('mean', 'median', 'std', 'count'))
    ref = d['ref']
    io.out('count', r['count'], ref['count'])
    io.out('mean', r['mean'], ref['mean'], ('ulp', 1))           # tests/test_gpu_parity.py::test_stack_sigclip_vs_oracle
    io.out('median', r['median'], ref['median'], ('ulp', 1))
    io.out('std', r['std'], ref['std'], ('ulp', 2))
    med, cnt = ops.stack_median(io.dev(d['clean'], shift), want_count=True)
    io.out('stack_median', med, d['med'], _median_tol(N))
    io.out('stack_median_count', cnt, np.full((P,), N, np.int32))


for _N in (3, 13, 64, 65, 128, 129, 130):
    for _P in (1031, 1032):
        for _dt in (F, np.uint16):
            both_shifts('stack N=%d P=%d %s' % (_N, _P, np.dtype(_dt).name), row_bytes=4 * _P)(
                lambda io, s, N=_N, P=_P, dt=_dt: _stack(io, N, P, dt, s))


def _stack_fused(io, N, P, dt, shift):
    """Fused calibration and a pixel mask: tests/test_gpu_parity.py::test_big_stacks_other_paths."""
    ops, apref = _ops(), _apref()

    def make():
        rng = np.random.default_rng(77 + N)
        shape = (P,)
        bias, dark, flat = synth_masters(rng, shape)
        flat[0], flat[1] = 0.0, np.nan
        raw = synth_cube(rng, N, shape, dtype=dt)
        if dt == F:
            raw = raw + bias + F(0.4) * dark
            raw[N // 2, 4] = np.inf
        nflat, _ = apref.flat_normalize(flat)
        e = rng.uniform(0.3, 0.5, N)
        ped = np.where(rng.random(N) < 0.3, -50.0, 0.0)
        pm = (rng.random(shape) < 0.05).astype(np.uint8)
        cal = apref.calibrate(raw.reshape(N, 1, P), bias, dark, nflat, e, ped, True).reshape(N, P)      # (a 2-D raw is one frame)
        return dict(raw=raw, bias=bias, dark=dark, nflat=nflat, e=e, ped=ped, pm=pm, ref=apref.stack_sigclip(cal, pixmask=pm, sigma=3.0, maxiters=5),
                    med=apref.stack_median(cal))
    d = io.once('data', make)
    calib = dict(bias=io.dev(d['bias'], shift), dark=io.dev(d['dark'], shift), nflat=io.dev(d['nflat'], shift), exp_ratio=d['e'], pedestal=d['ped'],
                 dark_still_biased=True)
    raw = io.dev(d['raw'], shift)
    r = ops.stack_sigclip(raw, calib=calib, pixmask=io.dev(d['pm'], shift), sigma=3.0, maxiters=5, outputs=('mean', 'median', 'std', 'count'))
    io.out('count', r['count'], d['ref']['count'])
    io.out('mean', r['mean'], d['ref']['mean'], ('ulp', 1))
    io.out('median', r['median'], d['ref']['median'], ('ulp', 1))
    io.out('std', r['std'], d['ref']['std'], ('ulp', 2))
    io.out('stack_median', ops.stack_median(raw, calib=calib), d['med'], ('ulp', 1))


for _N, _P, _dt in ((13, 1031, F), (64, 1032, np.uint16), (65, 1031, np.uint16), (130, 1032, F)):
    both_shifts('stack fused N=%d P=%d %s' % (_N, _P, np.dtype(_dt).name), row_bytes=4 * _P)(
        lambda io, s, N=_N, P=_P, dt=_dt: _stack_fused(io, N, P, dt, s))


@both_shifts('stack output layouts', row_bytes=4 * 1031)
def _stack_layouts(io, shift):
    """Every `outputs` layout once, the three finalize entry points, the ccdproc configuration on float32 and float64 slabs."""
    ops, apref = _ops(), _apref()
    N, P = 13, 1031

    def make():
        rng = np.random.default_rng(5)
        cube = synth_cube(rng, N, (P,), nan_frac=0.01)
        ref = apref.stack_sigclip(cube, sigma=3.0, maxiters=5)
        kept = np.where(ref['keep'], cube.astype(np.float64), 0.0)
        c64 = rng.normal(500, 20, (N, P))
        c64[rng.random(c64.shape) < 0.02] += 900.0
        return dict(cube=cube, ref=ref, ksum=kept.sum(0), ksq=(kept * kept).sum(0), c64=c64,
                    mad=apref.stack_sigclip(cube, sigma=5.0, maxiters=1, cenfunc='median', stdfunc='mad_std'),
                    ccd={f: apref.combine_ccdproc(c64, 5.0, 5.0, form=f) for f in ('astropy', 'legacy')})
    d = io.once('data', make)
    cube, ref = io.dev(d['cube'], shift), d['ref']
    cnt32 = ref['count'].astype(F)
    sums = ('rel', 3e-7, 1e-30)                                  # tests/test_gpu_parity.py::test_stack_sigclip_vs_oracle
    r = ops.stack_sigclip(cube, sigma=3.0, maxiters=5, outputs=('mean', 'std', 'count', 'mean_f64', 'std_f64', 'moments'))
    io.out('count', r['count'], ref['count'])
    io.out('mean', r['mean'], ref['mean'], ('ulp', 1))
    io.out('mean_f64', r['mean_f64'], ref['mean'], ('rel', 1e-14))           # tests/test_gpu_f64.py::test_stack_float64_planes
    io.out('std_f64', r['std_f64'], ref['std'], ('rel', 1e-12, 1e-300))
    io.out('moments_count', r['moments'][1], cnt32)
    io.out('moments_sum', r['moments'][0].double(), d['ksum'], sums)
    io.out('moments_sumsq', r['moments'][2].double(), d['ksq'], sums)
    mean_a, std_a = host(r['mean']), host(r['std'])

    def near_mean(got, want, what):                              # tests/test_gpu_parity.py::test_stack_properties_large
        ok = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), ok) and np.abs(got[ok] - want[ok]).max() < 1e-3, what

    def near_std(got, want, what):
        ok = np.isfinite(want) & (want > 0)
        assert (np.abs(got[ok] - want[ok]) / want[ok]).max() < 1e-5, what
    io.out('finalize_f32', ops.moments_finalize(r['moments']), mean_a, near_mean)
    for layout in ('moments_f64', 'moments_f64p'):
        m = ops.stack_sigclip(cube, sigma=3.0, maxiters=5, outputs=(layout,))[layout]
        io.out(layout + '_count', m['count'].to(torch.int32), ref['count'])
        io.out(layout + '_sum', m['sum'])
        (mean2, std2), (mean64, std64) = ops.moments_finalize(m, want_f64=True)
        io.out(layout + '_finalize_mean', mean2, mean_a, ('ulp', 1))
        io.out(layout + '_finalize_std', std2, std_a, near_std)
        io.out(layout + '_finalize_mean64_rounds_to_mean', mean64.float(), host(mean2))
        io.out(layout + '_finalize_std64', std64)
        own_mean = io.own((P,))
        ops.moments_finalize(m, want_std=False, out_mean=own_mean)
        io.out(layout + '_finalize_out_mean', own_mean, host(mean2))
    # the ccdproc configuration: one pass about the median with mad_std, float64 planes
    r = ops.stack_sigclip(cube, sigma=5.0, maxiters=1, cenfunc='median', stdfunc='mad_std', outputs=('mean', 'count', 'mean_f64', 'std_f64'))
    io.out('ccdproc_count', r['count'], d['mad']['count'])
    io.out('ccdproc_mean', r['mean'], d['mad']['mean'], ('ulp', 1))
    io.out('ccdproc_mean_f64', r['mean_f64'], d['mad']['mean'], ('rel', 1e-14))
    io.out('ccdproc_std_f64', r['std_f64'], d['mad']['std'], ('rel', 1e-12, 1e-300))
    c64 = io.dev(d['c64'], shift)
    for form in ('astropy', 'legacy'):                            # tests/test_gpu_classes.py: bit for bit the oracle
        rr = ops.combine_f64(c64, form=form)
        io.out('combine_f64_%s_count' % form, rr['count'], d['ccd'][form]['count'])
        io.out('combine_f64_%s_mean' % form, rr['mean_f64'], d['ccd'][form]['mean'])
        io.out('combine_f64_%s_std' % form, rr['std_f64'], d['ccd'][form]['std'])
    # no workspace attached (the library's own temporaries), one kernel, and a caller's workspace
    for tag, kw in (('no_workspace', dict(workspace=False)), ('single_kernel', dict(single_kernel=True)),
                    ('own_workspace', dict(workspace=ops.stack_workspace(P, cube.device)))):
        r = ops.stack_sigclip(cube, sigma=3.0, maxiters=5, outputs=('mean', 'count'), **kw)
        io.out(tag + '_count', r['count'], ref['count'])
        io.out(tag + '_mean', r['mean'], ref['mean'], ('ulp', 1))


# ---- resample ---------------------------------------------------------------------------------------------------------------
@both_shifts('resample 33x70 -> 37x66', row_bytes=4 * 3 * 66)      # the widest plane: block_mean's fine grid, 3 x 66 float32 a row
def _resample(io, shift):
    ops, apref = _ops(), _apref()
    H, W, h, w, N = 33, 70, 37, 66, 5

    def make():
        rng = np.random.default_rng(33)
        yy, xx = np.mgrid[0:H, 0:W]
        frames = (400.0 + 0.05 * xx + 0.03 * yy + rng.normal(0, 6, (N, H, W))).astype(F)
        hits = rng.random(frames.shape) < 0.01
        frames[hits] += rng.uniform(100, 4000, hits.sum()).astype(F)
        frames[1, 10, 11], frames[2, 20, 33] = np.nan, np.inf
        mask = (rng.random((H, W)) < 0.004).astype(np.uint8) * 3
        A = []
        for i in range(N):                                        # registration-sized: a fraction of a degree, a few pixels
            th = np.deg2rad(rng.uniform(-0.3, 0.3))
            A.append([np.cos(th), -np.sin(th), rng.uniform(-3, 3), np.sin(th), np.cos(th), rng.uniform(-3, 3)])
        A = np.array(A)
        A[0] = [1, 0, 0, 0, 1, 0]
        th = np.deg2rad(33.0)
        R = np.array([[np.cos(th), -np.sin(th), 20.0, np.sin(th), np.cos(th), -12.0], [3.5, 0.0, 1.0, 0.0, 4.0, 1.0], [1.0, 0.0, 1e7, 0.0, 1.0, 0.0],
                      [np.nan, 0.0, 0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0, 0.0, 0.0]])
        fs = rng.uniform(0.5, 2.0, N).astype(F)
        d = dict(frames=frames, mask=mask, A=A, R=R, fs=fs)
        d['reg'] = apref.resample_affine(frames, A, fscale=fs, mask=mask, out_shape=(h, w))
        d['rot'] = apref.resample_affine(frames, R, out_shape=(h, w), conserve_flux=True)
        for nph in (1024, 2048):
            res, _ = apref.resample_affine(frames, A, mask=mask, out_shape=(h, w), n_phases=nph)
            d['clip', nph] = apref.stack_sigclip(res, sigma=3.0, maxiters=5)
        res = d['reg'][0]
        d['coadd_clip'] = apref.stack_sigclip(res, sigma=3.0, maxiters=5)
        import warnings
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            d['coadd_med'] = np.nanmedian(res.astype(np.float64), axis=0)
            d['coadd_avg'] = np.nanmean(res.astype(np.float64), axis=0)
            d['coadd_sum'] = np.nansum(res.astype(np.float64), axis=0)
        d['n_ok'] = np.isfinite(res).sum(0).astype(np.int32)
        fine, _ = ops.oversampled_affines(A, 2, (h, w))
        d['over'] = apref.resample_oversampled(frames, fine.numpy(), 2, mask=mask, out_shape=(h, w))[0]
        wts = rng.uniform(0.2, 3.0, N).astype(F)
        num, den = np.zeros((h, w)), np.zeros((h, w))
        for i in range(N):                                        # tests/test_gpu_resample.py::test_weighted_mean...
            ok = np.isfinite(res[i])
            num += np.where(ok, float(wts[i]) * res[i].astype(np.float64), 0.0)
            den += np.where(ok, float(wts[i]), 0.0)
        with np.errstate(invalid='ignore', divide='ignore'):
            d['wmean'] = np.where(den > 0, num / den, np.nan).astype(F)
        d['wsum'], d['wts'] = den.astype(F), wts
        x = rng.normal(0, 1, (3 * h, 3 * w)).astype(F)
        x[5, 7] = np.nan
        d['fine'] = x
        d['block'] = np.array([[F(sum(float(x[3 * i + a, 3 * j + b]) for a in range(3) for b in range(3)) / 9.0) for j in range(w)] for i in range(h)])
        return d
    d = io.once('data', make)
    frames, mask = io.dev(d['frames'], shift), io.dev(d['mask'], shift)
    A = io.dev(d['A'], shift)
    out, wt = ops.resample_affine(frames, A, fscale=d['fs'], mask=mask, out_shape=(h, w))
    io.out('registration', out, d['reg'][0])
    io.out('registration_weight', wt, d['reg'][1])
    o = io.own((N, h, w))
    _, wt = ops.resample_affine(frames, d['A'], fscale=d['fs'], mask=mask, out_shape=(h, w), out=o)
    io.out('registration_out', o, d['reg'][0])
    out, wt = ops.resample_affine(frames, d['R'], out_shape=(h, w), conserve_flux=True)
    io.out('rotated', out, d['rot'][0])
    io.out('rotated_weight', wt, d['rot'][1])
    for nph in (1024, 2048):                                      # tests/test_gpu_resample_stack.py: survivors exact, mean 1 ulp
        r = ops.resample_stack_sigclip(frames, d['A'], mask=mask, out_shape=(h, w), n_phases=nph, sigma=3.0, maxiters=5, outputs=('mean', 'count'))
        io.out('fused_count_%d' % nph, r['count'], d['clip', nph]['count'])
        io.out('fused_mean_%d' % nph, r['mean'], d['clip', nph]['mean'], ('ulp', 1))
    for layout in ('moments', 'moments_f64', 'moments_f64p'):
        r = ops.resample_stack_sigclip(frames, d['A'], mask=mask, out_shape=(h, w), outputs=(layout, 'count'))
        io.out('fused_%s_count' % layout, r['count'], d['clip', 1024]['count'])
        m = r[layout]
        io.out('fused_%s_count_plane' % layout, (m[1] if layout == 'moments' else m['count']).to(torch.int32), d['clip', 1024]['count'])
    kw = dict(fscale=d['fs'], mask=mask, out_shape=(h, w))
    g = ops.coadd(frames, d['A'], combine='CLIPPED', sigma=3.0, maxiters=5, **kw)        # tests/test_gpu_resample.py::test_coadd_pipeline_small_config5
    io.out('coadd_clipped_count', g['count'], d['coadd_clip']['count'])
    io.out('coadd_clipped', g['image'], d['coadd_clip']['mean'], ('ulp', 1))
    g = ops.coadd(frames, d['A'], combine='MEDIAN', **kw)
    io.out('coadd_median', g['image'], d['coadd_med'], ('ulp', 1))
    g = ops.coadd(frames, d['A'], combine='AVERAGE', **kw)
    io.out('coadd_average_count', g['count'], d['n_ok'])
    io.out('coadd_average', g['image'], d['coadd_avg'], ('ulp', 1))
    g = ops.coadd(frames, d['A'], combine='SUM', **kw)
    ok = d['n_ok'] > 0
    io.out('coadd_sum', host(g['image'])[ok], d['coadd_sum'][ok], ('ulp', 1))
    g = ops.coadd(frames, d['A'], combine='CLIPPED', fused=True, mask=mask, out_shape=(h, w))
    io.out('coadd_fused_count', g['count'], d['clip', 1024]['count'])
    io.out('coadd_fused', g['image'], d['clip', 1024]['mean'], ('ulp', 1))
    io.out('oversampled', ops.resample_oversampled(frames, d['A'], 2, mask=mask, out_shape=(h, w)), d['over'])
    io.out('oversampled_two_step', ops.resample_oversampled_two_step(frames, d['A'], 2, mask=mask, out_shape=(h, w)), d['over'])
    res = io.dev(d['reg'][0], shift)
    mean, wsum = ops.weighted_mean(res, d['wts'])
    io.out('weighted_mean', mean, d['wmean'])
    io.out('weighted_sum', wsum, d['wsum'])
    g = ops.coadd(frames, d['A'], combine='WEIGHTED', weights=d['wts'], **kw)
    io.out('coadd_weighted', g['image'], d['wmean'])
    io.out('coadd_weighted_count', g['count'], d['n_ok'])
    io.out('block_mean', ops.block_mean(io.dev(d['fine'], shift), 3), d['block'])


# ---- background / L.A.Cosmic -------------------------------------------------------------------------------------------------
@both_shifts('background and lacosmic 45x67')
def _background(io, shift):
    ops = _ops()
    from oracle import background_ref as br, lacosmic_ref as L
    from scipy import ndimage
    from astrophotography_amd.core.ApMeasureBackground import _bspline3_prefilter
    from tests.test_gpu_background import _sky
    from tests.test_gpu_lacosmic import _field
    H, W = 45, 67

    def make():
        rng = np.random.default_rng(42)
        img = _sky(rng, H, W, nstars=8)
        d = dict(img=img)
        d['smask'], d['nsrc'], thr = br.make_source_mask(img)
        d['above'] = (img > thr).astype(np.uint8)
        im2 = img.copy()
        im2[5, 7] = np.nan
        im2[30:34, 40:50] = np.inf
        d['im2'] = im2
        d['bmask'] = (rng.random((H, W)) < 0.03).astype(np.uint8)
        d['box'] = br.box_clipped_stats(im2, d['bmask'], 16, 20, 3.0, 5)          # a ragged mesh: 3 x 4 boxes over 45 x 67
        d['box_nomask'] = br.box_clipped_stats(im2, None, 16, 20, 3.0, 5)
        mesh = rng.normal(500, 20, (3, 4))
        d['mesh'] = mesh
        d['coef'] = _bspline3_prefilter(mesh)
        d['zoom'] = np.clip(ndimage.zoom(mesh, (16, 20), order=3, mode='reflect', grid_mode=True)[:H, :W], mesh.min(), mesh.max())
        a = rng.normal(100, 20, (H, W)).astype(F)
        d['a'] = a
        d['sepmed'] = {size: L.sepmedfilt(a, size) for size in (5, 7, 9)}
        cr, _ = _field(rng, H, W, ncr=10)
        d['cr'] = cr
        d['lac'] = {fs: L.detect_cosmics(cr, gain=1.0, satlevel=65535.0, fsmode=fs) for fs in ('convolve', 'median')}
        return d
    d = io.once('data', make)
    mask, nsrc = ops.source_mask(io.dev(d['above'], shift), 5, 13)
    io.out('source_mask', host(mask).astype(bool), d['smask'])
    io.out('source_count', nsrc, np.array([d['nsrc']], np.int64))
    im2 = io.dev(d['im2'], shift)
    for tag, m, ref in (('masked', io.dev(d['bmask'], shift), d['box']), ('nomask', None, d['box_nomask'])):
        st = host(ops.box_clipped_stats(im2, m, 16, 20, sigma=3.0, maxiters=5))        # tests/test_gpu_background.py::test_box_clipped_stats_vs_oracle
        med, std, nfin, nm0 = ref
        io.out('box_survivors_' + tag, st[..., 2].astype(np.int64), nfin)
        io.out('box_masked_' + tag, st[..., 3].astype(np.int64), nm0)
        io.out('box_median_' + tag, st[..., 0], med)
        io.out('box_std_' + tag, st[..., 1], std, ('rel', 1e-12))
    z = ops.spline_zoom(io.dev(d['coef'], shift), 16, 20, H, W, d['mesh'].min(), d['mesh'].max())
    io.out('spline_zoom', z, d['zoom'], ('rel', 0, 1e-10))       # tests/test_gpu_background.py::test_spline_zoom_matches_scipy
    a = io.dev(d['a'], shift)
    for size in (5, 7, 9):
        io.out('sepmedfilt_%d' % size, ops.sepmedfilt(a, size), d['sepmed'][size])
    cr = io.dev(d['cr'], shift)
    for fsmode in ('convolve', 'median'):
        clean, crmask, niter = ops.lacosmic(cr, satlevel=65535.0, fsmode=fsmode)
        io.out('lacosmic_mask_' + fsmode, host(crmask).astype(bool), d['lac'][fsmode][1])
        io.out('lacosmic_clean_' + fsmode, clean, d['lac'][fsmode][0])


# ---- autobadcol -------------------------------------------------------------------------------------------------------------
@both_shifts('autobadcol 37x130')
def _autobadcol(io, shift):
    ops = _ops()
    from tests.test_gpu_autobadcol import G13, _data, _np_clip_stats
    H, W, win = 37, 130, 11

    def make():
        rng = np.random.default_rng(37)
        a = (500.0 + 5.0 * rng.standard_normal((H, W))).astype(F)
        a[:, 17] += 200.0
        a[9, :] -= 150.0
        a[rng.random((H, W)) < 0.01] = np.nan
        a[:, 3] = np.nan
        a[5, 100] = np.inf
        d = dict(a=a, a64=a.astype(np.float64), u=np.clip(np.nan_to_num(a, nan=0.0, posinf=65535.0), 0, 65535).astype(np.uint16))
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for k in ('a', 'a64', 'u'):
                d['med', k] = [np.nanmedian(d[k], axis=ax) for ax in (0, 1)]
            v = np.where(np.isfinite(d['med', 'a'][0]), d['med', 'a'][0], F(500))       # the 130 column medians as one clean line
            d['line'] = v
            hw = (win - 1) // 2
            wins = [_np_clip_stats(v[max(0, i - hw):i + hw + 1]) for i in range(v.size)]
            d['line_mean'] = np.array([np.nanmean(x) for x in wins], np.float64)         # tests/test_gpu_autobadcol.py::test_long_lines_exact
            d['line_std'] = np.array([np.nanstd(x) for x in wins], np.float64)
        return d
    d = io.once('data', make)
    for k in ('a', 'a64', 'u'):
        t = io.dev(d[k], shift)
        for ax in (0, 1):
            io.out('nanmedian_%s_axis%d' % (k, ax), ops.axis_nanmedian(t, ax), d['med', k][ax])
    slab = io.dev(np.stack([d['a'], d['a'][::-1]]), shift)
    io.out('nanmedian_slab', ops.axis_nanmedian(slab, 0), np.stack([d['med', 'a'][0], d['med', 'a'][0]]))
    r = ops.sliding_clipped_stats(io.dev(d['line'], shift), win)
    io.out('sliding_mean', r['mean'], d['line_mean'])
    io.out('sliding_std', r['std'], d['line_std'])
    io.out('sliding_nsig', r['nsig'])
    io.out('sliding_flag', r['flag'])
    r = ops.auto_badcols(io.dev(d['a'], shift), window_len=win)
    for tag in ('cols', 'rows'):
        for k in ('median', 'mean', 'std', 'nsig', 'flag'):
            io.out('auto_%s_%s' % (tag, k), r[tag][k], d['med', 'a'][0 if tag == 'cols' else 1] if k == 'median' else None)
    # the reference's own numbers (golden group G13) for every output of the composite
    name = 'u16_odd'
    r = ops.auto_badcols(io.dev(_data(name), shift), nsigma=float(G13[name + '/nsigma']), window_len=int(G13[name + '/window']))
    for tag in ('cols', 'rows'):
        io.out('g13_%s_median' % tag, r[tag]['median'], G13['%s/med_%s' % (name, tag)])
        for k in ('mean', 'std', 'nsig', 'flag'):
            io.out('g13_%s_%s' % (tag, k), r[tag][k], G13['%s/%s_%s' % (name, k, tag)])


# ---- find / measure / register -----------------------------------------------------------------------------------------------
@both_shifts('findstars', row_bytes=4 * 200)                     # the widest plane: the 64 x 200 image of spikes_image()
def _findstars(io, shift):
    ops = _ops()
    from tests.test_gpu_findstars import EPS, SKY, add_star, field, measure_bounds, phot_bound, quant, spikes_image

    def make():
        d = {}
        img = field(40, 70, seed=12, nstars=3)
        img[5, 5], img[20, 64], img[39, 0] = np.nan, np.inf, -np.inf
        k3 = fm.daofind_kernel(3.0)
        d['cimg'], d['conv_ref'] = img, fm.convolve(fm.subtract_bg(img, SKY), k3['K'])
        d['tiny'] = field(3, 4, seed=11, nstars=6)                                        # smaller than the kernel
        d['tiny_ref'] = fm.convolve(fm.subtract_bg(d['tiny'], SKY), k3['K'])
        sp, pos = spikes_image()
        d['spikes'], d['pos'] = sp, np.array(sorted(i * sp.shape[1] + j for i, j in pos), np.int64)
        d['pmask'] = np.zeros(sp.shape, np.uint8)
        d['pmask'][:, :8] = 1
        d['peaks_masked'] = fm.find_peaks(sp, np.ones((5, 5)), SKY + 500.0, mask=d['pmask'], border=2)
        # tests/test_gpu_findstars.py::test_measure_matches_the_model, fwhm 3
        fwhm, H, W = 3.0, 97, 131
        rng = np.random.default_rng(31)
        stars = [(rng.uniform(8, H - 8), rng.uniform(8, W - 8), rng.uniform(300, 6000), fwhm / 2.3548 * rng.uniform(0.8, 1.3)) for _ in range(22)]
        im = field(H, W, seed=32, nstars=0, noise=3.0, stars=stars).astype(np.float64)
        for t in range(10):
            i, j = int(rng.integers(14, H - 14)), int(rng.integers(14, W - 14))
            if t % 2:
                im[i, j] += 3000.0
            else:
                add_star(im, i, j, 900.0, 0.9)
                add_star(im, i, j + 2.0 * fwhm / 3.0, 850.0, 0.9)
        im = quant(im)
        im[50, 60] = np.nan
        thr_eff = 18.0 * k3['relerr']
        sub = fm.subtract_bg(im, SKY)
        conv = fm.convolve(sub, k3['K'])
        peaks = fm.find_peaks(conv, k3['fp'], thr_eff, border=k3['R'])
        m = fm.daofind_measure(sub, conv, peaks, k3, thr_eff)
        d.update(mimg=im, mconv=conv, peaks=peaks, m=m, bound=measure_bounds(m, k3, thr_eff), thr_eff=thr_eff, k3=k3)
        # tests/test_gpu_findstars.py::test_aperture_photometry_matches_the_model, fwhm 3
        r, r_in, r_out = fm.aperture_radii(fwhm)
        ph = field(H, W, seed=41, nstars=0, noise=3.0, stars=[(48.0, 60.0, 4000.0, 1.4), (48.0 + 1.2 * r, 60.0 + 0.3 * r, 9000.0, 1.4), (20.0, 100.0, 2500.0, 1.4)])
        ph[48, 60 - int(r) - 2], ph[47, 60 - int(r) - 2] = np.nan, np.inf
        xc = [60.0, 100.0, 30.5, 30.0, 77.5, 41.37, 88.113, 0.0, 3.3, 130.0, 128.6, 65.2, 64.0, 0.4, 129.9, 1.7, 129.2, -3.0, 135.0, 64.25]
        yc = [48.0, 20.0, 70.0, 70.5, 30.5, 66.81, 71.004, 50.0, 44.4, 52.0, 60.1, 0.0, 96.0, 0.3, 0.2, 95.8, 96.0, 40.0, 99.5, 2.5]
        pref = fm.aperture_photometry(ph, xc, yc, fwhm)
        d.update(ph=ph, xc=xc, yc=yc, pref=pref, pbound=phot_bound(ph, xc, yc, r, pref),
                 abound=pref['npix'] * EPS * pref['area'] + 16 * EPS * r * r * 8 * (r + 1))
        return d
    d = io.once('data', make)
    io.out('convolve', ops.daofind_convolve(io.dev(d['cimg'], shift), d['k3'], bg_median=SKY), d['conv_ref'])
    io.out('convolve_tiny', ops.daofind_convolve(io.dev(d['tiny'], shift), 3.0, bg_median=SKY), d['tiny_ref'])
    sp = io.dev(d['spikes'], shift)
    idx, n = ops.local_peaks(sp, 5, SKY + 500.0)
    io.out('peaks_all', idx.to(torch.int64), d['pos'])
    io.out('peaks_all_count', np.array([n]), np.array([200]))
    idx, n = ops.local_peaks(sp, np.ones((5, 5)), SKY + 500.0, mask=io.dev(d['pmask'], shift), border=2)
    io.out('peaks_masked', idx.to(torch.int64), d['peaks_masked'])

    def short_list(got, want, what):                             # 64 distinct members of the 200, which ones is up to the scheduling
        assert got.size == 64 and len(set(got.tolist())) == 64 and set(got.tolist()) <= set(want.tolist()), what
    buf = io.own(64, np.int32)                                    # exactly the capacity: 200 peaks must not run over it
    idx, n = ops.local_peaks(sp, 5, SKY + 500.0, capacity=64, list_out=buf)
    io.out('peaks_short_list_own', buf, d['pos'], short_list)
    io.out('peaks_short_count_own', np.array([n]), np.array([200]))
    idx, n = ops.local_peaks(sp, 5, SKY + 500.0, capacity=64)     # the list left to ops: the proxy guards it
    io.out('peaks_short_list', idx, d['pos'], short_list)
    io.out('peaks_short_count', np.array([n]), np.array([200]))
    buf0 = io.own(4, np.int32, init=np.full(4, -7, np.int32))
    _, n = ops.local_peaks(sp, 5, SKY + 500.0, capacity=0, list_out=buf0)
    io.out('peaks_capacity_0_untouched', buf0, np.full(4, -7, np.int32))
    # measurement
    m, bound, col = d['m'], d['bound'], {nm: i for i, nm in enumerate(fm.REC)}
    rec, keep = ops.daofind_measure(io.dev(d['mimg'], shift), io.dev(d['mconv'], shift), io.dev(d['peaks'].astype(np.int32), shift), d['k3'],
                                    d['thr_eff'], bg_median=SKY)
    io.out('measure_keep', host(keep).astype(bool), m['keep'])
    fin = np.isfinite(m['rec']).all(axis=1)

    def within(got, want, what):
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        assert np.all(np.abs(got[fin] - want[fin]) <= bound[fin]), what
    io.out('measure_records', rec, m['rec'], within)
    r = ops.find_stars(io.dev(d['mimg'], shift), 3.0, 18.0, bg_median=SKY, capacity=16)          # more candidates than the list holds: repeated
    io.out('find_stars_idx', r['idx'].to(torch.int64), d['peaks'][m['keep']])
    io.out('find_stars_conv', r['conv'], d['mconv'])
    # photometry
    pref = d['pref']
    got = ops.aperture_photometry(io.dev(d['ph'], shift), d['xc'], d['yc'], 3.0)
    io.out('phot_n_annulus', got['n_annulus'].to(torch.int64), pref['n_annulus'])
    io.out('phot_bkg_median', got['bkg_median'], pref['bkg_median'])
    pf = np.isfinite(pref['aperture_sum_raw'])

    def sums(g, want, what):
        assert np.array_equal(np.isfinite(g), pf) and np.all(np.abs(g - want)[pf] <= d['pbound'][pf]), what
    io.out('phot_sum_raw', got['aperture_sum_raw'], pref['aperture_sum_raw'], sums)
    io.out('phot_area', got['area'], pref['area'], ('abs', d['abound']))


@both_shifts('gauss2d_fit')
def _gauss2d(io, shift):
    ops = _ops()
    from tests.test_gpu_measurestars import bounds, synthetic
    k = 1                                                         # the golden case with the smallest box (12 pixels)
    c = msm.case(k)
    ref = c['res']
    got = ops.gauss2d_fit(io.dev(c['img'], shift), ref['xcenter'], ref['ycenter'], ref['peak_adu'], ref['bgmed_per_pix'], c['init_fwhm'])
    b_par, b_chi2, b_err, _ = bounds()

    # The fit's columns are host arrays of a dict, so the family's check is a callable over the whole dict: it reads `got` from this
    # run's closure and the arrays handed to io.out with it are placeholders.  It holds run A (and is not applied to B and C); runs B
    # and C are held by the bit comparison of every column, the 'golden_*' / 'corner_*' results below.
    def fits(_, __, what):                                        # tests/test_gpu_measurestars.py::test_fits_match_the_reference
        assert np.array_equal(got['fit_ok'], ref['fit_ok']), what
        for nm in ('xmin', 'xmax', 'ymin', 'ymax'):
            assert np.array_equal(got[nm], ref[nm]), (what, nm)
        for i in np.nonzero(ref['fit_ok'])[0]:
            x0, y0 = ref['xmin'][i], ref['ymin'][i]
            pr, er, _s = msm.canonical(*msm.params(ref, i, x0, y0))
            pg, eg, _t = msm.canonical(*msm.params(got, i, x0, y0))
            dd = np.abs(pg - pr) / er
            round_star = (pr[3] - pr[4]) < 3.0 * math.hypot(er[3], er[4])
            dd[5] = 0.0 if round_star else msm.angle_diff(pg[5], pr[5]) / er[5]
            de = np.abs(eg / er - 1.0)
            if round_star:
                de[5] = 0.0
            assert dd.max() <= b_par and de.max() <= b_err, (what, i, dd, de)
            assert abs(got['rchisq'][i] - ref['rchisq'][i]) / ref['rchisq'][i] <= b_chi2, (what, i)
            assert got['circular'][i] == ref['circular'][i], (what, i)
    io.out('golden_fits', np.zeros(1), np.zeros(1), fits)
    for col in ops.GAUSS2D_COLUMNS + ('bg_fit', 'niter'):
        io.out('golden_' + col, np.asarray(got[col]).astype(np.float64))
    # a 12-pixel box against the image corner, on a frame no larger than the box (test_box_sizes_corner_cap_and_empty_box)
    img = io.once('corner', lambda: synthetic(12, 12, 6.2, 5.7, 2.0))
    r = ops.gauss2d_fit(io.dev(img, shift), [5.7], [6.2], [4000.0], [50.0], 1.5)

    def corner(_, __, what):
        assert (r['xmin'][0], r['ymax'][0]) == (0, 12) and r['fit_ok'][0], what
        assert abs(r['fwhm_x'][0] - 2.0) < 0.1 and abs(r['fwhm_y'][0] - 2.0) < 0.1, what
        assert abs(r['xc_fit'][0] - 6.2) < 0.05 and abs(r['yc_fit'][0] - 5.7) < 0.05, what
    io.out('corner_fit', np.zeros(1), np.zeros(1), corner)
    for col in ops.GAUSS2D_COLUMNS + ('bg_fit', 'niter'):
        io.out('corner_' + col, np.asarray(r[col]).astype(np.float64))


@both_shifts('register')
def _register(io, shift):
    ops = _ops()
    K = 40

    def make():
        A = rm.make_affine(178.3, 1.004, shift=(11.0, -21.0))
        p0, p1, _, _ = rm.make_field(21, A)
        xy, count = rm.pad_lists([p0[:40], p1[:40], p0[:10], p0[:0], p0[:2], p0[:3]], M=40)          # short and empty lists among them
        tris, m1 = rm.triangle_build(xy, count, K=K)
        votes = {mir: rm.triangle_vote(tris, K=K, allow_mirror=mir) for mir in (False, True)}
        assert min(m1, votes[False][1], votes[True][1]) >= 1e-9                              # no decision of the model within rounding
        ref = np.array([[10.0, 10.0], [50.0, 50.0], [200.0, 200.0], [300.0, 300.0]])
        frm = np.array([[13.0, 10.0], [7.0, 10.0], [10.0, 13.0], [53.0, 54.0], [90.0, 90.0], [200.0, 205.0], [200.0, 195.0]])
        xy2, count2 = rm.pad_lists([ref, frm, ref[:1], ref[:0]])
        T = np.tile(rm.IDENTITY, (4, 1))
        T[2] = [0.0, -1.0, 0.0, 1.0, 0.0, 0.0]
        return dict(xy=xy, count=count, tris=tris, votes=votes, xy2=xy2, count2=count2, T=T,
                    nn={rad: rm.nearest_match(xy2, count2, T, rad) for rad in (3.0, 5.0)})
    d = io.once('data', make)
    xy, count = io.dev(np.asarray(d['xy'], np.float64), shift), io.dev(np.asarray(d['count'], np.int32), shift)
    tri = ops.triangle_build(xy, count, K=K)
    io.out('triangle_count', tri['count'], np.array([len(t['x']) for t in d['tris']], np.int32))
    for f, (dv, mo) in enumerate(zip(ops.triangle_unpack(tri), d['tris'])):              # the order of a frame's list carries no meaning
        ds, ms = rm.triangle_set(dv), rm.triangle_set(mo)
        keys = sorted(ms)
        io.out('triangle_keys_%d' % f, np.array(sorted(ds), np.int64).reshape(-1, 4), np.array(keys, np.int64).reshape(-1, 4))
        io.out('triangle_invariants_%d' % f, np.array([ds.get(k, (np.nan, np.nan)) for k in keys]).reshape(-1, 2),
               np.array([ms[k] for k in keys]).reshape(-1, 2))
    for mir in (False, True):
        io.out('votes_mirror%d' % mir, ops.triangle_vote(tri, allow_mirror=mir), d['votes'][mir][0].astype(np.int32))
    xy2, count2 = io.dev(np.asarray(d['xy2'], np.float64), shift), io.dev(np.asarray(d['count2'], np.int32), shift)
    for rad in (3.0, 5.0):
        r = ops.nearest_match(xy2, count2, d['T'], rad)
        for name, want in zip(('fwd_idx', 'fwd_d2', 'bwd_idx', 'bwd_d2'), d['nn'][rad]):
            io.out('nearest_%s_r%g' % (name, rad), r[name], want)


# ---- composite / demosaic ----------------------------------------------------------------------------------------------------
def _composite(io, W, shift):
    ops = _ops()
    H = 7
    Q = [[0.01, 0.995], [0.02, 0.99], [0.0, 1.0]]

    def make():
        rng = np.random.default_rng(W)
        planes = rng.normal(100.0, 30.0, (3, H, W)).astype(F)
        planes[0, 2, 3], planes[1, 0, W - 1], planes[2, H - 1, W - 1] = np.nan, np.inf, -np.inf
        lv, nf = cpm.quantile_levels(planes, Q)
        grid = [(1.0, 1.0), (0.8, 1.6), (1.3, 0.0)]
        tables, sat = np.stack([cpm.tone_table(2.2, gf) for gf, _ in grid]), [cs for _, cs in grid]
        levels = np.array([[40.0, 180.0], [35.0, 170.0], [50.0, 190.0]], F)
        return dict(planes=planes, lv=lv, nf=nf, tables=tables, sat=sat, levels=levels,
                    rgb={(bits, flip): cpm.composite_rgb(planes, levels, tables, sat, bits=bits, flip=flip) for bits in (8, 16) for flip in (True, False)})
    d = io.once('data', make)
    planes = io.dev(d['planes'], shift)
    lv, nf = ops.quantile_levels(planes, Q)
    io.out('levels', lv, d['lv'])
    io.out('n_finite', nf, d['nf'])
    levels, tables = io.dev(d['levels'], shift), io.dev(d['tables'], shift)
    for (bits, flip), want in d['rgb'].items():
        io.out('rgb_%d_flip%d' % (bits, flip), ops.composite_rgb(planes, levels, tables, d['sat'], bits=bits, flip=flip), want)
        o = io.own(want.shape, want.dtype)
        ops.composite_rgb(planes, levels, tables, d['sat'], bits=bits, flip=flip, out=o)
        io.out('rgb_%d_flip%d_out' % (bits, flip), o, want)


def _demosaic(io, W, shift):
    ops = _ops()
    from tests.test_gpu_demosaic import _mosaic
    gain, black = (1.8371, 1.0, 1.4142, 1.0007), [256, 250, 300, 255]
    region = (1, 5, 3, W - 2)

    def make():
        d = {}
        for H in (6, 7):
            for dt in (np.uint16, F):
                m = _mosaic((H, W), 100 + W + H, dt)
                if dt == F:
                    m[1, 2], m[H - 1, W - 1] = np.nan, np.inf
                d['m', H, dt] = m
        return d
    d = io.once('data', make)
    pats = sorted(dmm.ARRANGEMENTS.items())
    k = 0
    for H in (6, 7):
        for dt in (np.uint16, F):
            m = d['m', H, dt]
            t = io.dev(m, shift)
            tag = '%d_%s' % (H, np.dtype(dt).name)
            for method in ('bilinear', 'mhc', 'superpixel'):
                for output in ('rgb', 'rgb_u16', 'grey', 'direct'):
                    if (method == 'superpixel' and (H % 2 or W % 2)) or (output == 'direct' and method != 'bilinear'):
                        continue
                    pat = pats[k % len(pats)][1]
                    k += 1
                    want = io.once(('want', tag, method, output), lambda: dmm.demosaic(m, pat, black, gain, method, output))
                    if k % 2:
                        got = ops.bayer_demosaic(t, pat, black, gain, method, output)
                    else:
                        got = io.own(want.shape, want.dtype)
                        ops.bayer_demosaic(t, pat, black, gain, method, output, out=got)
                    io.out('demosaic_%s_%s_%s' % (tag, method, output), got, want)
            pat = pats[H % len(pats)][1]
            want_s, want_n, mags = io.once(('sums', tag), lambda: dmm.channel_sums(m, pat, black, region))
            sums, counts = ops.bayer_channel_sums(t, pat, black, region)
            io.out('channel_counts_' + tag, counts, np.array(want_n, np.int64))
            if dt == np.uint16:
                io.out('channel_sums_u16_' + tag, sums, np.array(want_s, np.uint64))
            else:
                io.out('channel_sums_f32_' + tag, sums, np.array(want_s), ('abs', np.array(want_n) * 2.0 ** -53 * np.array(mags)))
    slab = np.stack([d['m', 6, np.uint16], d['m', 6, np.uint16][::-1]])
    want = io.once('slab', lambda: np.stack([dmm.demosaic(f, (0, 1, 3, 2), None, None, 'mhc', 'rgb') for f in slab]))
    io.out('demosaic_slab', ops.bayer_demosaic(io.dev(slab, shift)), want)


for _W in (62, 63, 64, 65):
    # the widest row a composite call is given is a tone table's (APGPU_TONE_TABLE_LEN float32), not a plane's
    both_shifts('composite width %d' % _W, row_bytes=4 * TONE_TABLE_LEN)(lambda io, s, W=_W: _composite(io, W, s))
    both_shifts('demosaic width %d' % _W)(lambda io, s, W=_W: _demosaic(io, W, s))


# ---- continuum --------------------------------------------------------------------------------------------------------------
def _continuum(io, shape, shift):
    ops = _ops()
    from astrophotography_amd import _lib
    from tests.test_gpu_continuum import _image, _moment_case, _taps
    H, W = shape

    def make():
        rng = np.random.default_rng(H * 100 + W)
        d = dict(img=_image(rng, H, W, 'isolated'))
        for R in (1, 31, 32):
            d['blur', R] = ctm.gauss_blur(d['img'], _taps(R), 0.5)
        n, c, mask = _moment_case(rng, shape)
        d.update(n=n, c=c, mask=mask)
        for tag, mk, args in (('all', None, (0.0, 0.0, -np.inf, np.inf)), ('clipped', mask, (0.1, 2.0, -1.5, 1.0))):
            want = ctm.pair_moments(n, c, *args, mk)
            absum = ctm.moment_terms_abs(n, c, *args, mk)
            d['mom', tag] = (want, np.array([0.0] + [2.0 * want[0] * 2.0 ** -53 * absum[k] for k in range(1, 6)]), mk is not None, args)
        y = c.copy()
        d['comb'] = {(ca, cb, c0): ctm.linear_combine(n, y, ca, cb, c0) for ca, cb, c0 in ((1.0, -0.083, -0.4), (0.5, 2.0, 0.0))}
        d['comb1'] = ctm.linear_combine(n, None, 2.0, 0.0, 1.5)
        return d
    d = io.once('data', make)
    img = io.dev(d['img'], shift)
    for R in (1, 31, 32):
        io.out('blur_R%d' % R, ops.gauss_blur(img, _taps(R), 0.5), d['blur', R])
        o = io.own(shape)
        ops.gauss_blur(img, _taps(R), 0.5, out=o)
        io.out('blur_R%d_out' % R, o, d['blur', R])
    n, c, mask = io.dev(d['n'], shift), io.dev(d['c'], shift), io.dev(d['mask'], shift)
    need = _lib.load().apgpu_pair_moments_ws_bytes(n.numel())
    for tag in ('all', 'clipped'):
        want, bound, masked, args = d['mom', tag]
        for own in (False, True):                                 # tests/test_gpu_continuum.py::_check_moments
            ws = io.own(need, np.uint8) if own else None          # exactly the bytes the query reports
            io.out('moments_%s%s' % (tag, '_ws' if own else ''), ops.pair_moments(n, c, *args, mask if masked else None, ws), want, ('abs', bound))
    for (ca, cb, c0), want in d['comb'].items():
        io.out('combine_%g_%g_%g' % (ca, cb, c0), ops.linear_combine(n, c, ca, cb, c0), want)
        o = io.own(shape)
        ops.linear_combine(n, c, ca, cb, c0, out=o)
        io.out('combine_%g_%g_%g_out' % (ca, cb, c0), o, want)
    io.out('combine_y_none', ops.linear_combine(n, None, 2.0, 0.0, 1.5), d['comb1'])
    acc = io.own(shape, F, init=d['n'])                           # out may be x: in place on the caller's tensor
    ops.linear_combine(acc, None, 2.0, 0.0, 1.5, out=acc)
    io.out('combine_in_place', acc, d['comb1'])


for _shape in ((33, 65), (31, 63), (5, 3)):                      # tile 32 x 64
    both_shifts('continuum %dx%d' % _shape)(lambda io, s, shape=_shape: _continuum(io, shape, s))


# ---- deconvolve -------------------------------------------------------------------------------------------------------------
def _deconvolve(io, shape, shift):
    ops = _ops()
    from astrophotography_amd import _lib
    from tests.test_gpu_deconvolve import GAIN, RN, _image, _psf
    H, W = shape

    def make():
        rng = np.random.default_rng(H * 100 + W)
        img = _image(rng, H, W, 'isolated')
        u = (rng.random(shape) * 250.0 + 1.0).astype(F)
        d = dict(img=img, u=u, plane=(rng.random(shape) * 100.0 + 150.0).astype(F))
        for R in (0, 1, 12):
            p = _psf(rng, R)
            inv = dcm.norm(img, p)
            r = dcm.ratio(u, img, p, 95.0, GAIN, RN, 3.0)
            d['R', R] = dict(p=p, inv=inv, ratio=r, ratio0=dcm.ratio(u, img, p, 95.0, GAIN, RN, 0.0), update=dcm.update(u, r, inv, p))
        p = d['R', 1]['p']
        for niter in (0, 2):
            d['rl', niter, 'plane'] = dcm.richardson_lucy(img, p, 95.0, niter, 3.0, GAIN, RN, start=d['plane'])[0]
            d['rl', niter, 'scalar'] = dcm.richardson_lucy(img, p, 95.0, niter, 3.0, GAIN, RN, start=F(187.5))[0]
        return d
    d = io.once('data', make)
    img, u = io.dev(d['img'], shift), io.dev(d['u'], shift)
    for R in (0, 1, 12):
        k = d['R', R]
        p = k['p']
        for own in (False, True):
            tag = 'R%d%s' % (R, '_out' if own else '')
            o = [io.own(shape) if own else None for _ in range(4)]
            io.out('norm_' + tag, ops.deconv_norm(img, p, out=o[0]), k['inv'])
            io.out('ratio_T0_' + tag, ops.deconv_ratio(u, img, p, 95.0, GAIN, RN, 0.0, out=o[1]), k['ratio0'])
            io.out('ratio_T3_' + tag, ops.deconv_ratio(u, img, p, 95.0, GAIN, RN, 3.0, out=o[2]), k['ratio'])
            io.out('update_' + tag, ops.deconv_update(u, io.dev(k['ratio'], shift), io.dev(k['inv'], shift), p, out=o[3]), k['update'])
    p = d['R', 1]['p']
    need = _lib.load().apgpu_deconv_ws_bytes(H, W)
    plane = io.dev(d['plane'], shift)
    for niter in (0, 2):
        for name, start in (('plane', plane), ('scalar', 187.5)):
            got, _ = ops.richardson_lucy(img, p, 95.0, niter, 3.0, GAIN, RN, start=start)
            io.out('rl_%d_%s' % (niter, name), got, d['rl', niter, name])
            o, ws = io.own(shape), io.own(need, np.uint8)         # the caller's output and a workspace of exactly the reported bytes
            ops.richardson_lucy(img, p, 95.0, niter, 3.0, GAIN, RN, start=start, ws=ws, out=o)
            io.out('rl_%d_%s_own' % (niter, name), o, d['rl', niter, name])
    got, rep = ops.richardson_lucy(img, p, 95.0, 2, 3.0, GAIN, RN)                      # the default start: its level goes to the model
    want = io.once(('rl_default', rep['start']), lambda: dcm.richardson_lucy(d['img'], p, 95.0, 2, 3.0, GAIN, RN, start=F(rep['start']))[0])
    io.out('rl_default_start', got, want)
    io.out('rl_default_level', np.array([rep['start']]))


for _shape in ((33, 65), (32, 64), (3, 5)):
    both_shifts('deconvolve %dx%d' % _shape)(lambda io, s, shape=_shape: _deconvolve(io, shape, s))


# ---- multiscale -------------------------------------------------------------------------------------------------------------
def _multiscale(io, shape, shift):
    ops = _ops()
    from astrophotography_amd import _lib
    from tests.test_gpu_multiscale import _image
    H, W = shape

    def make():
        rng = np.random.default_rng(H * 100 + W)
        img = _image(rng, H, W, 'isolated')
        prev = rng.normal(0.0, 50.0, shape).astype(F)
        d = dict(img=img, prev=prev)
        with np.errstate(invalid='ignore'):
            for s in (1, 2, 32):
                cn = mlm.step(img, s)
                w = (img - cn).astype(F)
                acc = prev + F(2.5) * mlm.treat(w, F(30.0), 'soft') + F(0.75) * cn       # tests/test_gpu_multiscale.py::test_step_accumulates
                d['step', s] = (cn, np.where(np.isfinite(img), w, F(np.nan)).astype(F), np.where(np.isfinite(img), acc, F(np.nan)).astype(F))
        for J in (1, 6):
            d['planes', J] = mlm.planes(img, J)
            k, gains = (3.0, 0.0, 2.0, 1.0, 4.0, 0.5)[:J], (2.5, 0.0, 1.0, 1.7, 0.0, 0.6)[:J]
            d['ms', J] = (k, gains, mlm.multiscale(img, J, k, gains, 0.8, 'hard', sigma=40.0)[0])
        return d
    d = io.once('data', make)
    img = io.dev(d['img'], shift)
    for s in (1, 2, 32):
        cn, w, acc = d['step', s]
        # the tile form exists up to APGPU_STARLET_TILE_MAX_SPACING = 8 (the library refuses it beyond): spacing 32 runs 'direct', and
        # 'auto', which must choose it
        for form in (('tile', 'direct') if s <= 8 else ('direct', 'auto')):
            tag = 's%d_%s' % (s, form)
            plane = io.own(shape)
            io.out('step_c_' + tag, ops.starlet_step(img, s, plane=plane, form=form), cn)
            io.out('step_w_' + tag, plane, w)
            o, plane, a = io.own(shape), io.own(shape), io.own(shape, F, init=d['prev'])
            ops.starlet_step(img, s, out=o, plane=plane, acc=a, threshold=30.0, gain=2.5, g_res=0.75, mode='soft', first=False, last=True, form=form)
            io.out('step_own_c_' + tag, o, cn)
            io.out('step_own_w_' + tag, plane, w)
            io.out('step_own_acc_' + tag, a, acc)
    io.out('plane1', ops.starlet_plane1(img), d['planes', 1][0][0])
    o = io.own(shape)
    ops.starlet_plane1(img, out=o)
    io.out('plane1_out', o, d['planes', 1][0][0])
    need = _lib.load().apgpu_starlet_ws_bytes(H, W)
    for J in (1, 6):
        ws_ref, cJ = d['planes', J]
        want = np.stack(list(ws_ref) + [cJ])
        io.out('planes_J%d' % J, ops.starlet_planes(img, J), want)
        o, ws = io.own((J + 1, H, W)), io.own(need, np.uint8)
        ops.starlet_planes(img, J, ws=ws, out=o)
        io.out('planes_J%d_own' % J, o, want)
        k, gains, want = d['ms', J]
        io.out('multiscale_J%d' % J, ops.multiscale(img, J, k, gains, 0.8, 'hard', sigma=40.0)[0], want)
        o, ws = io.own(shape), io.own(need, np.uint8)
        ops.multiscale(img, J, k, gains, 0.8, 'hard', sigma=40.0, ws=ws, out=o)
        io.out('multiscale_J%d_own' % J, o, want)
    got, rep = ops.multiscale(img, 2, 3.0)                        # the noise measured on the device (plane 1, the global clip): the model
    want = io.once(('measured', rep['sigma']), lambda: mlm.multiscale(d['img'], 2, 3.0, sigma=rep['sigma'])[0])      # given that value
    io.out('multiscale_measured_sigma', got, want)                # (tests/test_gpu_multiscale.py::test_class_reproduces_the_model)
    io.out('measured_sigma', np.array([rep['sigma']]))


for _shape in ((33, 65), (40, 68)):
    both_shifts('multiscale %dx%d' % _shape)(lambda io, s, shape=_shape: _multiscale(io, shape, s))


# ---- drizzle ----------------------------------------------------------------------------------------------------------------
@both_shifts('drizzle 7x9 -> 5x65')
def _drizzle(io, shift):
    ops = _ops()
    from tests.test_gpu_drizzle import _affines, _frames
    H, W, N = 7, 9, 5
    out_shape = (5, 65)                                           # tile 4 x 64

    def make():
        rng = np.random.default_rng(21)
        fr, mask, fmask = _frames(rng, N, H, W, 'both')
        fr[0, 2, 3], fr[1, 6, 8] = np.nan, np.inf
        w, fs = rng.uniform(0.3, 3.0, N), rng.uniform(0.01, 1.0, N)
        d = dict(fr=fr, mask=mask, fmask=fmask, w=w, fs=fs)
        d['aff'] = {kind: _affines(kind, N, H, W, s) for kind, s in (('rot3', 7.0), ('half', 7.0), ('halfoff', 2.0))}
        d['rot3'] = drm.drizzle(fr, d['aff']['rot3'], 7.0, 0.5, mask=mask, frame_masks=fmask, out_shape=out_shape, fscale=fs, weights=w, conserve_flux=True)
        d['half'] = drm.drizzle(fr, d['aff']['half'], 7.0, 1.0, mask=mask, out_shape=out_shape)
        d['default_shape'] = drm.drizzle(fr, d['aff']['halfoff'], 2.0, 0.3, frame_masks=fmask)
        d['cfa'] = {c: drm.drizzle(fr, d['aff']['half'], 7.0, 0.5, frame_masks=fmask, out_shape=out_shape, cfa=(drm.COLOURS['GRBG'], c)) for c in range(3)}
        ref = rng.normal(300.0, 40.0, (2 * H, 2 * W)).astype(F)
        ref[rng.random(ref.shape) < 0.03] = np.nan
        d['ref'] = ref
        d['sig'] = rng.uniform(5.0, 20.0, N)
        d['rej'] = {kind: drm.drizzle_reject(fr, d['aff'][kind], ref, 2.0, fscale=fs + 0.8, sigmas=d['sig'], k=2.0, grow=0.5) for kind in ('rot3', 'halfoff')}
        return d
    d = io.once('data', make)
    fr, mask, fmask = io.dev(d['fr'], shift), io.dev(d['mask'], shift), io.dev(d['fmask'], shift)

    def put(tag, got, want):
        io.out(tag + '_image', got['image'], want['image'])
        io.out(tag + '_weight', got['weight'], want['weight'])
    put('rot3', ops.drizzle(fr, d['aff']['rot3'], 7.0, 0.5, mask=mask, frame_masks=fmask, out_shape=out_shape, fscale=d['fs'], weights=d['w'],
                            conserve_flux=True), d['rot3'])
    put('half', ops.drizzle(fr, d['aff']['half'], 7.0, 1.0, mask=mask, out_shape=out_shape), d['half'])
    put('default_shape', ops.drizzle(fr, d['aff']['halfoff'], 2.0, 0.3, frame_masks=fmask), d['default_shape'])
    for c in range(3):
        put('cfa_%d' % c, ops.drizzle(fr, d['aff']['half'], 7.0, 0.5, frame_masks=fmask, out_shape=out_shape, cfa=(drm.COLOURS['GRBG'], c)), d['cfa'][c])
    ref = io.dev(d['ref'], shift)
    for kind in ('rot3', 'halfoff'):
        io.out('reject_' + kind, ops.drizzle_reject(fr, d['aff'][kind], ref, 2.0, fscale=d['fs'] + 0.8, sigmas=d['sig'], k=2.0, grow=0.5), d['rej'][kind])


# ===========================================================================================================================
# the test over the table, and the coverage of the entry points (after the table, so that CASES is complete)
@pytest.mark.parametrize('name, fn, row_bytes', CASES, ids=[c[0] for c in CASES])
def test_guarded(name, fn, row_bytes, monkeypatch, side_stream):
    t0 = time.perf_counter()
    memo = {}
    default = torch.cuda.default_stream().cuda_stream
    assert torch.cuda.current_stream().cuda_stream == default
    A, sa = run(fn, row_bytes, 0xFF, memo, monkeypatch)
    assert sa and all(s == default for _, s in sa), ('run A: a call left the default stream', [c for c in sa if c[1] != default])
    for label, got, ref, tol in A:
        if ref is not None:
            compare(got, ref, tol, '%s: %s against the reference' % (name, label))
    B, _ = run(fn, row_bytes, 0x00, memo, monkeypatch)
    with torch.cuda.stream(side_stream):
        want = torch.cuda.current_stream().cuda_stream
        assert want == side_stream.cuda_stream != default
        Cr, sc = run(fn, row_bytes, 0xFF, memo, monkeypatch)
    assert [n for n, _ in sc] == [n for n, _ in sa], 'run C made other calls than run A'
    assert all(s == want for _, s in sc), ('run C: a call did not get the current stream', [c for c in sc if c[1] != want])
    for tag, other in (('B (poison 0x00)', B), ('C (side stream)', Cr)):
        assert [r[0] for r in other] == [r[0] for r in A]
        for (label, got, ref, tol), (_, first, _, _) in zip(other, A):
            what = '%s: %s, run %s' % (name, label, tag)
            if label in ORDER_DEPENDENT:
                ORDER_DEPENDENT_SEEN.add(label)
                compare(got, ref, tol, what + ' against the reference')
            else:
                compare(got, first, 'bit', what + ' against run A')
    RAN.add(name)
    TIMES[name] = time.perf_counter() - t0


def test_every_entry_point_ran_under_the_guard():
    assert RAN == {c[0] for c in CASES}, 'the coverage is that of the whole table: run the module as a whole'
    from astrophotography_amd import _lib
    assert set(EXCLUDED) <= set(_lib.SIGNATURES)
    assert ORDER_DEPENDENT_SEEN == set(ORDER_DEPENDENT), 'labels of ORDER_DEPENDENT that no case produced: %s' % sorted(set(ORDER_DEPENDENT) - ORDER_DEPENDENT_SEEN)
    missing = sorted(set(_lib.SIGNATURES) - SEEN - set(EXCLUDED))
    assert not missing, 'never called under the guard: %s' % missing
    print('guard catalogue: %d cases, %.1f s in all, slowest %s' % (len(TIMES), sum(TIMES.values()),
                                                                  sorted(TIMES.items(), key=lambda kv: -kv[1])[:3]))
