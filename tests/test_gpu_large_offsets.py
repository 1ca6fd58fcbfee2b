"""Stack, calibrate and resample kernels on cubes whose element offsets pass 2^31 or whose byte offsets pass 2^32.

Every other test of the suite stops at 2^32 bytes exactly (64 x 4096 x 4096 float32), the largest size at which a frame
offset `f * P + p` truncated to 32 bits is still harmless.  Here every kernel family that takes a [N, H, W] cube runs once on
the smallest cube that crosses the boundary and once on a cube of the same N just below it, and row bands of the result are
compared against the oracle with the assertion of the family's small-shape test (counts identical, clipped mean 1 ulp, median
0 / 1 ulp, std 2 ulp, float64 planes and the ccdproc configuration as test_gpu_redo / test_gpu_f64 / test_gpu_classes state
them, calibrate and resample bit for bit).

Data recipe: frame f is LEVEL0 + 7 f plus noise of sigma 3, so a value read from another frame cannot pass for the right one
(a wrapped read of the last frame lands in frame 0: the mean moves by ~7, the median of an even stack by 7).  The clips
(3 sigma about the median with std; 5 sigma with mad_std) leave such a column whole, so the count plane is N except at the
outliers planted in the LAST frame behind the crossing - a kernel that misses those values reports N there.
Bands: rows 0..7, the last 8 rows, the rows holding the pixel at which an offset first reaches 2^31 elements / 2^32 bytes, and
the rows of the planted outliers.  test_recipe_exposes_a_32bit_wrap (host only) replays the recipe in numpy with reads wrapped
at 2^32 bytes and asserts that the oracle then misses the tolerance on at least one compared band of every case.

Out of scope: the per-image kernels (imarith, threshold mask, demosaic, deconvolve, findstars, ...) would need ONE image of
more than 2^31 pixels, which nobody has.  The fused resample + clip takes at most 16 frames per call, so 17 x 8192 x 8192 and
68 x 4096 x 4096 are refused (asserted); its crossing cube is 16 x 8200 x 8200.
"""
import time

import numpy as np
import pytest

from tests.util import assert_biteq, assert_ulp, ulp_diff

torch = pytest.importorskip('torch')

gpu = pytest.mark.gpu

LEVEL0 = 1000.0
STEP = 7.0
NOISE = 3.0
OUTLIER = 6000.0
BAND = 8
GB = 1 << 30


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from astrophotography_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def apref():
    from oracle import apref as _a
    return _a


# ---- the recipe's geometry (host arithmetic, shared by the GPU tests and the host-only design check) -------------------------
def crossings(N, P, itemsize):
    """(frame, pixel) at which the element offset f * P + p first reaches 2^31, and the byte offset 2^32."""
    out = []
    for bound in (1 << 31, (1 << 32) // itemsize):
        f, p = divmod(bound, P)
        if f < N and (f, p) not in out:
            out.append((f, p))
    return out


def outliers(N, H, W, itemsize):
    """(frame, row, col) of the planted outliers: the last frame, behind every crossing that lies in it, and its last rows."""
    pts = [(N - 1, H - 3, 17), (N - 1, H - 6, W - 2)]
    for f, p in crossings(N, H * W, itemsize):
        if f == N - 1:
            r = p // W
            pts.append((N - 1, min(r + 1, H - 1), W // 3))
            if p + 5 < H * W:
                pts.append((N - 1, (p + 5) // W, (p + 5) % W))
    return sorted(set(pts))


def bands(N, H, W, itemsize):
    """First rows of the compared 8-row bands."""
    rows = [0, H - BAND]
    for f, p in crossings(N, H * W, itemsize):
        rows.append(p // W)
    rows += [r for _, r, _ in outliers(N, H, W, itemsize)]
    return sorted({min(max(r - 3, 0), H - BAND) for r in rows})


def below_side(N, itemsize, even=False):
    """Largest square side whose N-frame cube stays below both boundaries (even: the pair kernels need an even P)."""
    pmax = min(((1 << 31) - 1) // N, ((1 << 32) // itemsize - 1) // N)
    s = int(np.sqrt(pmax))
    while s * s > pmax or (even and s % 2):
        s -= 1
    return s


# ---- device helpers -----------------------------------------------------------------------------------------------------------
def need_memory(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + 2 * GB:
        pytest.skip('free device memory %.2f GB < cube %.2f GB + 2 GB' % (free / 1e9, nbytes / 1e9))


def make_cube(N, H, W, dtype, seed):
    """The recipe on the device; uint16 cubes are returned as torch.uint16 (values stay below 2^15)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    store = {np.uint16: torch.int16, np.float32: torch.float32, np.float64: torch.float64}[dtype]
    cube = torch.empty((N, H, W), dtype=store, device='cuda')
    for f in range(N):
        fr = torch.randn((H, W), generator=g, device='cuda') * NOISE + (LEVEL0 + STEP * f)
        cube[f] = fr.round().to(torch.int16) if dtype == np.uint16 else fr.to(store)
    for f, r, c in outliers(N, H, W, np.dtype(dtype).itemsize):
        cube[f, r, c] += int(OUTLIER) if dtype == np.uint16 else OUTLIER
    return cube.view(torch.uint16) if dtype == np.uint16 else cube


def host(t):
    t = t.contiguous()
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def run_above_and_below(name, N, side, dtype, run, check, even=False, extra_bytes=0):
    """run(cube) -> results (device tensors), once per cube; check(results, host band [N, 8, W], row slice, what) per band.
    The cube just below the boundary is compared on its last band only: a failure above it then points at the boundary."""
    itemsize = np.dtype(dtype).itemsize
    sb = below_side(N, itemsize, even)
    for tag, (H, W) in (('below', (sb, sb)), ('above', (side, side))):
        nbytes = N * H * W * itemsize
        assert (tag == 'above') == bool(crossings(N, H * W, itemsize)), (tag, N, H, W)
        need_memory(nbytes + extra_bytes)
        t0 = time.perf_counter()
        cube = make_cube(N, H, W, dtype, seed=N + H)
        res = run(cube)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rows = bands(N, H, W, itemsize) if tag == 'above' else [H - BAND]
        for r0 in rows:
            sl = slice(r0, r0 + BAND)
            check(res, host(cube[:, sl]), sl, '%s %s %d x %d x %d rows %d..' % (name, tag, N, H, W, r0))
        print('%s %s: %d x %d x %d %s = %.3f GB, crossings %s, bands %s, device %.2f s, bands %.2f s'
              % (name, tag, N, H, W, np.dtype(dtype).name, nbytes / 1e9, crossings(N, H * W, itemsize), rows, t1 - t0,
                 time.perf_counter() - t1))
        del cube, res
        torch.cuda.empty_cache()


def check_clip(apref, res, band, sl, what, **kw):
    """The assertions of test_stack_sigclip_vs_oracle / test_big_stacks_other_paths on whatever planes were asked for."""
    ref = apref.stack_sigclip(band, **kw)
    assert ref['count'].min() > 1, what                      # the clip keeps more than one value per pixel
    assert np.array_equal(host(res['count'][sl]), ref['count']), what
    assert_ulp(host(res['mean'][sl]), ref['mean'].astype(np.float32), 1, 'mean ' + what)
    if 'median' in res:
        assert_ulp(host(res['median'][sl]), ref['median'].astype(np.float32), 1, 'median ' + what)
    if 'std' in res:
        assert_ulp(host(res['std'][sl]), ref['std'].astype(np.float32), 2, 'std ' + what)
    if 'mean_f64' in res:
        np.testing.assert_allclose(host(res['mean_f64'][sl]), ref['mean'], rtol=1e-13, equal_nan=True, err_msg=what)
    if 'moments_f64' in res:
        assert np.array_equal(host(res['moments_f64']['count'][sl]), ref['count']), what
        kept = np.where(ref['keep'], band.astype(np.float64), 0.0)
        np.testing.assert_allclose(host(res['moments_f64']['sum'][sl]), kept.sum(0), rtol=1e-14, err_msg=what)      # (C3 share test)
        np.testing.assert_allclose(host(res['moments_f64']['sumsq'][sl]), (kept * kept).sum(0), rtol=1e-13, err_msg=what)


def check_ccdproc(apref, res, band, sl, what):
    """The assertions of test_ccdproc_configuration_fast_path (form 'legacy' = the library's default)."""
    ref = apref.combine_ccdproc(band.astype(np.float32) if band.dtype == np.uint16 else band, form='legacy')
    assert np.array_equal(host(res['count'][sl]), ref['count']), what
    np.testing.assert_allclose(host(res['mean_f64'][sl]), ref['mean'], rtol=4e-16, atol=0, equal_nan=True, err_msg=what)
    assert_ulp(host(res['mean'][sl]), ref['mean'].astype(np.float32), 1, what)
    np.testing.assert_allclose(host(res['std_f64'][sl]), ref['std'], rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=what)


# ---- 1, 2: fast float32 kernel, full and padded slot counts -------------------------------------------------------------------
def _fast_f32(ops, apref, name, N, side):
    print(name, 'kernel:', ops.stack_kernel_name(N, 'f32', calibrated=False, outputs=('mean', 'count')))
    run_above_and_below(name, N, side, np.float32,
                        lambda cube: ops.stack_sigclip(cube, sigma=3.0, maxiters=5, outputs=('mean', 'count')),
                        lambda res, band, sl, what: check_clip(apref, res, band, sl, what, sigma=3.0, maxiters=5))


@gpu
def test_fast_f32_full_slots(ops, apref):
    _fast_f32(ops, apref, 'case 1', 128, 2900)


@gpu
def test_fast_f32_padded_slots(ops, apref):
    _fast_f32(ops, apref, 'case 2', 100, 3300)


# ---- 3: uint16 pair kernels -----------------------------------------------------------------------------------------------------
@gpu
def test_u16_pairs_clip_and_median(ops, apref):
    N = 128
    print('case 3 kernels:', ops.stack_kernel_name(N, 'u16', calibrated=False, outputs=('mean', 'count')), '|',
          ops.stack_kernel_name(N, 'u16', calibrated=False, outputs=(), median_only=True))

    def run(cube):
        r = ops.stack_sigclip(cube, sigma=3.0, maxiters=5, outputs=('mean', 'count'))
        r['plain_median'], r['plain_count'] = ops.stack_median(cube, want_count=True)
        return r

    def check(res, band, sl, what):
        check_clip(apref, res, band, sl, what, sigma=3.0, maxiters=5)
        assert int(res['plain_count'][sl].min()) == N and int(res['plain_count'][sl].max()) == N, what
        # (test_stack_median_u16_pairs_paths: 1 ulp for an even frame count)
        assert_ulp(host(res['plain_median'][sl]), apref.stack_median(band.astype(np.float32)).astype(np.float32), 1, 'median ' + what)

    run_above_and_below('case 3', N, 4100, np.uint16, run, check, even=True)


# ---- 4, 5: chunk path, 129 .. 512 frames ------------------------------------------------------------------------------------------
def _chunks(ops, apref, name, dtype, side):
    N = 512
    dn = 'u16' if dtype == np.uint16 else 'f32'
    print(name, 'kernels:', ops.stack_kernel_name(N, dn, calibrated=False, outputs=('mean', 'count')), '|',
          ops.stack_kernel_name(N, dn, calibrated=False, outputs=('mean', 'median', 'std', 'count')))

    def run(cube):
        r = ops.stack_sigclip(cube, sigma=3.0, maxiters=5, outputs=('mean', 'median', 'std', 'count'))
        lean = ops.stack_sigclip(cube, sigma=3.0, maxiters=5, outputs=('mean', 'count'))
        r['lean_mean'], r['lean_count'] = lean['mean'], lean['count']
        return r

    def check(res, band, sl, what):
        check_clip(apref, res, band, sl, what, sigma=3.0, maxiters=5)
        check_clip(apref, dict(mean=res['lean_mean'], count=res['lean_count']), band, sl, what + ' (mean, count only)', sigma=3.0, maxiters=5)

    run_above_and_below(name, N, side, dtype, run, check, even=True)


@gpu
def test_chunk_path_f32(ops, apref):
    _chunks(ops, apref, 'case 4', np.float32, 1460)


@gpu
def test_chunk_path_u16(ops, apref):
    _chunks(ops, apref, 'case 5', np.uint16, 2050)


# ---- 6: the ccdproc configuration (median / mad_std, one strict 5-sigma pass) ----------------------------------------------------
@gpu
@pytest.mark.parametrize('N,dtype,side', [(128, np.float32, 2900), (300, np.uint16, 2700)])
def test_ccdproc_configuration(ops, apref, N, dtype, side):
    kw = dict(sigma=5.0, maxiters=1, cenfunc='median', stdfunc='mad_std')
    outs = ('mean', 'count', 'mean_f64', 'std_f64')
    print('case 6 kernel:', ops.stack_kernel_name(N, 'u16' if dtype == np.uint16 else 'f32', calibrated=False, outputs=outs,
                                                  stdfunc='mad_std', maxiters=1))
    run_above_and_below('case 6', N, side, dtype, lambda cube: ops.stack_sigclip(cube, outputs=outs, **kw),
                        lambda res, band, sl, what: check_ccdproc(apref, res, band, sl, what), even=True)


# ---- 7: fused calibrate + stack ---------------------------------------------------------------------------------------------------
def masters(H, W, N):
    """Small fixed masters (only the frame offset crosses) and per-frame exposure ratios."""
    g = torch.Generator(device='cuda').manual_seed(7 + H)
    bias = torch.randn((H, W), generator=g, device='cuda') * 2.0 + 100.0
    dark = torch.randn((H, W), generator=g, device='cuda') * 1.0 + 10.0
    nflat = torch.randn((H, W), generator=g, device='cuda') * 0.01 + 1.0
    e = 0.4 + 0.001 * np.arange(N)
    return bias, dark, nflat, e


@gpu
def test_fused_calibrate_stack(ops, apref):
    N = 128
    print('case 7 kernel:', ops.stack_kernel_name(N, 'f32', calibrated=True, outputs=('mean', 'count')))
    keep = {}

    def run(cube):
        H, W = cube.shape[1:]
        bias, dark, nflat, e = keep['m'] = masters(H, W, N)
        return ops.stack_sigclip(cube, sigma=3.0, maxiters=5, calib=dict(bias=bias, dark=dark, nflat=nflat, exp_ratio=e),
                                 outputs=('mean', 'count'))

    def check(res, band, sl, what):
        bias, dark, nflat, e = keep['m']
        # (test_fused_calibrate_stack_vs_oracle)
        ref_mean, ref_cnt = apref.calibrate_stack(band, host(bias[sl]), host(dark[sl]), host(nflat[sl]), e, sigma=3.0, maxiters=5)
        assert ref_cnt.min() > 1
        assert np.array_equal(host(res['count'][sl]), ref_cnt), what
        assert_ulp(host(res['mean'][sl]), ref_mean, 1, what)

    run_above_and_below('case 7', N, 2900, np.float32, run, check)


# ---- 8: the LDS-resident kernel of 129 .. 512 frames and the float64 moments -----------------------------------------------------
@gpu
def test_big_stack_rich_outputs_and_moments(ops, apref):
    N = 256
    outs = ('mean', 'median', 'std', 'count', 'mean_f64', 'moments_f64')
    print('case 8 kernels:', ops.stack_kernel_name(N, 'f32', calibrated=False, outputs=outs), '|',
          ops.stack_kernel_name(N, 'f32', calibrated=False, outputs=(), median_only=True))

    def run(cube):
        r = ops.stack_sigclip(cube, sigma=3.0, maxiters=5, outputs=outs)
        r['plain_median'] = ops.stack_median(cube)
        ch = ops.stack_sigclip_chunked(cube, chunk=128, sigma=3.0, maxiters=5)            # hierarchical moments: 2 x 128 frames
        r['chunk_mean'], r['chunk_count'] = ch['mean'], ch['count']
        return r

    def check(res, band, sl, what):
        check_clip(apref, res, band, sl, what, sigma=3.0, maxiters=5)
        assert_ulp(host(res['plain_median'][sl]), apref.stack_median(band).astype(np.float32), 1, 'plain median ' + what)
        tot, cnt = np.zeros(band.shape[1:]), np.zeros(band.shape[1:], np.int64)           # (test_c3_share_full_size_moments (4))
        for lo in (0, 128):
            rr = apref.stack_sigclip(band[lo:lo + 128], sigma=3.0, maxiters=5, want=('keep', 'count'))
            tot += np.where(rr['keep'], band[lo:lo + 128].astype(np.float64), 0.0).sum(0)
            cnt += rr['count']
        assert np.array_equal(host(res['chunk_count'][sl]), cnt), what
        assert_ulp(host(res['chunk_mean'][sl]), (tot / cnt).astype(np.float32), 1, 'chunked ' + what)

    run_above_and_below('case 8', N, 2100, np.float32, run, check, even=True)


# ---- 9: float64 frames ------------------------------------------------------------------------------------------------------------
@gpu
def test_float64_cube_combine(ops, apref):
    N, side = 40, 3700

    def check(res, band, sl, what):
        ref = apref.combine_ccdproc(band, 5.0, 5.0)                                      # (test_gpu_classes: bit for bit)
        assert ref['count'].min() > 1
        assert np.array_equal(host(res['count'][sl]), ref['count']), what
        assert_biteq(host(res['mean_f64'][sl]), ref['mean'], 'mean ' + what)
        assert_biteq(host(res['std_f64'][sl]), ref['std'], 'std ' + what)

    # (the entry allocates a workspace of two more cubes)
    run_above_and_below('case 9', N, side, np.float64, lambda cube: ops.combine_f64(cube), check)


# ---- 10: slab calibrate --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('N,side', [(65, 4096), (129, 4100)])
def test_slab_calibrate(ops, apref, N, side):
    """65 x 4096 x 4096 uint16: the float32 OUTPUT passes 2^32 bytes (the input stays below 2^31 elements); 129 x 4100 x 4100:
    the input passes 2^31 elements too.  The output starts as NaN, so a store that lands elsewhere leaves a mark."""
    keep = {}

    def run(cube):
        H, W = cube.shape[1:]
        bias, dark, nflat, e = keep['m'] = masters(H, W, N)
        out = torch.full(cube.shape, float('nan'), dtype=torch.float32, device='cuda')
        ops.calibrate(cube, bias, dark, nflat, e, out=out)
        return dict(out=out)

    def check(res, band, sl, what):
        bias, dark, nflat, e = keep['m']
        assert_biteq(host(res['out'][:, sl]), apref.calibrate(band, host(bias[sl]), host(dark[sl]), host(nflat[sl]), e), what)

    itemsize = 2
    # the boundary of this case is the OUTPUT's (4 bytes per value): the cube "below" keeps N * P * 4 under 2^32
    sb = below_side(N, 4)
    for tag, (H, W) in (('below', (sb, sb)), ('above', (side, side))):
        need_memory(N * H * W * (itemsize + 4))
        t0 = time.perf_counter()
        cube = make_cube(N, H, W, np.uint16, seed=N + H)
        res = run(cube)
        torch.cuda.synchronize()
        rows = sorted(set(bands(N, H, W, 4) + bands(N, H, W, 2))) if tag == 'above' else [H - BAND]
        for r0 in rows:
            sl = slice(r0, r0 + BAND)
            check(res, host(cube[:, sl]), sl, 'case 10 %s %d x %d x %d rows %d..' % (tag, N, H, W, r0))
        print('case 10 %s: %d x %d x %d, output crossings %s, input crossings %s, bands %s, %.2f s'
              % (tag, N, H, W, crossings(N, H * W, 4), crossings(N, H * W, 2), rows, time.perf_counter() - t0))
        del cube, res
        torch.cuda.empty_cache()


# ---- 11: resample, clipped co-add of the resampled slab, fused resample + clip ------------------------------------------------------
def dither(N, seed=5):
    """The dithered transforms of test_c5_share_full_size_resample_clip: rotations below 0.2 degrees, shifts below 3 pixels."""
    rng = np.random.default_rng(seed)
    th = np.deg2rad(rng.uniform(-0.2, 0.2, N))
    A = np.stack([np.cos(th), -np.sin(th), rng.uniform(-3, 3, N), np.sin(th), np.cos(th), rng.uniform(-3, 3, N)], 1)
    A[0] = [1, 0, 0, 0, 1, 0]
    A[1] = [1, 0, 2, 0, 1, -1]
    return A


def resample_frames(N, H, W, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    frames = torch.empty((N, H, W), dtype=torch.float32, device='cuda')
    for f in range(N):
        frames[f] = torch.randn((H, W), generator=g, device='cuda') * NOISE + (LEVEL0 + STEP * f)
    frames[N - 1, 4, W // 3] += OUTLIER                        # behind the crossing (the last frame starts at 2^32 bytes or just before)
    frames[N - 1, H - 3, 17] += OUTLIER
    mask = (torch.rand((H, W), generator=g, device='cuda') < 2e-4).to(torch.uint8)
    return frames, mask


def check_resampled(apref, res, wt, frames, mask, A, f, r0, rows, what):
    """Output rows r0 .. r0 + rows of frame f, bit for bit (the oracle computes the rows 0 .. r0 + rows with the SAME transform and
    reads the whole input frame, as in the C5 test)."""
    W = frames.shape[2]
    ref, wref = apref.resample_affine(host(frames[f]), [A[f]], mask=host(mask), out_shape=(r0 + rows, W))
    assert_biteq(host(res[f, r0:r0 + rows]), ref[0][r0:], what)
    assert np.array_equal(host(wt[f, r0:r0 + rows]), wref[0][r0:]), what


@gpu
def test_slab_resample_and_coadd(ops, apref):
    N = 17
    sb = below_side(N, 4)
    for tag, (H, W) in (('below', (sb, sb)), ('above', (8192, 8192))):
        need_memory(N * H * W * 4)
        assert (tag == 'above') == bool(crossings(N, H * W, 4))
        t0 = time.perf_counter()
        frames, mask = resample_frames(N, H, W, seed=H)
        A = dither(N)
        res, wt = ops.resample_affine(frames, A, mask=mask)
        st = ops.stack_sigclip(res, sigma=3.0, maxiters=5, outputs=('mean', 'count'))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        # the last frame's contribution itself: its last rows; above the boundary also its first rows (where the byte offset
        # reaches 2^32) and the last rows of the frame in front of it
        check_resampled(apref, res, wt, frames, mask, A, N - 1, H - 16, 16, 'case 11 %s last frame, last rows' % tag)
        rows = [H - BAND]
        if tag == 'above':
            check_resampled(apref, res, wt, frames, mask, A, N - 1, 0, 16, 'case 11 last frame, first rows')
            check_resampled(apref, res, wt, frames, mask, A, 2, 0, 16, 'case 11 frame 2, first rows')
            rows = [0, 4090, H - BAND]
        # the clipped co-add of the slab (N = 17 columns over the same offsets): dropping or swapping the last frame moves the
        # mean by ~ 7 * 16 / 17 and the count by one
        for r0 in rows:
            sl = slice(r0, r0 + BAND)
            ref = apref.stack_sigclip(host(res[:, sl]), sigma=3.0, maxiters=5)
            assert np.array_equal(host(st['count'][sl]), ref['count']), (tag, r0)
            assert_ulp(host(st['mean'][sl]), ref['mean'].astype(np.float32), 1, 'case 11 %s co-add rows %d..' % (tag, r0))
        assert int(st['count'][8:-8, 8:-8].max()) == N
        print('case 11 %s: %d x %d x %d, crossings %s, device %.2f s, oracle %.2f s'
              % (tag, N, H, W, crossings(N, H * W, 4), t1 - t0, time.perf_counter() - t1))
        del frames, mask, res, wt, st
        torch.cuda.empty_cache()


@gpu
def test_fused_resample_clip(ops, apref):
    """The fused kernel takes at most 16 frames per call: the issue's 17- and 68-frame cubes are refused, and the smallest cube
    it accepts that passes 2^32 bytes is 16 x 8200 x 8200.  Reference: resample_affine + the oracle's clip on row bands (the
    two-step form, as in the C5 test: same survivors, mean within 1 ulp of the oracle)."""
    for n, h in ((17, 64), (68, 64)):
        with pytest.raises(Exception, match='16'):
            ops.resample_stack_sigclip(torch.zeros((n, h, 64), device='cuda'), dither(n))
    N = 16
    sb = below_side(N, 4)
    for tag, (H, W) in (('below', (sb, sb)), ('above', (8200, 8200))):
        need_memory(N * H * W * 4)
        assert (tag == 'above') == bool(crossings(N, H * W, 4))
        t0 = time.perf_counter()
        frames, mask = resample_frames(N, H, W, seed=H)
        A = dither(N)
        fu = ops.resample_stack_sigclip(frames, A, mask=mask, sigma=3.0, maxiters=5, outputs=('mean', 'count'))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        # the reference's resampled values come frame by frame (one 8200 x 8200 image per call: no offset near the boundary)
        per_frame = [ops.resample_affine(frames[f], A[f:f + 1], mask=mask, weight=False)[0][0] for f in range(N)]
        p = crossings(N, H * W, 4)[0][1] if tag == 'above' else 0
        rows = sorted({0, min(max(p // W - 3, 0), H - BAND), H - BAND}) if tag == 'above' else [H - BAND]
        for r0 in rows:
            sl = slice(r0, r0 + BAND)
            ref = apref.stack_sigclip(np.stack([host(r[sl]) for r in per_frame]), sigma=3.0, maxiters=5)
            assert np.array_equal(host(fu['count'][sl]), ref['count']), (tag, r0)
            assert_ulp(host(fu['mean'][sl]), ref['mean'].astype(np.float32), 1, 'case 11 fused %s rows %d..' % (tag, r0))
        assert int(fu['count'][8:-8, 8:-8].max()) == N
        print('case 11 fused %s: %d x %d x %d, crossings %s, bands %s, device %.2f s' % (tag, N, H, W, crossings(N, H * W, 4), rows, t1 - t0))
        del frames, mask, per_frame, fu
        torch.cuda.empty_cache()


# ---- the design check: host only --------------------------------------------------------------------------------------------------
def synthetic_band(N, H, W, dtype, r0, wrap):
    """The recipe as a map from flat index to value, on rows r0 .. r0 + 8: value(i) = level of frame i // P + noise(i) + outlier;
    wrap: frame f's pixel p is read from flat index (f P + p) mod (2^32 / itemsize) - what a 32-bit byte offset does."""
    itemsize = np.dtype(dtype).itemsize
    P = H * W
    f = np.arange(N, dtype=np.int64)[:, None]
    p = (np.arange(r0 * W, (r0 + BAND) * W, dtype=np.int64))[None, :]
    i = f * P + p
    if wrap:
        i = i % ((1 << 32) // itemsize)
    h = ((i % 2147483629) * 48271 + (i >> 17)) % 65521
    noise = (h / 65521.0 - 0.5) * np.sqrt(12.0) * NOISE                                  # uniform, sigma 3
    v = LEVEL0 + STEP * (i // P) + noise
    for fo, r, c in outliers(N, H, W, itemsize):
        v[i == fo * P + r * W + c] += OUTLIER
    v = np.rint(v).astype(np.uint16) if dtype == np.uint16 else v.astype(dtype)
    return v.reshape(N, BAND, W)


def _missed(got, ref, tol):
    """Would the band's assertion fail?  counts identical, float32 planes within tol ulp."""
    if not np.array_equal(got['count'], ref['count']):
        return True
    return bool(ulp_diff(np.float32(got['mean']), np.float32(ref['mean'])).max() > tol)


HOST_CASES = [('1', 128, 2900, np.float32, 'clip'), ('2', 100, 3300, np.float32, 'clip'), ('3', 128, 4100, np.uint16, 'clip'),
              ('3 median', 128, 4100, np.uint16, 'median'), ('4', 512, 1460, np.float32, 'clip'), ('5', 512, 2050, np.uint16, 'clip'),
              ('6 f32', 128, 2900, np.float32, 'ccdproc'), ('6 u16', 300, 2700, np.uint16, 'ccdproc'), ('7', 128, 2900, np.float32, 'calib'),
              ('8', 256, 2100, np.float32, 'clip'), ('9', 40, 3700, np.float64, 'ccdproc'), ('10 in', 129, 4100, np.uint16, 'calibrate')]


@pytest.mark.parametrize('name,N,side,dtype,kind', HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_recipe_exposes_a_32bit_wrap(apref, name, N, side, dtype, kind):
    """No kernel involved: with reads wrapped at 2^32 bytes the oracle's planes miss the tolerance of the case on at least one
    of the compared bands, and the clip rejects the planted outliers (count N - 1 there, N elsewhere)."""
    itemsize = np.dtype(dtype).itemsize
    H = W = side

    def planes(b, r0):
        if kind == 'clip':
            return apref.stack_sigclip(b, sigma=3.0, maxiters=5, want=('mean', 'count')), 1
        if kind == 'median':
            return dict(mean=apref.stack_median(b.astype(np.float32)), count=np.zeros(1)), 1
        if kind == 'ccdproc':
            r = apref.combine_ccdproc(b.astype(np.float32) if dtype == np.uint16 else b, form='legacy' if dtype != np.float64 else 'astropy')
            return r, (1 if dtype != np.float64 else 0)
        rng = np.random.default_rng(r0)
        bias, dark = rng.normal(100, 2, (BAND, W)).astype(np.float32), rng.normal(10, 1, (BAND, W)).astype(np.float32)
        nflat, e = rng.normal(1, 0.01, (BAND, W)).astype(np.float32), 0.4 + 0.001 * np.arange(N)
        if kind == 'calib':
            m, c = apref.calibrate_stack(b, bias, dark, nflat, e, sigma=3.0, maxiters=5)
            return dict(mean=m, count=c), 1
        out = apref.calibrate(b, bias, dark, nflat, e)                                    # bit for bit: tol 0 on every value
        return dict(mean=out, count=np.zeros(1)), 0

    assert crossings(N, H * W, itemsize)
    hit = []
    for r0 in bands(N, H, W, itemsize):
        true, tol = planes(synthetic_band(N, H, W, dtype, r0, wrap=False), r0)
        if 'count' in true and kind != 'median' and kind != 'calibrate':
            assert true['count'].min() > 1                                                # the clip keeps more than one value per pixel
        wrapped, _ = planes(synthetic_band(N, H, W, dtype, r0, wrap=True), r0)
        if _missed(wrapped, true, tol):
            hit.append(r0)
    assert hit, 'case %s: a 32-bit wrap passes every compared band' % name
    # the outliers are rejected by the clip: a kernel that misses them gets the count wrong
    if kind in ('clip', 'ccdproc', 'calib'):
        f, r, c = outliers(N, H, W, itemsize)[0]
        r0 = min(max(r - 3, 0), H - BAND)
        true, _ = planes(synthetic_band(N, H, W, dtype, r0, wrap=False), r0)
        assert true['count'][r - r0, c] == N - 1 and np.median(true['count']) == N


def test_recipe_exposes_a_wrapped_store_and_frame_base(apref):
    """Case 10 (65 x 4096 x 4096): the input does not wrap, the float32 output does - a store at (f P + p) mod 2^30 leaves the
    last frame's band unwritten (NaN).  Case 11: a frame base wrapped at 2^32 bytes makes frame 16 of 17 x 8192 x 8192 read
    frame 0 (and byte 2^32 of 16 x 8200 x 8200 lies in its last frame): the resampled values differ in every bit-for-bit band and
    the clipped mean of the 17 values moves by more than an ulp."""
    N, H, W = 65, 4096, 4096
    (f, p), = crossings(N, H * W, 4)
    assert not crossings(N, H * W, 2) and f == N - 1 and any(r0 <= p // W < r0 + BAND for r0 in bands(N, H, W, 4))
    assert (H - BAND) * W >= p                               # the last band of the last frame lies behind the crossing: never stored
    N, H, W = 17, 8192, 8192
    assert crossings(N, H * W, 4) == [(16, 0)] and crossings(16, 8200 * 8200, 4)[0][0] == 15
    rng = np.random.default_rng(3)
    fr = [(rng.normal(0, NOISE, (48, 256)) + LEVEL0 + STEP * f).astype(np.float32) for f in (0, N - 1)]
    A = dither(N)[N - 1]
    a, _ = apref.resample_affine(fr[1], [A], out_shape=(32, 256))
    b, _ = apref.resample_affine(fr[0], [A], out_shape=(32, 256))
    ok = ~np.isnan(a) & ~np.isnan(b)
    assert ok.any() and (a[ok] != b[ok]).all()
    col = (LEVEL0 + STEP * np.arange(N)[:, None] + rng.normal(0, NOISE, (N, 64))).astype(np.float32)
    true = apref.stack_sigclip(col, sigma=3.0, maxiters=5, want=('mean', 'count'))
    col[N - 1] = col[0]
    wrapped = apref.stack_sigclip(col, sigma=3.0, maxiters=5, want=('mean', 'count'))
    assert true['count'].min() > 1 and _missed(wrapped, true, 1)
