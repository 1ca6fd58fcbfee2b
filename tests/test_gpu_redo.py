"""The stack's two-kernel scheme (fast kernel + redo pass) at its edges: the caller's workspace (apgpu_stack_args.workspace:
size, zero prefix kept zero, statistics, too small -> APGPU_EWORKSPACE, none at all -> temporary), the guard against stacks
whose pixels mostly fail the fast path (64-pixel blocks given up, reduced whole by the redo pass; the mode word), uint16 pair stacks whose frames do
not share one exposure ratio, and APGPU_STACK_SINGLE_KERNEL - every route against the CPU oracle (identical survivor
counts, means within 1 ulp)."""
import ctypes as C

import numpy as np
import pytest

from tests.util import assert_ulp, synth_masters

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


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


def dev(a, ops):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return ops.to_device_u16(a)
    return torch.from_numpy(a).cuda()


def _raw_frames(rng, N, shape, bias, dark, nf, e, dtype):
    sky = rng.normal(400, 15, (N,) + shape)
    hits = rng.random(sky.shape) < 0.01
    sky[hits] += rng.uniform(200, 4000, hits.sum())
    raw = bias + e * dark + nf * sky
    if dtype == np.uint16:
        return np.clip(np.rint(raw), 0, 65535).astype(np.uint16)
    return raw.astype(np.float32)


def _zero_prefix_is_zero(ops, ws, P):
    from astrophotography_amd import _lib
    zero = C.c_size_t(0)
    _lib.load().apgpu_stack_ws_bytes(P, C.byref(zero))
    pre = ws.view(torch.int32)[:zero.value // 4].clone()
    o = _lib.STACK_WS_STATS_OFFSET // 4
    pre[o:o + 8] = 0                                         # the statistics are cumulative by design,
    pre[o + 16 + 3] = 0                                      # and the mode words are the workspace's memory of the last call
    pre[o + 16 + 10] = 0                                     # (the median / mad_std pair's)
    return int(pre.abs().max().item()) == 0


@pytest.mark.parametrize('dtype', [np.float32, np.uint16])
def test_guard_against_mostly_failing_stacks(ops, apref, dtype):
    """2048 x 2048 (16384 tiles: 64 workgroups per segment - 32 for the pair kernels - so the guard can trip after a segment's first
    12), 16 frames, fused calibration.  A chosen share
    of the columns is forced off the fast path two ways - a NaN in the flat (the whole column is non-finite) and five staggered
    outliers that five passes peel off one by one (a fifth value to trim).  At 0.5 % the pixels go through the lists, at 60 % and
    100 % the segments give their tiles up; every route must reproduce the oracle, leave the workspace's prefix zero and count
    what it did."""
    rng = np.random.default_rng(91)
    H, W, N = 2048, 2048, 16
    e = 0.4
    bias, dark, flat = synth_masters(rng, (H, W))
    nf0 = (flat / np.float32(flat.mean())).astype(np.float32)
    base = _raw_frames(rng, N, (H, W), bias, dark, nf0, e, dtype)
    for share in (0.005, 0.6, 1.0):
        sel = rng.random((H, W)) < share
        how = rng.random((H, W)) < 0.5
        nf = nf0.copy()
        nf[sel & how] = np.nan
        raw = base.copy()
        stag = sel & ~how
        for k, amp in enumerate((300.0, 3000.0, 30000.0) if dtype == np.uint16 else (3e2, 3e3, 3e4, 3e5, 3e6)):
            raw[3 * k + 1][stag] = (raw[3 * k + 1][stag].astype(np.float64) + amp).clip(0, 65535 if dtype == np.uint16 else 1e30).astype(dtype)
        calib = dict(bias=dev(bias, ops), dark=dev(dark, ops), nflat=dev(nf, ops), exp_ratio=e)
        d = dev(raw, ops)
        with np.errstate(all='ignore'):
            mean_ref, cnt_ref = apref.calibrate_stack(raw, bias, dark, nf, e, sigma=3.0, maxiters=5)
        what = f'{np.dtype(dtype).name} share={share}'
        # the FIRST call on data that has just turned bad still runs in the mode the last call left (quiet after the 0.5 % case:
        # no guard, every failing pixel listed); it must be right all the same, and it arms the guard for the second
        for attempt in (0, 1):
            ops.stack_redo_stats(reset=True)
            r = ops.stack_sigclip(d, sigma=3.0, maxiters=5, calib=calib, outputs=('mean', 'count'))
            st = ops.stack_redo_stats()
            assert np.array_equal(r['count'].cpu().numpy(), cnt_ref), (what, attempt)
            assert_ulp(r['mean'].cpu().numpy(), mean_ref, 1, what)
            assert st['calls'] == 1 and st['pixels'] == H * W, st
            assert st['fraction'] >= 0.45 * share, (what, st)              # (half of the selected columns are all-NaN for sure)
        # what really fails: every selected column for float32; for uint16 only the NaN-flat half (three staggered outliers fit
        # the fast path's tails).  The guard tips at 40 %: clearly above -> the segments give their blocks up after the first
        # 32 finished blocks each; clearly below -> everything goes through the lists; in between either route is right.
        failing = share if dtype == np.float32 else share / 2
        if failing >= 0.5:
            assert st['blocks_given_up'] > 4 * 6000, (what, st)
        elif failing <= 0.3:
            assert st['blocks_given_up'] == 0 and st['pixels_listed'] >= sel.sum() // 2, (what, st)
        assert _zero_prefix_is_zero(ops, ops.stack_workspace(H * W, d.device), H * W), what
        # the same stack in ONE kernel, and without a caller's workspace: same survivors, same 1 ulp
        for kw in (dict(single_kernel=True), dict(workspace=False)):
            r2 = ops.stack_sigclip(d, sigma=3.0, maxiters=5, calib=calib, outputs=('mean', 'count'), **kw)
            assert np.array_equal(r2['count'].cpu().numpy(), cnt_ref), (what, kw)
            assert_ulp(r2['mean'].cpu().numpy(), mean_ref, 1, what + str(kw))


def test_uint16_pairs_with_per_frame_exposure_ratios(ops, apref):
    """The pair kernels need one exposure ratio for all frames; the host cannot see the ratios (a device array), so the fast
    pair kernel tests them itself and gives every tile up - the redo pass then reduces the stack with the one-pixel-per-lane
    body, float32 fast path included (this used to send every pixel through the list and the float64 clip)."""
    rng = np.random.default_rng(92)
    H, W, N = 96, 512, 32
    bias, dark, flat = synth_masters(rng, (H, W))
    nf = (flat / np.float32(flat.mean())).astype(np.float32)
    e = (0.4 + 0.01 * np.arange(N)).astype(np.float32)
    raw = _raw_frames(rng, N, (H, W), bias, dark, nf, e[:, None, None], np.uint16)
    calib = dict(bias=dev(bias, ops), dark=dev(dark, ops), nflat=dev(nf, ops), exp_ratio=[float(x) for x in e])
    mean_ref, cnt_ref = apref.calibrate_stack(raw, bias, dark, nf, [float(x) for x in e], sigma=3.0, maxiters=5)
    ops.stack_redo_stats(reset=True)
    r = ops.stack_sigclip(dev(raw, ops), sigma=3.0, maxiters=5, calib=calib, outputs=('mean', 'count'))
    st = ops.stack_redo_stats()
    assert np.array_equal(r['count'].cpu().numpy(), cnt_ref)
    assert_ulp(r['mean'].cpu().numpy(), mean_ref, 1, 'per-frame ratios')
    assert st['blocks_given_up'] == H * W // 64 and st['pixels_listed'] == 0, st
    assert ops.stack_kernel_name(N, 'u16', calibrated=True).startswith('stack_fast_u16_pairs_kernel<32')


def test_workspace_contract(ops, apref):
    from astrophotography_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(93)
    H, W, N = 64, 301, 24                                    # 19264 pixels: 75 tiles + a partial one of 64
    bias, dark, flat = synth_masters(rng, (H, W))
    nf = (flat / np.float32(flat.mean())).astype(np.float32)
    raw = _raw_frames(rng, N, (H, W), bias, dark, nf, 0.4, np.float32)
    raw[:, 5, 7] = np.nan
    calib = dict(bias=dev(bias, ops), dark=dev(dark, ops), nflat=dev(nf, ops), exp_ratio=0.4)
    d = dev(raw, ops)
    with np.errstate(all='ignore'):
        mean_ref, cnt_ref = apref.calibrate_stack(raw, bias, dark, nf, 0.4, sigma=3.0, maxiters=5)
    zero = C.c_size_t(0)
    need = lib.apgpu_stack_ws_bytes(H * W, C.byref(zero))
    # a caller's own workspace, zeroed once, used for several calls
    ws = torch.full((need // 4 + 3,), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
    ws[:zero.value // 4] = 0
    for k in range(3):
        r = ops.stack_sigclip(d, sigma=3.0, maxiters=5, calib=calib, outputs=('mean', 'count'), workspace=ws)
        assert np.array_equal(r['count'].cpu().numpy(), cnt_ref)
        assert_ulp(r['mean'].cpu().numpy(), mean_ref, 1, 'own workspace, call %d' % k)
        assert _zero_prefix_is_zero(ops, ws, H * W)
    o = _lib.STACK_WS_STATS_OFFSET // 4
    calls, pixels, listed, blocks = ws[o:o + 8].view(torch.int64)[:4].tolist()
    assert calls == 3 and pixels == 3 * H * W and blocks == 0 and listed >= 3 * (H * W % 256 + 1)   # the partial tile + the NaN column
    assert int(ws[need // 4:].min()) == 0x5a5a5a5a            # nothing written behind the advertised size
    # too small, misaligned
    with pytest.raises(_lib.ApGpuError) as ei:
        ops.stack_sigclip(d, sigma=3.0, maxiters=5, calib=calib, workspace=ws[:need // 4 - 4])
    assert ei.value.code == _lib.E_WORKSPACE
    with pytest.raises(_lib.ApGpuError) as ei:
        ops.stack_sigclip(d, sigma=3.0, maxiters=5, calib=calib, workspace=ws[1:])
    assert ei.value.code == _lib.E_INVAL
    # chunked kernel (129 .. 512 frames): its redo list lives in the same workspace
    raw2 = _raw_frames(rng, 160, (H, W), bias, dark, nf, 0.4, np.float32)
    calib2 = dict(calib, exp_ratio=0.4)
    m2, c2 = apref.calibrate_stack(raw2, bias, dark, nf, 0.4, sigma=3.0, maxiters=5)
    before = ws[o:o + 8].view(torch.int64)[0].item()
    r = ops.stack_sigclip(dev(raw2, ops), sigma=3.0, maxiters=5, calib=calib2, outputs=('mean', 'count'), workspace=ws)
    assert np.array_equal(r['count'].cpu().numpy(), c2)
    assert_ulp(r['mean'].cpu().numpy(), m2, 1, '160 frames, chunked kernel')
    assert ws[o:o + 8].view(torch.int64)[0].item() == before + 1 and _zero_prefix_is_zero(ops, ws, H * W)


@pytest.mark.parametrize('N,dtype', [(257, np.float32), (320, np.uint16), (384, np.float32), (385, np.uint16), (448, np.float32), (470, np.float32), (512, np.float32),
                                     (512, np.uint16), (300, np.uint16), (420, np.uint16)])
def test_chunked_pairs_257_to_512_frames(ops, apref, N, dtype):
    """257 .. 512 frames on the chunked kernel (round 5: pairs of chunks, tails of 16): fused calibration, a sky level that drifts
    in acquisition order, 1 % outliers per frame (five per column on average: some columns use the tails up), a dead column,
    a NaN in the flat, per-frame exposure ratios - against the oracle; and the fast pass must really carry the stack (the
    exact kernel redoes a small share), with its list in the caller's workspace."""
    rng = np.random.default_rng(600 + N)
    H, W = 24, 512
    bias, dark, flat = synth_masters(rng, (H, W))
    nf = (flat / np.float32(flat.mean())).astype(np.float32)
    nf[3, 5] = np.nan
    e = (0.4 + 0.0005 * np.arange(N)).astype(np.float32)
    sky = rng.normal(400, 15, (N, H, W)) + np.linspace(0.0, 60.0, N)[:, None, None]       # four sigma of drift over the sequence
    hits = rng.random(sky.shape) < 0.01
    sky[hits] += rng.uniform(200, 4000, hits.sum())
    sky[:, 7, 9] = 123.0
    raw = bias + e[:, None, None] * dark + np.where(np.isnan(nf), 1.0, nf) * sky
    raw = np.clip(np.rint(raw), 0, 65535).astype(np.uint16) if dtype == np.uint16 else raw.astype(np.float32)
    el = [float(x) for x in e]
    with np.errstate(all='ignore'):
        mean_ref, cnt_ref = apref.calibrate_stack(raw, bias, dark, nf, el, sigma=3.0, maxiters=5)
    calib = dict(bias=dev(bias, ops), dark=dev(dark, ops), nflat=dev(nf, ops), exp_ratio=el)
    name = ops.stack_kernel_name(N, 'u16' if dtype == np.uint16 else 'f32', calibrated=True)
    K = -(-N // 64)                                          # chunks; KS windows, the first K - KS of them pairs (5 = 4 + 1 and 7 = 4 + 3: round 6)
    KS = 3 if K in (3, 6) else 4
    assert name.startswith('stack_chunks_kernel<%d, %d,' % (KS, K - KS)), name
    d = dev(raw, ops)
    ops.stack_redo_stats(reset=True)
    r = ops.stack_sigclip(d, sigma=3.0, maxiters=5, calib=calib, outputs=('mean', 'count'))
    st = ops.stack_redo_stats()
    assert np.array_equal(r['count'].cpu().numpy(), cnt_ref), N
    assert_ulp(r['mean'].cpu().numpy(), mean_ref, 1, '%d frames, chunked pairs' % N)
    assert st['calls'] == 1 and 0 < st['pixels_listed'] < 0.25 * H * W, st
    x = ops.stack_sigclip(d, sigma=3.0, maxiters=5, calib=calib, outputs=('mean', 'count'), exact=True)
    assert np.array_equal(x['count'].cpu().numpy(), cnt_ref), N
    assert_ulp(x['mean'].cpu().numpy(), mean_ref, 1, '%d frames, exact kernel' % N)
    assert _zero_prefix_is_zero(ops, ops.stack_workspace(H * W, d.device), H * W)


@pytest.mark.parametrize('N,dtype', [(3, np.float32), (4, np.uint16), (5, np.uint16), (10, np.float32), (16, np.uint16), (25, np.float32),
                                     (32, np.uint16), (33, np.uint16), (47, np.float32), (63, np.uint16), (64, np.float32), (64, np.uint16),
                                     (65, np.float32), (96, np.uint16), (101, np.float32), (127, np.uint16), (128, np.float32), (128, np.uint16)])
def test_ccdproc_configuration_fast_path(ops, apref, N, dtype):
    """A6 on the register-resident fast kernel (stack_mad.hip, round 5): one pass of median / mad_std with 5-sigma bounds on
    stacks of 3 .. 128 frames (odd and even counts), float64 mean / std + count, against the oracle's restatement of ccdproc.combine.  Columns built for its edges:
    plain noise, 1 % outliers, columns with 3 .. 12 outliers on one side (more than the tails of 8 hold), low-noise integer data
    (ties; more than half of the values equal: MAD = 0), values planted next to the bound, NaN / inf (float32), and a pixel count
    that leaves a partial last block.  Unsure blocks go to the rich kernel: the results must equal the oracle either way, the
    workspace's flags must be clear afterwards, and the fast kernel must carry most of the blocks."""
    rng = np.random.default_rng(700 + N + (1 if dtype == np.uint16 else 0))
    # 15949 pixels: 62 full tiles + a partial one (odd: one pixel per lane); uint16 stacks also with an even
    # pixel count - two pixels per lane on the packed network (stack_mad_pairs.hip), 30 full 512-pixel tiles + a partial one
    for H, W in ((41, 389),) + (((40, 390),) if dtype == np.uint16 else ()):
        _ccdproc_fast_case(ops, apref, N, dtype, H, W)


def _ccdproc_fast_case(ops, apref, N, dtype, H, W):
    rng = np.random.default_rng(700 + N + (1 if dtype == np.uint16 else 0) + W)
    cube = rng.normal(1000.0, 12.0, (N, H, W))
    hits = rng.random(cube.shape) < 0.01
    cube[hits] += rng.uniform(100, 5000, hits.sum())
    for k in range(3, 13):                                   # columns with k outliers on one side
        sgn = 1.0 if k % 2 else -0.4
        cube[:max(min(k, N - 2), 1), 2, k] += sgn * 2000.0
    cube[:, 3, :] = np.rint(rng.normal(500.0, 0.6, (N, W)))  # a few distinct integer values: ties, often MAD = 0
    cube[:, 4, :] = 777.0                                     # constant columns
    cube[:, 5, :] = np.rint(rng.normal(300.0, 2.0, (N, W)))
    # a value next to the upper bound: base + 5 * 1.4826 * MAD (+- a few ulp) computed from the column as it stands
    for x in range(0, W, 3):
        col = np.sort(cube[1:, 6, x].astype(np.float32).astype(np.float64))
        base = np.median(col)
        mad = np.median(np.abs(col - base))
        cube[0, 6, x] = base + 5 * 1.482602218505602 * mad * (1 + rng.integers(-3, 4) * 2.0 ** -23)
    if dtype == np.uint16:
        cube = np.clip(np.rint(cube), 0, 65535).astype(np.uint16)
    else:
        cube = cube.astype(np.float32)
        cube[1, 7, 10:40] = np.nan
        cube[2, 7, 50] = np.inf
        cube[:, 7, 60] = np.nan
    d = dev(cube, ops)
    what0 = '%d frames %s' % (N, np.dtype(dtype).name)
    # both published forms of Combiner.sigma_clipping (golden group G12): 'legacy' masks non-finite values and clips the rest,
    # 'astropy' (APGPU_STACK_NONFINITE_UNCLIPPED) leaves a column that holds one unclipped
    for form, flag in (('legacy', False), ('astropy', True)):
        what = what0 + ' ' + form
        ref = apref.combine_ccdproc(cube.astype(np.float32) if dtype == np.uint16 else cube, form=form)
        ops.stack_redo_stats(reset=True)
        r = ops.stack_sigclip(d, sigma=5.0, maxiters=1, cenfunc='median', stdfunc='mad_std', outputs=('mean', 'count', 'mean_f64', 'std_f64'),
                              nonfinite_unclipped=flag)
        st = ops.stack_redo_stats()
        assert np.array_equal(r['count'].cpu().numpy(), ref['count']), what
        np.testing.assert_allclose(r['mean_f64'].cpu().numpy(), ref['mean'], rtol=4e-16, atol=0, equal_nan=True, err_msg=what)
        assert_ulp(r['mean'].cpu().numpy(), ref['mean'].astype(np.float32), 1, what)
        np.testing.assert_allclose(r['std_f64'].cpu().numpy(), ref['std'], rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=what)
        nblocks = (H * W + 63) // 64
        assert st['calls'] == 1 and st['pixels'] == H * W and 0 < st['blocks_given_up'] < (0.5 if N >= 8 else 0.9) * nblocks, (what, st)
        assert _zero_prefix_is_zero(ops, ops.stack_workspace(H * W, d.device), H * W), what
        # the same call on the rich kernel alone, and without a workspace: same numbers
        for kw in (dict(single_kernel=True), dict(workspace=False)):
            r2 = ops.stack_sigclip(d, sigma=5.0, maxiters=1, cenfunc='median', stdfunc='mad_std', outputs=('mean_f64', 'count'),
                                   nonfinite_unclipped=flag, **kw)
            assert np.array_equal(r2['count'].cpu().numpy(), ref['count']), (what, kw)
            np.testing.assert_allclose(r2['mean_f64'].cpu().numpy(), ref['mean'], rtol=4e-16, atol=0, equal_nan=True, err_msg=what)
    if dtype == np.float32 and N >= 16:
        # the forms part on the columns of row 7 that hold a NaN / inf (unless nothing is rejected there anyway)
        a = apref.combine_ccdproc(cube, form='legacy')['count']
        b = apref.combine_ccdproc(cube, form='astropy')['count']
        assert (a != b).any() and np.array_equal(a[:7], b[:7]) and np.array_equal(a[8:], b[8:])


def test_ccdproc_configuration_guard(ops, apref):
    """The median / mad_std pair's guard: float32 frames with a NaN in every 64-pixel block send every block to the rich kernel; the
    call after that tries only every 16th tile (mode 1) and hands the rest over untried; clean data bring the fast kernel back
    one call later.  Results against the oracle in every mode."""
    rng = np.random.default_rng(801)
    N, H, W = 32, 128, 512                                   # 256 tiles, 1024 blocks, 16 sampled tiles
    clean = rng.normal(1000.0, 12.0, (N, H, W)).astype(np.float32)
    bad = clean.copy()
    bad[3].reshape(-1)[::61] = np.nan                        # at least one NaN per 64-pixel block
    nblocks = H * W // 64
    ref = {id(clean): apref.combine_ccdproc(clean, form='legacy'), id(bad): apref.combine_ccdproc(bad, form='legacy')}
    dc, db = dev(clean, ops), dev(bad, ops)

    def call(d, cube):
        ops.stack_redo_stats(reset=True)
        r = ops.stack_sigclip(d, sigma=5.0, maxiters=1, cenfunc='median', stdfunc='mad_std', outputs=('count', 'mean_f64', 'std_f64'))
        st = ops.stack_redo_stats()
        assert np.array_equal(r['count'].cpu().numpy(), ref[id(cube)]['count'])
        np.testing.assert_allclose(r['mean_f64'].cpu().numpy(), ref[id(cube)]['mean'], rtol=4e-16, atol=0, equal_nan=True)
        np.testing.assert_allclose(r['std_f64'].cpu().numpy(), ref[id(cube)]['std'], rtol=1e-12, atol=1e-12, equal_nan=True)
        assert _zero_prefix_is_zero(ops, ops.stack_workspace(H * W, d.device), H * W)
        return st['blocks_given_up']

    assert call(dc, clean) < nblocks // 8                     # mode 0, clean: the fast kernel carries it
    assert call(db, bad) == nblocks                          # mode 0, bad: every block tried and given up -> mode 1
    assert call(db, bad) == nblocks                          # mode 1: sampled tiles tried (and given up), the others handed over
    assert call(dc, clean) >= nblocks - nblocks // 16         # still mode 1 (the decision is the previous call's): mostly handed over
    assert call(dc, clean) < nblocks // 8                     # the sampled tiles were clean: mode 0 again


@pytest.mark.parametrize('N,dt', [(130, np.float32), (192, np.uint16), (256, np.float32), (300, np.uint16), (320, np.float32), (384, np.float32), (400, np.uint16),
                                  (448, np.float32), (500, np.float32), (512, np.uint16)])
def test_big_stacks_median_and_std_planes_on_the_chunk_path(ops, apref, N, dt):
    """129 .. 512 frames with the median and std planes of the survivors (round 6): the chunked float32 path + its second pass
    (stack_std_pass_kernel) instead of the LDS-resident exact kernel - against the oracle: counts identical, mean and median
    within 1 ulp, std within 2 ulp; fused calibration with per-frame exposure ratios and pedestals, a zero and a NaN in the flat,
    non-finite values, a pixel mask, a partly filled last workgroup."""
    from tests.util import synth_cube, synth_masters
    rng = np.random.default_rng(900 + N)
    shape = (11, 97)
    bias, dark, flat = synth_masters(rng, shape)
    flat[0, 0] = 0.0
    flat[0, 1] = np.nan
    raw = synth_cube(rng, N, shape, dtype=dt)
    if dt == np.float32:
        raw = raw + bias + 0.4 * dark
        raw[5, 3, 4] = np.inf
        raw[7, 2, 2] = np.nan
    nflat, _ = apref.flat_normalize(flat)
    e = rng.uniform(0.3, 0.5, N)
    ped = np.where(rng.random(N) < 0.3, -50.0, 0.0)
    pm = (rng.random(shape) < 0.05).astype(np.uint8)
    cal = apref.calibrate(raw, bias, dark, nflat, e, ped, True)
    calib = dict(bias=dev(bias, ops), dark=dev(dark, ops), nflat=dev(nflat, ops), exp_ratio=e, pedestal=ped, dark_still_biased=True)
    d = dev(raw, ops)
    name = ops.stack_kernel_name(N, 'f32' if dt == np.float32 else 'u16', calibrated=True, outputs=('mean', 'median', 'std'))
    assert 'stack_chunks_kernel' in name, name
    for outs in (('mean', 'median', 'std', 'count'), ('median',), ('std', 'count'), ('mean', 'count', 'mean_f64', 'std_f64')):
        for kw in (dict(sigma=3.0, maxiters=5), dict(sigma=2.0, maxiters=None), dict(sigma_lower=2.5, sigma_upper=4.0, maxiters=2)):
            ref = apref.stack_sigclip(cal, pixmask=pm, **kw)
            r = ops.stack_sigclip(d, calib=calib, pixmask=dev(pm, ops), outputs=outs, **kw)
            what = f'big rich N={N} {dt.__name__} {outs} {kw}'
            if 'count' in outs:
                assert np.array_equal(r['count'].cpu().numpy(), ref['count']), what
            if 'mean' in outs:
                assert_ulp(r['mean'].cpu().numpy(), ref['mean'].astype(np.float32), 1, 'mean ' + what)
            if 'median' in outs:
                assert_ulp(r['median'].cpu().numpy(), ref['median'].astype(np.float32), 1, 'median ' + what)
            if 'std' in outs:
                assert_ulp(r['std'].cpu().numpy(), ref['std'].astype(np.float32), 2, 'std ' + what)
            if 'mean_f64' in outs:                            # the float64 planes (ApStack, the N-shard exchange): from the second pass
                np.testing.assert_allclose(r['mean_f64'].cpu().numpy(), ref['mean'], rtol=1e-13, equal_nan=True, err_msg=what)
                np.testing.assert_allclose(r['std_f64'].cpu().numpy(), ref['std'], rtol=1e-11, atol=1e-12, equal_nan=True, err_msg=what)
    # plain (unfused) frames as well
    ref = apref.stack_sigclip(raw.astype(np.float32), sigma=3.0, maxiters=5)
    r = ops.stack_sigclip(d, sigma=3.0, maxiters=5, outputs=('mean', 'median', 'std', 'count'))
    assert np.array_equal(r['count'].cpu().numpy(), ref['count'])
    assert_ulp(r['median'].cpu().numpy(), ref['median'].astype(np.float32), 1, 'plain median')
    assert_ulp(r['std'].cpu().numpy(), ref['std'].astype(np.float32), 2, 'plain std')


@pytest.mark.parametrize('N,dtype', [(129, np.float32), (192, np.uint16), (200, np.float32), (256, np.float32), (256, np.uint16), (257, np.float32),
                                     (300, np.uint16), (320, np.float32), (384, np.float32), (385, np.uint16), (448, np.float32), (449, np.float32), (512, np.float32), (512, np.uint16)])
def test_ccdproc_configuration_129_to_512_frames(ops, apref, N, dtype):
    """The ccdproc.combine configuration (ap_combine_darks.py:394-420: one pass of median / mad_std at 5 deviations, float64 planes)
    beyond 128 frames (round 6): three chunked passes - the column's middle values, the middle deviations, the float64 sums of what
    the bounds keep - with the exact kernel behind them for the pixels they are not sure of.  Both published forms against the oracle:
    counts identical, float64 mean to 4e-16, std to 1e-12; the same numbers from the exact kernel alone and without a workspace."""
    H, W = 9, 131
    rng = np.random.default_rng(1700 + N + (1 if dtype == np.uint16 else 0))
    cube = rng.normal(1000.0, 12.0, (N, H, W))
    hits = rng.random(cube.shape) < 0.01
    cube[hits] += rng.uniform(100, 5000, hits.sum())
    for k in range(3, 40):                                   # columns with k outliers on one side (the clipped mean's tails hold 8 / 16)
        sgn = 1.0 if k % 2 else -0.4
        cube[:k, 2, k] += sgn * 2000.0
    cube[:, 3, :] = np.rint(rng.normal(500.0, 0.6, (N, W)))  # a few distinct integer values: ties, often MAD = 0
    cube[:, 4, :] = 777.0                                     # constant columns
    cube[:, 5, :] = np.rint(rng.normal(300.0, 2.0, (N, W)))
    for x in range(0, W, 3):                                  # a value next to the upper bound (+- a few ulp)
        col = np.sort(cube[1:, 6, x].astype(np.float32).astype(np.float64))
        base = np.median(col)
        mad = np.median(np.abs(col - base))
        cube[0, 6, x] = base + 5 * 1.482602218505602 * mad * (1 + rng.integers(-3, 4) * 2.0 ** -23)
    cube[:, 8, :] += np.linspace(0, 60, N)[:, None]          # a drift of five sigma over the sequence (interleaved chunks)
    if dtype == np.uint16:
        cube = np.clip(np.rint(cube), 0, 65535).astype(np.uint16)
    else:
        cube = cube.astype(np.float32)
        cube[1, 7, 10:40] = np.nan
        cube[2, 7, 50] = np.inf
        cube[:, 7, 60] = np.nan
    d = dev(cube, ops)
    name = ops.stack_kernel_name(N, 'f32' if dtype == np.float32 else 'u16', calibrated=False, outputs=('mean_f64', 'std_f64'), stdfunc='mad_std', maxiters=1)
    assert 'stack_rank_chunks_kernel' in name, name
    for form, flag in (('legacy', False), ('astropy', True)):
        what = '%d frames %s %s' % (N, np.dtype(dtype).name, form)
        ref = apref.combine_ccdproc(cube.astype(np.float32) if dtype == np.uint16 else cube, form=form)
        for kw in (dict(), dict(workspace=False), dict(exact=True)):
            ops.stack_redo_stats(reset=True)
            r = ops.stack_sigclip(d, sigma=5.0, maxiters=1, cenfunc='median', stdfunc='mad_std', outputs=('mean', 'count', 'mean_f64', 'std_f64'),
                                  nonfinite_unclipped=flag, **kw)
            assert np.array_equal(r['count'].cpu().numpy(), ref['count']), (what, kw)
            np.testing.assert_allclose(r['mean_f64'].cpu().numpy(), ref['mean'], rtol=4e-16, atol=0, equal_nan=True, err_msg=what)
            assert_ulp(r['mean'].cpu().numpy(), ref['mean'].astype(np.float32), 1, what)
            np.testing.assert_allclose(r['std_f64'].cpu().numpy(), ref['std'], rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=what)
            if not kw:
                st = ops.stack_redo_stats()
                # the chunked passes carry most of the image: rows 3 (ties at the bound when MAD = 0 are decided exactly), 6 and 7 hold the unsure ones
                assert st['calls'] == 1 and st['pixels'] == H * W and st['pixels_listed'] < 0.25 * H * W, (what, st)
                assert _zero_prefix_is_zero(ops, ops.stack_workspace(H * W, d.device), H * W), what
    # asymmetric thresholds
    ref = apref.combine_ccdproc(cube.astype(np.float32) if dtype == np.uint16 else cube, low=3.0, high=4.0, form='astropy')
    r = ops.stack_sigclip(d, sigma_lower=3.0, sigma_upper=4.0, maxiters=1, cenfunc='median', stdfunc='mad_std', outputs=('count', 'mean_f64'), nonfinite_unclipped=True)
    assert np.array_equal(r['count'].cpu().numpy(), ref['count'])
    np.testing.assert_allclose(r['mean_f64'].cpu().numpy(), ref['mean'], rtol=4e-16, atol=0, equal_nan=True)
    # a row stripe of the slab reduced in place (frame_stride > n_pixels, an odd first pixel)
    rs = ops.stack_sigclip(d[:, 1:8], sigma_lower=3.0, sigma_upper=4.0, maxiters=1, cenfunc='median', stdfunc='mad_std', outputs=('count', 'mean_f64', 'std_f64'),
                           nonfinite_unclipped=True)
    assert np.array_equal(rs['count'].cpu().numpy(), ref['count'][1:8])
    np.testing.assert_allclose(rs['mean_f64'].cpu().numpy(), ref['mean'][1:8], rtol=4e-16, atol=0, equal_nan=True)
    np.testing.assert_allclose(rs['std_f64'].cpu().numpy(), ref['std'][1:8], rtol=1e-12, atol=1e-12, equal_nan=True)


@pytest.mark.parametrize('N,dtype', [(129, np.float32), (200, np.uint16), (256, np.float32), (257, np.uint16), (300, np.float32), (384, np.uint16),
                                     (320, np.uint16), (440, np.float32), (448, np.uint16), (450, np.float32), (512, np.float32), (512, np.uint16)])
def test_plain_median_129_to_512_frames(ops, apref, N, dtype):
    """np.nanmedian along N (config 4) beyond 128 frames on the chunked windows (round 6): an order statistic, so bit-exact; columns
    holding NaN / inf, a partly filled last workgroup, a drifting sequence, few distinct values."""
    H, W = 7, 150
    rng = np.random.default_rng(2700 + N)
    cube = rng.normal(1000.0, 12.0, (N, H, W))
    cube[:, 1, :] = np.rint(rng.normal(500.0, 0.6, (N, W)))
    cube[:, 2, :] = 42.0
    cube[:, 3, :] += np.linspace(0, 100, N)[:, None]
    cube[:, 4, :] = np.sort(cube[:, 4, :], axis=0)           # monotone in acquisition order
    if dtype == np.uint16:
        cube = np.clip(np.rint(cube), 0, 65535).astype(np.uint16)
    else:
        cube = cube.astype(np.float32)
        cube[3, 5, 5:60] = np.nan
        cube[4, 5, 70] = np.inf
        cube[:, 5, 80] = np.nan
    d = dev(cube, ops)
    name = ops.stack_kernel_name(N, 'f32' if dtype == np.float32 else 'u16', calibrated=False, median_only=True)
    assert 'stack_rank_chunks_kernel' in name, name
    med, cnt = ops.stack_median(d, want_count=True)
    with np.errstate(all='ignore'):
        ref = apref.stack_median(cube.astype(np.float32))
    got = med.cpu().numpy()
    same = (got == ref.astype(np.float32)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), (N, np.argwhere(~same)[:5])
    assert np.array_equal(cnt.cpu().numpy(), (~np.isnan(cube.astype(np.float32))).sum(0))
    np.testing.assert_array_equal(ops.stack_median(d[:, 1:6]).cpu().numpy(), got[1:6])       # a row stripe reduced in place (NaN == NaN here)


@pytest.mark.parametrize('N,dtype', [(130, np.uint16), (192, np.float32), (256, np.uint16), (257, np.float32), (300, np.uint16), (384, np.float32),
                                     (400, np.uint16), (448, np.float32), (512, np.uint16), (512, np.float32)])
def test_calibrated_median_129_to_512_frames(ops, apref, N, dtype):
    """Config 4's reduction (fused bias / dark / flat + median along N) beyond 128 frames on the chunked windows (round 6, MODE 3): per-frame
    exposure ratios and pedestals, a zero and a NaN in the flat, non-finite values, a pixel mask - against the oracle's median of the
    calibrated cube (float32 values, so the median is exact up to the rounding of the middle pair's mean: 1 ulp), counts, a row stripe."""
    from tests.util import synth_cube
    rng = np.random.default_rng(3900 + N)
    shape = (10, 83)
    bias, dark, flat = synth_masters(rng, shape)
    flat[0, 0] = 0.0
    flat[0, 1] = np.nan
    raw = synth_cube(rng, N, shape, dtype=dtype)
    if dtype == np.float32:
        raw = raw + bias + 0.4 * dark
        raw[5, 3, 4] = np.inf
        raw[7, 2, 2] = np.nan
    nflat, _ = apref.flat_normalize(flat)
    e = rng.uniform(0.3, 0.5, N)
    ped = np.where(rng.random(N) < 0.3, -50.0, 0.0)
    pm = (rng.random(shape) < 0.05).astype(np.uint8)
    cal = apref.calibrate(raw, bias, dark, nflat, e, ped, True)
    d = dev(raw, ops)
    name = ops.stack_kernel_name(N, 'f32' if dtype == np.float32 else 'u16', calibrated=True, median_only=True)
    assert 'stack_rank_chunks_kernel' in name and name.rstrip('>').endswith('3'), name
    for use_ped, use_pm in ((True, True), (False, False)):
        calib = dict(bias=dev(bias, ops), dark=dev(dark, ops), nflat=dev(nflat, ops), exp_ratio=e, pedestal=ped if use_ped else None, dark_still_biased=True)
        c = cal if use_ped else apref.calibrate(raw, bias, dark, nflat, e, None, True)
        with np.errstate(all='ignore'):
            mm = apref.stack_median(c).astype(np.float32)
        nn = (~np.isnan(c)).sum(0).astype(np.int32)
        if use_pm:
            mm[pm != 0] = np.nan
            nn[pm != 0] = 0
        med, cnt = ops.stack_median(d, calib=calib, pixmask=dev(pm, ops) if use_pm else None, want_count=True)
        what = 'calibrated median N=%d %s ped=%s mask=%s' % (N, np.dtype(dtype).name, use_ped, use_pm)
        assert np.array_equal(cnt.cpu().numpy(), nn), what
        assert_ulp(med.cpu().numpy(), mm, 1, what)
        rows = ops.stack_median(d[:, 2:9], calib={k: (v[2:9] if k in ('bias', 'dark', 'nflat') else v) for k, v in calib.items()},
                                pixmask=dev(pm[2:9], ops) if use_pm else None)
        np.testing.assert_array_equal(rows.cpu().numpy(), med[2:9].cpu().numpy(), err_msg='stripe ' + what)


@pytest.mark.parametrize('N,dtype', [(130, np.float32), (256, np.float32), (300, np.uint16), (512, np.float32)])
def test_ccdproc_configuration_129_to_512_frames_rejecting_everything(ops, apref, N, dtype):
    """mad_std with sigma = 0.5 on two-level columns of an even length: the bounds median +- 0.5 * 1.4826 MAD lie inside both
    levels, so the chunked sums pass rejects every value with certainty.  Nothing survives: count 0, mean and std NaN, as in the
    oracle (and in the exact kernel)."""
    H, W = 4, 96
    rng = np.random.default_rng(1900 + N)
    lo = np.rint(rng.uniform(200.0, 900.0, (H, W)))
    hi = lo + np.rint(rng.uniform(3.0, 40.0, (H, W)))
    two = np.zeros((N, H, W), bool)
    two[: N // 2] = True
    two = rng.permuted(two, axis=0)
    cube = np.where(two, hi[None], lo[None])
    cube[:, 3, :] = rng.normal(500.0, 10.0, (N, W))                   # ordinary columns next to them
    cube = np.clip(np.rint(cube), 0, 65535).astype(np.uint16) if dtype == np.uint16 else cube.astype(np.float32)
    d = dev(cube, ops)
    for form, flag in (('legacy', False), ('astropy', True)):
        ref = apref.combine_ccdproc(cube.astype(np.float32) if dtype == np.uint16 else cube, low=0.5, high=0.5, form=form)
        assert (ref['count'][:3] == 0).all() and np.isnan(ref['std'][:3]).all() and np.isnan(ref['mean'][:3]).all()
        for kw in (dict(), dict(exact=True)):
            what = '%d frames %s %s %s' % (N, np.dtype(dtype).name, form, kw)
            r = ops.stack_sigclip(d, sigma=0.5, maxiters=1, cenfunc='median', stdfunc='mad_std', outputs=('mean', 'count', 'mean_f64', 'std_f64'),
                                  nonfinite_unclipped=flag, **kw)
            assert np.array_equal(r['count'].cpu().numpy(), ref['count']), what
            np.testing.assert_allclose(r['mean_f64'].cpu().numpy(), ref['mean'], rtol=4e-16, atol=0, equal_nan=True, err_msg=what)
            np.testing.assert_allclose(r['std_f64'].cpu().numpy(), ref['std'], rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=what)
            assert_ulp(r['mean'].cpu().numpy(), ref['mean'].astype(np.float32), 1, what)
