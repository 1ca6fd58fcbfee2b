"""Frame normalisation and weights inside the rejection rules (APGPU_STACK_FRAME_PARAMS, csrc/stack_reject.hip) on the GPU:
mean_f64, std_f64 and count equal the NumPy model (tests/stack_frame_model.py) bit for bit, mean and std are their roundings -
at every slot count's edges, on special values, on the tie rule and the frame order; the flag's errors; the guard bands of
tests/guard.py; ops.frame_stats; and end to end on the scene the feature was added for."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import stack_frame_model as model
from tests.guard import current, guarded, intact, place, unchanged
from tests.util import assert_biteq, synth_cube

pytestmark = pytest.mark.gpu
F = np.float32
OUTPUTS = ('mean', 'std', 'count', 'mean_f64', 'std_f64')
RULES = (('winsorized', dict(sigma_lower=2.5, sigma_upper=3.0)), ('minmax', dict(nlow=1, nhigh=2)))


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _model(values, a, b, w, method, kw, pixmask=None):
    values = np.asarray(values, F)
    values = values.reshape(values.shape[0], -1)
    if method == 'winsorized':
        rule = dict(kl=kw.get('sigma_lower', 3.0), kh=kw.get('sigma_upper', 3.0), maxiters=kw.get('maxiters'))
    else:
        rule = dict(nlow=kw.get('nlow', 1), nhigh=kw.get('nhigh', 1))
    return model.frame_params(values, a, b, w, method, pixmask=None if pixmask is None else pixmask.reshape(-1), **rule)


def _compare(got, ref, what):
    with np.errstate(over='ignore', invalid='ignore'):
        want = dict(count=ref['count'], mean_f64=ref['mean_f64'], std_f64=ref['std_f64'], mean=ref['mean_f64'].astype(F),
                    std=ref['std_f64'].astype(F))
    for k in OUTPUTS:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert_biteq(g, want[k].reshape(g.shape), '%s: %s' % (what, k))
        if k in ('mean', 'std'):                             # the NaN of a pixel without data: quiet, positive, no payload
            assert (g.view(np.uint32)[np.isnan(g)] == 0x7fc00000).all(), what


def _check(raw, a, b, w, method, kw, what, values=None, pixmask=None):
    from astrophotography_amd import ops
    values = np.asarray(raw, F) if values is None else values
    ref = _model(values, a, b, w, method, kw, pixmask)
    t = raw if torch.is_tensor(raw) else _dev(raw)
    got = ops.stack_reject(t, method, pixmask=None if pixmask is None else _dev(pixmask), outputs=OUTPUTS, scale=a, offset=b,
                           weights=w, **kw)
    _compare(got, ref, what)
    return ref


def _params(rng, n):
    return (rng.uniform(0.5, 2.0, n).astype(F), rng.uniform(-300.0, 300.0, n).astype(F), rng.uniform(0.05, 1.0, n).astype(F))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F, np.uint16], ids=['f32', 'u16'])
@pytest.mark.parametrize('method, kw', RULES, ids=[r[0] for r in RULES])
def test_slot_edges(method, kw, dtype):
    """P = 200: three full wavefronts and a partial one."""
    from astrophotography_amd import ops
    rng = np.random.default_rng(16)
    for n in (1, 2, 3, 8, 9, 16, 17, 32, 33, 64, 65, 128):
        raw = synth_cube(rng, n, (200,), nan_frac=0.02 if dtype == F else 0.0, dtype=dtype)
        a, b, w = _params(rng, n)
        _check(raw, a, b, w, method, kw, '%s %d frames' % (method, n))
    # missing parameters default to 1, 0, 1; all-ones parameters keep the existing rule's survivors, count and std
    raw = synth_cube(rng, 12, (200,), nan_frac=0.02 if dtype == F else 0.0, dtype=dtype)
    t = _dev(raw)
    _, b, w = _params(rng, 12)
    got = ops.stack_reject(t, method, outputs=OUTPUTS, offset=b, **kw)
    _compare(got, _model(raw, np.ones(12), b, np.ones(12), method, kw), 'offset only')
    got = ops.stack_reject(t, method, outputs=OUTPUTS, weights=w, **kw)
    _compare(got, _model(raw, np.ones(12), np.zeros(12), w, method, kw), 'weights only')
    plain = ops.stack_reject(t, method, outputs=OUTPUTS, **kw)
    for k in ('count', 'std', 'std_f64'):
        assert_biteq(got[k].cpu().numpy(), plain[k].cpu().numpy(), k)


@pytest.mark.parametrize('method, kw', RULES, ids=[r[0] for r in RULES])
def test_special_values(method, kw):
    rng = np.random.default_rng(8)
    n, P = 20, 130
    cube = synth_cube(rng, n, (P,), nan_frac=0.15)
    cube[:, 0] = np.nan                                      # nothing finite
    cube[:, 1] = np.inf
    cube[:, 2] = [np.nan, np.inf, -np.inf, 1.0] * 5          # few finite values
    cube[1:, 3] = np.nan                                     # one value
    cube[2:, 4] = -np.inf                                    # two
    cube[:, 5] = 3.5                                         # constant before the map
    cube[:, 6] = 0.0                                         # zeros: the map below makes -0.0 of some
    cube[:, 7] = [0.0, -0.0] * 10
    cube[:, 8] = 3e38                                        # the map sends these out of range in the frames with a > 1
    a, b, w = _params(rng, n)
    pm = (rng.random(P) < 0.1).astype(np.uint8)
    pm[:9] = 0
    _check(cube, a, b, w, method, kw, 'special values')
    _check(cube, a, b, w, method, kw, 'special values, mask', pixmask=pm)
    # offsets of -0.0 and scales of either sign: v = -0.0 where a x = -0.0 (a < 0, x = +0; a > 0, x = -0), else +0.0
    a0 = np.where(np.arange(n) % 3 == 0, -1.0, 1.0).astype(F)
    b0 = np.where(np.arange(n) % 2 == 0, -0.0, 0.0).astype(F)
    ref = _check(cube, a0, b0, w, method, kw, 'zeros of both signs')
    assert np.signbit(ref['v'][:, 6]).any() and not np.signbit(ref['v'][:, 6]).all()
    for rule in ((dict(nlow=1, nhigh=0), dict(nlow=0, nhigh=3), dict(nlow=9, nhigh=9), dict(nlow=0, nhigh=0)) if method == 'minmax' else
                 (dict(maxiters=1), dict(sigma_lower=0.0, sigma_upper=0.0), dict(sigma_lower=1.0, sigma_upper=4.0))):
        _check(cube, a0, b0, w, method, rule, 'zeros of both signs %r' % (rule,))
        _check(cube, a, b, w, method, rule, 'special values %r' % (rule,))
    # columns left with 0, 1 and 2 survivors by the rule itself
    if method == 'minmax':
        few = synth_cube(rng, 5, (70,))
        a5, b5, w5 = _params(rng, 5)
        for nlow, nhigh in ((3, 2), (2, 2), (1, 2)):
            r = _check(few, a5, b5, w5, 'minmax', dict(nlow=nlow, nhigh=nhigh), 'few survivors')
            assert (r['count'] == 5 - nlow - nhigh).all()


@pytest.mark.parametrize('method, kw', RULES, ids=[r[0] for r in RULES])
def test_row_stripes(method, kw):
    """frames[:, r0:r1] of a contiguous slab is reduced in place (frame_stride > n_pixels)."""
    rng = np.random.default_rng(5)
    n, H, W = 10, 19, 67
    a, b, w = _params(rng, n)
    for dtype in (F, np.uint16):
        cube = synth_cube(rng, n, (H, W), nan_frac=0.01 if dtype == F else 0.0, dtype=dtype)
        t = _dev(cube)
        for r0, r1 in ((0, 5), (5, 6), (7, 19)):
            stripe = t[:, r0:r1]
            assert stripe.stride(0) == H * W
            _check(stripe, a, b, w, method, kw, 'rows %d:%d' % (r0, r1), values=cube[:, r0:r1].astype(F))


def test_tie_rule_decides_the_weighted_mean():
    """Two frames whose MAPPED values are equal, weights 0.1 and 1.0, nlow = 1, everything else larger: the lower frame index
    goes, and the weighted mean says which one went."""
    n = 9
    raw = np.full((n, 70), 50.0, F) + np.arange(n, dtype=F)[:, None]
    a = np.ones(n, F)
    b = np.zeros(n, F)
    w = np.ones(n, F)
    raw[2], a[2], b[2], w[2] = 5.0, 2.0, 1.0, 0.1          # 2 * 5 + 1 = 11
    raw[6], a[6], b[6], w[6] = 22.0, 0.5, 0.0, 1.0         # 0.5 * 22 = 11
    ref = _check(raw, a, b, w, 'minmax', dict(nlow=1, nhigh=0), 'tie')
    assert ref['v'][2, 0] == ref['v'][6, 0] == 11.0
    assert not ref['keep'][2, 0] and ref['keep'][6, 0]
    other = ref['keep'][:, 0].copy()
    other[[2, 6]] = [True, False]
    v = ref['v'][:, 0].astype(np.float64)
    m_other = (w[other].astype(np.float64) * v[other]).sum() / w[other].astype(np.float64).sum()
    assert abs(m_other - ref['mean_f64'][0]) > 1.0
    # the high end: the LAST of the equal values goes
    ref = _check(-raw, a, -b, w, 'minmax', dict(nlow=0, nhigh=1), 'tie, high end')
    assert ref['keep'][2, 0] and not ref['keep'][6, 0]


def test_winsorized_weights_follow_the_frames_not_the_compact_column():
    """Columns where round 2 removes a value that round 1 kept and that lies between two survivors in frame order: weights
    looked up at the positions of the compact column would be those of other frames."""
    from tests import stack_reject_model as reject
    rng = np.random.default_rng(11)
    n = 12
    raw = rng.normal(0.0, 1.0, (n, 400)).astype(F)
    raw[3] += 8.0
    raw[7, ::2] += 4.0
    one, free = reject.winsorized(raw, 2.0, 2.0, maxiters=1)['keep'], reject.winsorized(raw, 2.0, 2.0)['keep']
    later = one & ~free                                      # removed after round 1
    idx = np.arange(n)[:, None]
    first = np.where(free, idx, n).min(0)
    last = np.where(free, idx, -1).max(0)
    between = (later & (idx > first) & (idx < last)).any(0)
    assert between.sum() >= 20, between.sum()
    w = (np.arange(n) + 1.0).astype(F) / F(n)
    a, b = np.ones(n, F), np.zeros(n, F)
    ref = _check(raw, a, b, w, 'winsorized', dict(sigma_lower=2.0, sigma_upper=2.0), 'rounds')
    assert (ref['keep'] == free).all()
    # the weights of the compact positions give another mean in those columns
    v = raw.astype(np.float64)
    c = int(np.flatnonzero(between)[0])
    k = free[:, c]
    wrong = (w[:k.sum()].astype(np.float64) * v[k, c]).sum() / w[:k.sum()].astype(np.float64).sum()
    assert abs(wrong - ref['mean_f64'][c]) > 1e-3
    _check(raw, a, b, w, 'winsorized', dict(sigma_lower=2.0, sigma_upper=2.0, maxiters=1), 'one round')
    a, b, w = _params(rng, n)
    _check(raw, a, b, w, 'winsorized', dict(sigma_lower=2.0, sigma_upper=2.0), 'rounds, random parameters')


# ---------------------------------------------------------------------------------------------------------------------------
def _abi_args(frames, n, P, flags, mean, **kw):
    from astrophotography_amd import _lib
    a = _lib.StackArgs()
    a.frames, a.dtype, a.n_frames, a.n_pixels, a.frame_stride = frames.data_ptr(), 0, n, P, P
    a.center, a.dev, a.maxiters = 0, 0, -1
    a.sigma_lower, a.sigma_upper = (1.0, 1.0) if flags & _lib.STACK_REJECT_MINMAX else (3.0, 3.0)
    a.mean = mean.data_ptr()
    a.flags = flags
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_flag_errors():
    from astrophotography_amd import _lib
    lib = _lib.load()
    W, M, FP = _lib.STACK_REJECT_WINSORIZED, _lib.STACK_REJECT_MINMAX, _lib.STACK_FRAME_PARAMS
    n, P = 6, 100
    frames = torch.ones((n, P), device='cuda')
    plane = torch.zeros(P, device='cuda')
    block = torch.ones((3, n), device='cuda')
    mean = torch.full((P,), -7.0, device='cuda')
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e = block.data_ptr()
    for a, want in ((_abi_args(frames, n, P, FP, mean, exp_ratio=e), _lib.E_UNSUPPORTED),
                    (_abi_args(frames, n, P, FP | W, mean), _lib.E_INVAL),
                    (_abi_args(frames, n, P, FP | M, mean), _lib.E_INVAL),
                    (_abi_args(frames, n, P, FP | W, mean, exp_ratio=e, bias=plane.data_ptr(), dark=plane.data_ptr()), _lib.E_INVAL),
                    (_abi_args(frames, n, P, FP | M, mean, exp_ratio=e, pedestal=e), _lib.E_INVAL),
                    (_abi_args(frames, n, P, FP | W | M, mean, exp_ratio=e), _lib.E_INVAL)):
        assert lib.apgpu_stack_sigclip(C.byref(a), st) == want, lib.apgpu_last_error()
    a = _abi_args(frames, n, P, FP, mean, exp_ratio=e, median=mean.data_ptr())
    a.mean = None
    assert lib.apgpu_stack_median(C.byref(a), st) == _lib.E_UNSUPPORTED
    a = _abi_args(frames.reshape(n, 10, 10), n, P, FP | W, mean, exp_ratio=e)
    aff = torch.tensor([[1.0, 0, 0, 0, 1, 0]] * n, dtype=torch.float64, device='cuda')
    lut = torch.zeros(6 * 1025, device='cuda')
    r = lib.apgpu_resample_stack_sigclip(C.byref(a), 10, 10, None, aff.data_ptr(), 0, 0, None, lut.data_ptr(), 1024, 10, 10, None, 0, st)
    assert r == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (mean == -7.0).all()                              # a refused call wrote nothing
    a = _abi_args(frames, n, P, FP | W, mean, exp_ratio=e)  # and the good call
    assert lib.apgpu_stack_sigclip(C.byref(a), st) == 0, lib.apgpu_last_error()
    torch.cuda.synchronize()
    assert (mean == 2.0).all()                               # scale 1, offset 1 on frames of ones


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method, kw', RULES, ids=[r[0] for r in RULES])
def test_guard_bands(method, kw, monkeypatch):
    """Two poisons, inputs one element off alignment, a side stream: no load outside an input reaches a result, no store leaves
    an output, no input - the frames, the mask, the [3][N] block - is written, and the call runs on the current stream."""
    from astrophotography_amd import _lib, ops
    rng = np.random.default_rng(77)
    n, P = 13, 1031
    raw = synth_cube(rng, n, (P,), dtype=np.uint16)
    f32 = synth_cube(rng, n, (P,), nan_frac=0.02)
    pm = (rng.random(P) < 0.05).astype(np.uint8)
    a, b, w = _params(rng, n)
    refs = [_model(raw, a, b, w, method, kw, pm), _model(f32, a, b, w, method, kw)]
    G = 64 * 1024

    def run(poison, shift):
        with guarded(monkeypatch, G) as g:
            toks = []

            def dev(x):
                t, tok = place(x, poison, shift * x.dtype.itemsize, G)
                toks.append(tok)
                return t
            r1 = ops.stack_reject(dev(raw), method, pixmask=dev(pm), outputs=OUTPUTS, scale=a, offset=b, weights=w, **kw)
            r2 = ops.stack_reject(dev(f32), method, outputs=OUTPUTS, scale=a, offset=b, weights=w, **kw)
            torch.cuda.current_stream().synchronize()
            for tok in toks:
                unchanged(tok)
            out = [{k: v.cpu().numpy() for k, v in r.items()} for r in (r1, r2)]
        return out, g.lib.streams()

    default = torch.cuda.default_stream().cuda_stream
    A, sa = run(0xFF, 0)
    assert sa and all(s == default for _, s in sa)
    B, _ = run(0x00, 1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Cr, sc = run(0xFF, 1)
    assert sc and all(s == side.cuda_stream for _, s in sc)
    for i in range(2):
        _compare(A[i], refs[i], 'run A %d' % i)
        for other, tag in ((B, 'poison 0x00, shifted'), (Cr, 'side stream')):
            for k in OUTPUTS:
                assert_biteq(other[i][k], A[i][k], '%s: %s' % (tag, k))

    # the C ABI itself with every buffer of the call inside a poisoned surround: the [3][N] block, the outputs
    lib = _lib.load()
    for poison in (0xFF, 0x00):
        frames, ftok = place(f32, poison, 4, G)
        block, btok = place(np.stack([a, b, w]).astype(F), poison, 4, G)
        mean, mtok = place(np.zeros(P, F), poison, 4, G, what='mean')
        m64, dtok = place(np.zeros(P, np.float64), poison, 0, G, what='mean_f64')
        cnt, ctok = place(np.zeros(P, np.int32), poison, 4, G, what='count')
        args = _abi_args(frames, n, P, _lib.STACK_FRAME_PARAMS | (_lib.STACK_REJECT_MINMAX if method == 'minmax' else _lib.STACK_REJECT_WINSORIZED),
                         mean, exp_ratio=block.data_ptr(), mean_f64=m64.data_ptr(), count=cnt.data_ptr())
        if method == 'minmax':
            args.sigma_lower, args.sigma_upper = float(kw['nlow']), float(kw['nhigh'])
        else:
            args.sigma_lower, args.sigma_upper = kw['sigma_lower'], kw['sigma_upper']
        _lib.check(lib.apgpu_stack_sigclip(C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        unchanged(ftok)
        unchanged(btok)
        for tok in (mtok, dtok, ctok):
            intact(tok)
        assert_biteq(current(dtok).view(np.float64), refs[1]['mean_f64'], 'ABI mean_f64')
        assert_biteq(current(ctok).view(np.int32), refs[1]['count'], 'ABI count')
        assert_biteq(current(mtok).view(F), refs[1]['mean_f64'].astype(F), 'ABI mean')


# ---------------------------------------------------------------------------------------------------------------------------
def test_frame_stats_is_sigclip_global_per_frame():
    from astrophotography_amd import ops
    rng = np.random.default_rng(40)
    cube = rng.normal(300.0, 12.0, (5, 40, 70)).astype(F)
    cube[rng.random(cube.shape) < 0.01] += 2000.0
    cube[rng.random(cube.shape) < 0.03] = np.nan
    cube[3] = 17.5                                           # a constant frame
    t = _dev(cube)
    for kw in (dict(), dict(sigma=2.0, maxiters=2)):
        st = ops.frame_stats(t, **kw)
        assert st.shape == (5, 2) and st.dtype == torch.float64 and st.is_cuda
        want = np.stack([ops.sigclip_global(t[i], **kw).cpu().numpy()[1:3] for i in range(5)])
        assert_biteq(st.cpu().numpy(), want)
    assert st[3].tolist() == [17.5, 0.0]
    u = _dev(np.clip(np.nan_to_num(cube[:2], nan=300.0), 0, 65535).astype(np.uint16))
    assert_biteq(ops.frame_stats(u).cpu().numpy(), np.stack([ops.sigclip_global(u[i]).cpu().numpy()[1:3] for i in range(2)]))
    empty = _dev(np.full((2, 8, 8), np.nan, F))
    with pytest.raises(ValueError, match='frame 0 has no finite pixel'):
        ops.frame_normalization(ops.frame_stats(empty), 'additive')
    with pytest.raises(ValueError, match='frame 3 has scale S = 0'):
        ops.frame_normalization(ops.frame_stats(t), 'additive+scaling')
    assert np.array_equal(ops.background_weights(t[:3]), 1.0 / ops.frame_stats(t[:3]).cpu().numpy()[:, 1] ** 2)


# ---------------------------------------------------------------------------------------------------------------------------
# truth: the trail under unequal sky
N_TRAIL = 10
# The row's mean error against the scene at the reference's sky, over the W - 2 * 8 = 48 interior pixels of the trail row: every
# pixel is the mean of at most N - 2 = 8 values of noise 8, so a pixel's error has sigma 8 / sqrt(8) = 2.83 and the row's mean
# 2.83 / sqrt(48) = 0.41; each frame's offset carries the error of a clipped median over 3072 pixels, 1.25 * 8 / sqrt(3072) =
# 0.18, the reference's in full and the others' averaged: 0.19.  Together sigma = 0.45; the bound is 3 sigma = 1.35 ADU (far
# inside 3 sigma / sqrt(N - 2) = 8.5).  The model on the CPU measures -0.64 ADU over the whole row at this seed, and 23.6 ADU
# without the normalisation (tests/test_stack_frame_model_host.py).
TRAIL_BOUND = 1.35


@pytest.fixture(scope='module')
def trail():
    cube, stars, sky = model.trail_scene(N_TRAIL, seed=20261019 + N_TRAIL)
    return cube, stars, sky


def _trail_checks(image, count, stars, sky, normalised, what):
    row, edge = model.TRAIL_ROW, 8
    cnt = count[row, edge:-edge]
    if not normalised:
        assert (cnt == N_TRAIL).all(), what                  # the sky spread is the sigma the trail is judged by: it stays
        return
    assert (cnt <= N_TRAIL - 2).all() and (cnt >= 4).all(), (what, cnt.min(), cnt.max())
    err = float((image[row, edge:-edge].astype(np.float64) - (stars[row, edge:-edge] + sky[0])).mean())
    print('%s: trail row mean error %+.3f ADU (bound %.2f)' % (what, err, TRAIL_BOUND))
    assert abs(err) <= TRAIL_BOUND, what


def test_trail_coadd_apresample_and_script(trail, tmp_path):
    import yaml
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio, ops
    from astrophotography_amd.scripts import ap_coadd
    cube, stars, sky = trail
    n = cube.shape[0]
    ident = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * n
    t = _dev(cube)
    res, _ = ops.resample_affine(t, ident, weight=False)
    assert torch.isfinite(res[:, 8:-8, 8:-8]).all()
    plain = ops.coadd(t, ident, combine='WINSORIZED', sigma=3.0, maxiters=5)
    assert set(plain) == {'image', 'count'}
    _trail_checks(plain['image'].cpu().numpy(), plain['count'].cpu().numpy(), stars, sky, False, 'ops.coadd none')
    r = ops.coadd(t, ident, combine='WINSORIZED', sigma=3.0, maxiters=5, normalize='additive')
    _trail_checks(r['image'].cpu().numpy(), r['count'].cpu().numpy(), stars, sky, True, 'ops.coadd additive')
    # what ops.coadd did, step by step, against the model
    a, b, w = ops.frame_normalization(ops.frame_stats(res), 'additive')
    assert np.array_equal(a, r['scale']) and np.array_equal(b, r['offset']) and np.array_equal(w, r['norm_weights'])
    assert np.abs(b - (sky[0] - sky)).max() < 1.0
    ref = _model(res.cpu().numpy(), a, b, w, 'winsorized', dict(maxiters=5))
    assert_biteq(r['image'].cpu().numpy().reshape(-1), ref['mean_f64'].astype(F))
    assert_biteq(r['count'].cpu().numpy().reshape(-1), ref['count'])
    # the other combine types get the same map on the slab
    m = ops.coadd(t, ident, combine='MEDIAN', normalize='additive')
    want = ops.stack_median(_dev(model.frame_map(res.cpu().numpy(), a, b)))
    assert_biteq(m['image'].cpu().numpy(), want.cpu().numpy())
    c = ops.coadd(t, ident, combine='CLIPPED', normalize='additive+scaling', reference=3)
    assert abs(float(c['image'][8:-8, 8:-8].median()) - sky[3]) < 2.0
    # the class
    rs = ap.ApResample('CRITICAL', combine='WINSORIZED', sigma=3.0, maxiters=5, conserve_flux=False, normalize='additive')
    rr = rs.coadd(t, ident)
    assert_biteq(rr['image'].cpu().numpy(), r['image'].cpu().numpy())
    # the script: frames of one exposure, identity transforms
    names = []
    for i in range(n):
        names.append(str(tmp_path / ('c%d.fits' % i)))
        h = fitsio.Header()
        h['EXPOSURE'] = 1.0
        fitsio.write(names[-1], cube[i], h)
    with open(tmp_path / 't.yml', 'w') as fh:
        yaml.safe_dump({'transforms': {'c%d.fits' % i: ident[i] for i in range(n)}}, fh)
    common = ['--transforms', str(tmp_path / 't.yml'), '--combine', 'WINSORIZED', '--sigma', '3', '--maxiters', '5', '-l', 'CRITICAL']
    out, wout = str(tmp_path / 'none.fits'), str(tmp_path / 'none_w.fits')
    assert ap_coadd.main([out, *names, *common, '--weight_image', wout]) == 0
    img, h = fitsio.read(out)
    cnt, _ = fitsio.read(wout)
    assert 'NORMMODE' not in h
    _trail_checks(img, cnt, stars, sky, False, 'ap_coadd none')
    out, wout = str(tmp_path / 'add.fits'), str(tmp_path / 'add_w.fits')
    assert ap_coadd.main([out, *names, *common, '--weight_image', wout, '--normalize', 'additive', '--reference', 'c0.fits',
                          '--weighting', 'noise']) == 0
    img, h = fitsio.read(out)
    cnt, _ = fitsio.read(wout)
    _trail_checks(img, cnt, stars, sky, True, 'ap_coadd additive')
    assert h['NORMMODE'] == 'additive' and h['NORMREF'] == 'c0.fits' and h['NSCL000'] == 1.0 and h['NOFF000'] == 0.0
    assert abs(h['NOFF%03d' % (n - 1)] - (sky[0] - sky[-1])) < 1.0 and 0.0 < h['NWGT%03d' % (n - 1)] <= 1.0
    out2 = str(tmp_path / 'ref4.fits')
    assert ap_coadd.main([out2, *names, *common, '--normalize', 'additive', '--reference', '4']) == 0
    img2, h2 = fitsio.read(out2)
    assert h2['NORMREF'] == 'c4.fits' and h2['NOFF004'] == 0.0
    assert abs(float(np.median(img2[8:-8, 8:-8] - img[8:-8, 8:-8])) - (sky[4] - sky[0])) < 1.0


def test_apstack_normalises(trail):
    import astrophotography_amd as ap
    from astrophotography_amd import ops
    cube, stars, sky = trail
    t = _dev(cube)
    st = ap.ApStack('CRITICAL', sigma=3.0, maxiters=5)
    r = st.stack(t, method='winsorized', outputs=('mean', 'count'), normalize='additive', weighting='noise')
    a, b, w = ops.frame_normalization(ops.frame_stats(t), 'additive', weighting='noise')
    assert np.array_equal(w, r['norm_weights']) and w.max() == 1.0
    ref = _model(cube, a, b, w, 'winsorized', dict(maxiters=5))
    assert_biteq(r['mean'].cpu().numpy().reshape(-1), ref['mean_f64'].astype(F))
    assert not ref['keep'][list(model.TRAIL_FRAMES), model.TRAIL_ROW * 64:(model.TRAIL_ROW + 1) * 64].any()
    r = st.stack(t, method='minmax', outputs=('mean', 'count'), normalize='multiplicative', reference=2)
    a, b, w = ops.frame_normalization(ops.frame_stats(t), 'multiplicative', reference=2)
    assert_biteq(r['mean'].cpu().numpy().reshape(-1), _model(cube, a, b, w, 'minmax', dict())['mean_f64'].astype(F))


# ---------------------------------------------------------------------------------------------------------------------------
# truth: the weights.  12 frames, equal sky, noise sigma 4 .. 32.  The model on the CPU (tests/test_stack_frame_model_host.py)
# gives an rms of 5.44 with equal weights and 2.92 with weighting='noise': ratio 0.538 (a plain weighted mean's theory says 0.491;
# the rule removes more of the noisy frames' values than of the quiet ones').  Here each rms is taken over the 32 x 48 interior
# pixels (relative error 1 / sqrt(2 * 1536) = 1.8 %), so the ratio holds within 3 * sqrt(2) * 1.8 % = 7.7 %.
WEIGHT_RATIO = 0.538 * 1.077


def test_noise_weights_lower_the_rms():
    from astrophotography_amd import ops
    rng = np.random.default_rng(12)
    n = 12
    sig = np.linspace(4.0, 32.0, n)
    cube = (200.0 + rng.normal(0.0, 1.0, (n, 48, 64)) * sig[:, None, None]).astype(F)
    t = _dev(cube)
    ident = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * n
    rms = {}
    for weighting in (None, 'noise'):
        r = ops.coadd(t, ident, combine='WINSORIZED', sigma=3.0, maxiters=5, normalize='additive', weighting=weighting)
        rms[weighting] = float(r['image'][8:-8, 8:-8].double().std())
        if weighting == 'noise':
            assert np.abs(r['norm_weights'] * sig ** 2 / sig[0] ** 2 - 1.0).max() < 0.1
    print('rms equal weights %.3f, noise weights %.3f, ratio %.3f (bound %.3f)' % (rms[None], rms['noise'], rms['noise'] / rms[None], WEIGHT_RATIO))
    assert rms['noise'] <= WEIGHT_RATIO * rms[None]
