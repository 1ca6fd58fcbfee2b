"""The local normalisation inside the rejection rules (APGPU_STACK_FRAME_LOCAL) on the CPU: the NumPy model
(tests/stack_local_model.py), the scene the feature was added for, ops.local_normalization, the argument checks that need no
device, and the C ABI's checks of the flag and its descriptor."""
import ctypes as C

import numpy as np
import pytest

from tests import stack_frame_model as frame
from tests import stack_local_model as model
from tests.util import assert_biteq

F = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the map
def test_map_is_the_mesh_at_box_centres_and_held_beyond_the_outer_ones():
    """Odd boxes have a pixel at every centre (j + 0.5) b - 0.5.  Whole-number mesh values keep the lerp's arithmetic exact, so
    the last centre (t = 1: M0 + 1 * (M1 - M0)) is exact as well."""
    rng = np.random.default_rng(3)
    bh, bw, ny, nx = 5, 7, 3, 4
    M = rng.integers(-1000, 1000, (2, ny, nx)).astype(F)
    H, W = ny * bh + 9, nx * bw + 11                          # the mesh is smaller than the image: held beyond it
    m = model.local_map(M, (H, W), (bh, bw))
    assert m.dtype == F and m.shape == (2, H, W)
    cy, cx = np.arange(ny) * bh + bh // 2, np.arange(nx) * bw + bw // 2
    assert_biteq(m[:, cy][:, :, cx], M)
    assert_biteq(m[:, :cy[0] + 1][:, :, cx], np.broadcast_to(M[:, :1], (2, cy[0] + 1, nx)))
    assert_biteq(m[:, cy[-1]:][:, :, cx], np.broadcast_to(M[:, -1:], (2, H - cy[-1], nx)))
    assert_biteq(m[:, cy][:, :, :cx[0] + 1], np.broadcast_to(M[:, :, :1], (2, ny, cx[0] + 1)))
    assert_biteq(m[:, cy][:, :, cx[-1]:], np.broadcast_to(M[:, :, -1:], (2, ny, W - cx[-1])))
    assert_biteq(m[:, 0, 0], M[:, 0, 0])
    assert_biteq(m[:, -1, -1], M[:, -1, -1])
    # between two centres the values lie between the two cells', and a stripe is the whole image's rows
    lo, hi = np.minimum(M[:, 0, 0], M[:, 0, 1]), np.maximum(M[:, 0, 0], M[:, 0, 1])
    seg = m[:, cy[0], cx[0]:cx[1] + 1]
    assert (seg >= lo[:, None]).all() and (seg <= hi[:, None]).all()
    assert_biteq(model.local_map(M, (6, W), (bh, bw), row0=8), m[:, 8:14])
    # one cell on an axis: no interpolation along it; a box larger than the image: the cell's value everywhere
    assert_biteq(model.local_map(M[:, :1, :1], (H, W), (300, 400)), np.broadcast_to(M[:, :1, :1], (2, H, W)))
    j0, j1, t = model.axis_weights(10, 4, 1)
    assert (j0 == 0).all() and (j1 == 0).all()
    j0, j1, t = model.axis_weights(12, 4, 3)                  # even boxes: centres at 1.5, 5.5, 9.5
    assert j0.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1] and j1.tolist() == [1] * 6 + [2] * 6
    assert t.tolist() == [0, 0, 0.125, 0.375, 0.625, 0.875, 0.125, 0.375, 0.625, 0.875, 1, 1]


def test_map_agrees_with_float64():
    """The same formula in float64.  Every one of the three lerps rounds three times, and its t once, each on a magnitude of at
    most 2 max|M|: 3 * 4 * 2 = 24 units of 2^-24 max|M| bound the difference (the test prints what it finds)."""
    rng = np.random.default_rng(5)
    for (bh, bw), (ny, nx), (H, W) in (((16, 24), (3, 4), (37, 83)), ((3, 3), (7, 9), (20, 30)), ((256, 256), (2, 2), (300, 290))):
        M = rng.uniform(-500.0, 500.0, (3, ny, nx)).astype(F)
        got = model.local_map(M, (H, W), (bh, bw)).astype(np.float64)
        j0, j1, ty = model.axis_weights(H, bh, ny)
        k0, k1, tx = model.axis_weights(W, bw, nx)
        u = 2 * np.arange(H) + 1 - bh
        ty64 = np.clip(u - 2 * bh * j0, 0, 2 * bh) / (2.0 * bh)
        u = 2 * np.arange(W) + 1 - bw
        tx64 = np.clip(u - 2 * bw * k0, 0, 2 * bw) / (2.0 * bw)
        D = M.astype(np.float64)
        top = D[:, j0][:, :, k0] + tx64 * (D[:, j0][:, :, k1] - D[:, j0][:, :, k0])
        bot = D[:, j1][:, :, k0] + tx64 * (D[:, j1][:, :, k1] - D[:, j1][:, :, k0])
        want = top + ty64[:, None] * (bot - top)
        err = np.abs(got - want).max() / (2.0 ** -24 * np.abs(M).max())
        print('box %s mesh %s: %.2f units of 2^-24 max|M|' % ((bh, bw), (ny, nx), err))
        assert err <= 24.0


@pytest.mark.parametrize('method, rule', [('winsorized', dict(kl=2.5, kh=3.0, maxiters=None)), ('minmax', dict(nlow=1, nhigh=2))])
def test_constant_meshes_are_the_frame_parameters(method, rule):
    """A + t * (A - A) = A: a mesh that is constant per frame gives the bits of APGPU_STACK_FRAME_PARAMS with those scalars."""
    rng = np.random.default_rng(16)
    n, H, W = 9, 13, 21
    cube = rng.normal(500.0, 40.0, (n, H, W)).astype(F)
    cube[rng.random(cube.shape) < 0.1] += 700.0
    cube[rng.random(cube.shape) < 0.04] = np.nan
    a = rng.uniform(0.5, 2.0, n).astype(F)
    b = rng.uniform(-300.0, 300.0, n).astype(F)
    w = rng.uniform(0.05, 1.0, n).astype(F)
    want = frame.frame_params(cube, a, b, w, method, **rule)
    for ny, nx, box in ((1, 1, 4), (3, 4, (5, 6)), (2, 7, (16, 2))):
        A = np.broadcast_to(a[:, None, None], (n, ny, nx))
        B = np.broadcast_to(b[:, None, None], (n, ny, nx))
        got = model.local_params(cube, A, B, w, box, method, **rule)
        assert (got['keep'] == want['keep']).all()
        for k in ('mean_f64', 'std_f64', 'count'):
            assert_biteq(got[k], want[k], k)
    # no scale mesh = a mesh of ones
    B = rng.uniform(-300.0, 300.0, (n, 3, 4)).astype(F)
    g1 = model.local_params(cube, None, B, w, (5, 6), method, **rule)
    g2 = model.local_params(cube, np.ones((n, 3, 4), F), B, w, (5, 6), method, **rule)
    for k in ('mean_f64', 'std_f64', 'count'):
        assert_biteq(g1[k], g2[k], k)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the scene the feature was added for.  The figures of the issue's table, measured on these models (N: global | local):
#      trail values kept           8: 67 % | 0     10: 60 % | 0     16: 57 % | 0
#      error along the trail row   8: +20.7 | -0.19   10: +15.7 | -0.11   16: +9.9 | +0.01   ADU
#      rms error off the trail     8: 16.9 | 3.27     10: 16.3 | 2.95     16: 15.5 | 2.37    ADU (sigma / sqrt(N): 2.83, 2.53, 2.00)
#    with the meshes as local_normalization returns them by default (no median filter over the mesh).  With filter_size = 3 the
#    rms off the trail is 4.43, 4.15 and 3.68 ADU: the filter's windows are cut off at the mesh's rim, which pulls the rim cells
#    of a sloping mesh inwards by up to half a box of slope - see test_mesh_filter_pulls_the_rim_of_a_gradient_inwards.
@pytest.mark.parametrize('n', [8, 10, 16])
def test_scene_global_keeps_the_trail_and_local_removes_it(n):
    from astrophotography_amd import ops
    cube, stars, sky = model.gradient_scene(n)
    rule = dict(kl=3.0, kh=3.0, maxiters=5)
    st = np.array([frame.clipped_stats(f) for f in cube])
    a, b, w = ops.frame_normalization(st, 'additive', reference=0)
    g = model.scene_figures(frame.frame_params(cube, a, b, w, 'winsorized', **rule), cube.shape, stars)
    print('n = %d global: %r' % (n, g))
    assert g['trail_kept'] >= 0.5 and g['row_error'] >= 0.5 * 2 * model.TRAIL_ADU / n
    A, B, w = ops.local_normalization(model.box_stats(cube, 16), 'additive', reference=0, box=16)
    assert A is None and B.shape == (n, 6, 8) and B.dtype == F
    loc = model.scene_figures(model.local_params(cube, A, B, w, 16, 'winsorized', **rule), cube.shape, stars)
    print('n = %d local: %r' % (n, loc))
    assert loc['trail_kept'] == 0.0 and abs(loc['row_error']) <= 1.0
    assert loc['rms_off'] <= 1.5 * model.SCENE_NOISE / np.sqrt(n)


def test_mesh_filter_pulls_the_rim_of_a_gradient_inwards():
    """Why local_normalization does not filter by default: on a plane of 1 unit per cell the 3 x 3 nanmedian leaves the inner
    cells alone and moves every rim cell half a cell towards the middle."""
    from astrophotography_amd.mesh import nanmedian_filter
    plane = np.add.outer(np.zeros(5), np.arange(6.0))
    f = nanmedian_filter(plane, 3)
    assert np.array_equal(f[:, 1:-1], plane[:, 1:-1])
    assert (f[:, 0] == 0.5).all() and (f[:, -1] == 4.5).all()
    assert nanmedian_filter(plane, 1) is plane


# ---------------------------------------------------------------------------------------------------------------------------
# 3. ops.local_normalization on a hand-made 2 x 3 mesh
def _stats(L, S, cnt=None, masked=None):
    L = np.asarray(L, np.float64)
    st = np.zeros(L.shape + (4,))
    st[..., 0], st[..., 1] = L, S
    st[..., 2] = 100.0 if cnt is None else cnt
    st[..., 3] = 0.0 if masked is None else masked
    return st


def test_local_normalization_modes():
    from astrophotography_amd import ops
    L = np.array([[[100.0, 200.0, 400.0], [50.0, 80.0, 10.0]],
                  [[200.0, 100.0, 100.0], [25.0, 160.0, 40.0]],
                  [[110.0, 220.0, 440.0], [55.0, 88.0, 11.0]]])
    S = np.array([[[8.0, 8.0, 4.0], [2.0, 16.0, 1.0]],
                  [[4.0, 16.0, 4.0], [2.0, 4.0, 0.5]],
                  [[8.0, 8.0, 4.0], [2.0, 16.0, 1.0]]])
    st = _stats(L, S)
    A, B, w = ops.local_normalization(st, 'additive', box=10)
    assert A is None and B.dtype == F and w.dtype == np.float64 and w.tolist() == [1, 1, 1]
    assert B.tolist() == [[[0, 0, 0], [0, 0, 0]], [[-100, 100, 300], [25, -80, -30]], [[-10, -20, -40], [-5, -8, -1]]]
    A, B, w = ops.local_normalization(st, 'multiplicative', reference=1, box=10)
    assert A.dtype == F and A[1].tolist() == [[1, 1, 1], [1, 1, 1]] and not B.any()
    assert A[0].tolist() == [[2, 0.5, 0.25], [0.5, 2, 4]]
    assert_biteq(A[2], (L[1] / L[2]).astype(F))
    A, B, w = ops.local_normalization(st, 'additive+scaling', box=10)
    assert A[1].tolist() == [[2, 0.5, 1], [1, 4, 2]] and A[2].tolist() == [[1, 1, 1], [1, 1, 1]]
    assert B[1].tolist() == [[-300, 150, 300], [25, -560, -70]]
    assert_biteq(B[2], (L[0] - L[2]).astype(F))
    assert A[0].tolist() == [[1, 1, 1], [1, 1, 1]] and not B[0].any()           # the reference: exactly (1, 0)
    A, B, w = ops.local_normalization(st, 'none', box=10)
    assert A is None and not B.any() and w.tolist() == [1, 1, 1]
    # the weights: 1 / (median over the boxes of a S)^2, divided by the largest
    A, B, w = ops.local_normalization(st, 'additive', weighting='noise', box=10)
    med = np.array([np.median(S[i]) for i in range(3)])                       # 6, 4, 6
    assert med.tolist() == [6, 4, 6] and w[1] == 1.0 and np.allclose(w, [(4 / 6) ** 2, 1.0, (4 / 6) ** 2], rtol=1e-15, atol=0)
    A, B, w = ops.local_normalization(st, 'additive+scaling', weighting='noise', box=10)
    assert w.tolist() == [1, 1, 1]                                             # a_i S_i = S_r in every box
    # the mesh filter on request: the 3 x 3 nanmedian of the meshes above
    from astrophotography_amd.mesh import nanmedian_filter
    A1, B1, _ = ops.local_normalization(st, 'additive', box=10)
    A3, B3, _ = ops.local_normalization(st, 'additive', filter_size=3, box=10)
    assert_biteq(B3[1], nanmedian_filter(B1[1].astype(np.float64), 3).astype(F))
    assert not B3[0].any()
    for bad, match in ((dict(mode='best'), 'normalize'), (dict(mode='additive', weighting='snr'), 'weighting'),
                       (dict(mode='additive', reference=3), 'reference'), (dict(mode='additive', min_fraction=1.5), 'min_fraction')):
        with pytest.raises(ValueError, match=match):
            ops.local_normalization(st, box=10, **bad)
    with pytest.raises(ValueError, match='stats must be'):
        ops.local_normalization(st[..., :2], 'additive')


def test_local_normalization_fills_unusable_boxes():
    from astrophotography_amd import ops
    from astrophotography_amd.mesh import fill_excluded
    L = np.array([[[100.0, 200.0, 400.0], [50.0, 80.0, 10.0]], [[200.0, 100.0, 100.0], [25.0, 160.0, 40.0]]])
    S = np.full(L.shape, 4.0)
    cnt = np.full(L.shape, 100.0)
    cnt[1, 0, 2] = 49.0                                       # under half of the 10 x 10 box: a partial box, a resampling hole
    cnt[0, 1, 0] = 0.0                                        # the reference's box: unusable for every frame
    L[0, 1, 0] = np.nan
    st = _stats(L, S, cnt, 100.0 - cnt)
    A, B, w = ops.local_normalization(st, 'additive', box=10)
    good = np.array([[True, True, False], [False, True, True]])
    raw = np.where(good, L[0] - L[1], np.nan)
    assert_biteq(B[1], fill_excluded(raw, good).astype(F))
    assert B[1, 0, 0] == -100 and np.isfinite(B).all() and not B[0].any()
    # the box area is the FULL box: with box = 7 (area 49) the 49 survivors are enough; min_fraction moves the bar
    _, B7, _ = ops.local_normalization(st, 'additive', box=7)
    assert B7[1, 0, 2] == 300
    _, Bq, _ = ops.local_normalization(st, 'additive', box=10, min_fraction=0.375)
    assert Bq[1, 0, 2] == 300
    # without box: the largest survivors + masked count stands in for the area
    _, Bn, _ = ops.local_normalization(st, 'additive')
    assert_biteq(Bn, B)
    # the scaling modes also want S > 0, multiplicative L > 0 - in the frame and in the reference
    S2 = S.copy()
    S2[1, 0, 1] = 0.0
    A, B, w = ops.local_normalization(_stats(np.nan_to_num(L, nan=50.0), S2), 'additive+scaling', box=10)
    good = np.ones((2, 3), bool)
    good[0, 1] = False
    assert_biteq(A[1], fill_excluded(np.where(good, 1.0, np.nan), good).astype(F))
    L2 = np.nan_to_num(L, nan=50.0)
    L2[0, 1, 1] = -1.0
    A, B, w = ops.local_normalization(_stats(L2, S), 'multiplicative', box=10)
    good = np.ones((2, 3), bool)
    good[1, 1] = False
    assert_biteq(A[1], fill_excluded(np.where(good, L2[0] / L2[1], np.nan), good).astype(F))
    # a frame without one usable box is named
    cnt2 = np.full(L.shape, 100.0)
    cnt2[1] = 10.0
    with pytest.raises(ValueError, match='frame 1 has no usable box'):
        ops.local_normalization(_stats(L2, S, cnt2), 'additive', box=10)
    cnt2[1] = 100.0
    cnt2[0] = 0.0
    with pytest.raises(ValueError, match='frame 0 has no usable box'):
        ops.local_normalization(_stats(L2, S, cnt2), 'additive', box=10)
    with pytest.raises(ValueError, match='not finite as float32'):
        ops.local_normalization(_stats(L2 * np.array([1e39, 1.0])[:, None, None], S), 'additive', box=10)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. argument checks that need no device
def test_ops_argument_errors():
    import torch
    from astrophotography_amd import ops
    from astrophotography_amd.core.ApResample import ApResample
    from astrophotography_amd.core.ApStack import ApStack
    from astrophotography_amd.scripts import ap_coadd
    x = torch.zeros((4, 8, 8))
    B = np.zeros((4, 2, 2))
    for kw, match in ((dict(offset=B, box=0), 'box must be'), (dict(offset=B, box=(4, 40000)), 'box must be'),
                      (dict(offset=B, box=2.5), 'box must be'), (dict(box=4), 'offset is a mesh'),
                      (dict(offset=B[:3], box=4), 'offset must be a mesh'), (dict(offset=np.zeros(4), box=4), 'offset must be a mesh'),
                      (dict(offset=B, scale=np.ones((4, 2, 3)), box=4), 'scale must be a mesh'),
                      (dict(offset=B + np.inf, box=4), 'offset must be finite'), (dict(offset=B, scale=B + 1e39, box=4), 'scale must be finite'),
                      (dict(offset=B, weights=[1, 1, 1], box=4), 'one value per frame'), (dict(offset=B, weights=[1, 0, 1, 1], box=4), 'weights must be > 0'),
                      (dict(offset=B, weights=[1, np.nan, 1, 1], box=4), 'weights must be finite'), (dict(offset=B, box=4, row0=-1), 'row0'),
                      (dict(offset=B, box=4, calib=dict()), 'calib')):
        with pytest.raises(ValueError, match=match):
            ops.stack_reject(x, **kw)
    with pytest.raises(ValueError, match=r'frames must be \[N, H, W\]'):
        ops.stack_reject(x.reshape(4, 64), offset=B, box=4)
    loc = ops._frame_local(x, None, B + 2, [1, 2, 3, 4], (4, 6), 0, None)
    assert loc['box'] == (4, 6) and loc['scale'] is None and loc['offset'].dtype == F and loc['weight'].tolist() == [1, 2, 3, 4]
    for combine in ('MEDIAN', 'AVERAGE', 'CLIPPED', 'WEIGHTED', 'SUM'):
        with pytest.raises(ValueError, match='norm_box .* WINSORIZED and MINMAX only'):
            ops.coadd(x, None, combine=combine, normalize='additive', norm_box=16)
        with pytest.raises(ValueError, match='norm_box goes with combine WINSORIZED and MINMAX only'):
            ApResample(loglevel='ERROR', combine=combine, normalize='additive', norm_box=16)
    with pytest.raises(ValueError, match='fused'):
        ops.coadd(x, None, combine='WINSORIZED', norm_box=16, fused=True)
    with pytest.raises(ValueError, match='norm_box'):
        ApResample(loglevel='ERROR', combine='WINSORIZED', norm_box=0)
    rs = ApResample(loglevel='ERROR', combine='MINMAX', normalize='additive', norm_box=256)
    assert rs.norm_box == 256 and ApResample(loglevel='ERROR').norm_box is None
    with pytest.raises(ValueError, match='norm_box'):
        ApStack(loglevel='ERROR').stack(x, method='sigclip', norm_box=16)
    with pytest.raises(ValueError, match='fused calibration'):
        ApStack(loglevel='ERROR').stack(x, method='winsorized', normalize='additive', norm_box=16, calib=dict())
    p = ap_coadd.command_line_opts(['out.fits', 'a.fits', 'b.fits'])
    assert p.norm_box is None
    p = ap_coadd.command_line_opts(['out.fits', 'a.fits', 'b.fits', '--combine', 'WINSORIZED', '--normalize', 'additive', '--norm_box', '256'])
    assert p.norm_box == 256
    with pytest.raises(SystemExit):
        ap_coadd.command_line_opts(['out.fits', 'a.fits', '--norm_box', 'big'])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the C ABI: the flag's rules and the descriptor are checked on the host, before any device work
def _args(flags, n_frames=10, **kw):
    from astrophotography_amd._lib import StackArgs
    a = StackArgs()
    a.frames = 0x1000                                         # placeholders: never dereferenced by a call that fails its checks
    a.dtype, a.n_frames, a.n_pixels, a.frame_stride = 0, n_frames, 4096, 4096
    a.center, a.dev, a.maxiters = 0, 0, 5
    a.sigma_lower = a.sigma_upper = 3.0
    a.mean = 0x1000
    a.flags = flags
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _desc(**kw):
    from astrophotography_amd._lib import StackLocal
    d = StackLocal()
    d.width, d.row0, d.box_height, d.box_width, d.ny, d.nx = 64, 0, 16, 16, 4, 4
    d.scale, d.offset, d.weight = None, 0x1000, None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _with(a, d, nbytes=None):
    a.workspace = C.addressof(d)
    a.workspace_bytes = C.sizeof(d) if nbytes is None else nbytes
    return a


def test_capi_checks_of_the_flag_and_the_descriptor():
    import os
    from astrophotography_amd import _lib
    lib = _lib.load()
    W, M, FP, LOC = _lib.STACK_REJECT_WINSORIZED, _lib.STACK_REJECT_MINMAX, _lib.STACK_FRAME_PARAMS, _lib.STACK_FRAME_LOCAL
    assert LOC == 128 and lib.apgpu_version() == 130 and C.sizeof(_lib.StackArgs) == 192
    assert C.sizeof(_lib.StackLocal) == 56 and _lib.StackLocal.offset.offset == 40
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), 'include', 'apgpu.h')).read()
    assert '#define APGPU_STACK_FRAME_LOCAL 128\n' in hdr and '} apgpu_stack_local;' in hdr
    assert not any('stack_local' in name or 'frame_local' in name for name in _lib.SIGNATURES)               # the flag rides on apgpu_stack_sigclip
    buf = C.create_string_buffer(256)

    def rc(a, median_only=0):
        r = (lib.apgpu_stack_median if median_only else lib.apgpu_stack_sigclip)(C.byref(a), None)
        assert r != 0                                                           # (a good call would launch: not here)
        assert lib.apgpu_stack_kernel_name(C.byref(a), median_only, buf, 256) == r
        return r

    good = _desc()
    mm = dict(sigma_lower=1.0, sigma_upper=1.0)
    # without a rule, or through the other entry points: not served
    assert rc(_with(_args(LOC), good)) == _lib.E_UNSUPPORTED
    assert 'FRAME_LOCAL' in lib.apgpu_last_error().decode()
    assert rc(_with(_args(LOC | 1 | 2), good)) == _lib.E_UNSUPPORTED
    assert rc(_with(_args(LOC, mean=None, median=0x1000), good), 1) == _lib.E_UNSUPPORTED
    assert rc(_with(_args(LOC | W, mean=None, median=0x1000), good), 1) == _lib.E_UNSUPPORTED
    for flags in (LOC | W, LOC | M, LOC):
        a = _with(_args(flags, n_frames=4, n_pixels=64 * 64), good)
        r = lib.apgpu_resample_stack_sigclip(C.byref(a), 64, 64, None, 0x1000, 0, 0, None, 0x1000, 1024, 64, 64, None, 0, None)
        assert r == _lib.E_UNSUPPORTED
    # with a rule: the combinations
    assert rc(_with(_args(LOC | W | FP, exp_ratio=0x1000), good)) == _lib.E_INVAL
    assert 'exclude each other' in lib.apgpu_last_error().decode()
    assert rc(_with(_args(LOC | W | M), good)) == _lib.E_INVAL
    assert rc(_with(_args(LOC | W, bias=0x1000, dark=0x1000, exp_ratio=0x1000), good)) == _lib.E_INVAL
    for plane in ('bias', 'dark', 'nflat', 'pedestal', 'exp_ratio'):
        for flag, kw in ((W, {}), (M, mm)):
            assert rc(_with(_args(LOC | flag, **{plane: 0x1000}, **kw), good)) == _lib.E_INVAL, plane
    # the descriptor's place and size
    assert rc(_args(LOC | W)) == _lib.E_INVAL                                   # workspace NULL
    assert 'apgpu_stack_local' in lib.apgpu_last_error().decode()
    for nbytes in (0, 55, 57, 64):
        assert rc(_with(_args(LOC | M, **mm), good, nbytes)) == _lib.E_INVAL
    # its contents
    for bad in (dict(width=0), dict(width=-64), dict(width=100), dict(width=8192), dict(row0=-1), dict(row0=1 << 30), dict(width=1 << 30),
                dict(box_height=0), dict(box_height=32769), dict(box_width=0), dict(box_width=32769), dict(box_width=-1),
                dict(ny=0), dict(nx=0), dict(ny=-3), dict(ny=1 << 16, nx=1 << 15), dict(offset=None)):
        d = _desc(**bad)
        assert rc(_with(_args(LOC | W), d)) == _lib.E_INVAL, bad
        assert rc(_with(_args(LOC | M, **mm), d)) == _lib.E_INVAL, bad
    # and what is in order, by the name of the kernel it would launch (nothing is launched)
    for d in (good, _desc(width=4096), _desc(width=1), _desc(row0=1000), _desc(box_height=32768, box_width=1, ny=1, nx=9),
              _desc(scale=0x1000, weight=0x1000), _desc(ny=1, nx=1)):
        a = _with(_args(LOC | W), d)
        assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0, lib.apgpu_last_error()
    # the no-effect bits stay without effect
    a = _with(_args(LOC | W | 1 | 2 | 4), good)
    assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0


def test_capi_names_the_local_kernels():
    from astrophotography_amd import _lib
    lib = _lib.load()
    W, M, FP, LOC = _lib.STACK_REJECT_WINSORIZED, _lib.STACK_REJECT_MINMAX, _lib.STACK_FRAME_PARAMS, _lib.STACK_FRAME_LOCAL
    buf = C.create_string_buffer(256)
    d = _desc()
    names = set()
    for dtype, tname in ((0, 'float'), (1, 'unsigned short')):
        for n, slots in ((1, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64), (65, 128), (128, 128)):
            for flag, kw in ((W, {}), (M, dict(sigma_lower=1.0, sigma_upper=1.0))):
                a = _with(_args(flag | LOC, n_frames=n, dtype=dtype, **kw), d)
                assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0, lib.apgpu_last_error()
                assert buf.value.decode() == 'stack_reject_kernel<%d, %s, false, false, true>' % (slots, tname)
                names.add(buf.value)
                a = _args(flag | FP, n_frames=n, dtype=dtype, exp_ratio=0x1000, **kw)     # the other instances: named as before
                assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0
                assert buf.value.decode() == 'stack_reject_kernel<%d, %s, false, true>' % (slots, tname)
                a = _args(flag, n_frames=n, dtype=dtype, **kw)
                assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0
                assert buf.value.decode() == 'stack_reject_kernel<%d, %s, false>' % (slots, tname)
    assert len(names) == 10
    a = _with(_args(W | LOC, n_frames=129), d)
    assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == _lib.E_UNSUPPORTED
