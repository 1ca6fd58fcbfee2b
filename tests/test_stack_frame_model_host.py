"""Frame normalisation and weights inside the rejection rules (APGPU_STACK_FRAME_PARAMS) on the CPU: the NumPy model
(tests/stack_frame_model.py), the normalisation formulas, the argument checks that need no device, and the experiment the
feature was added for."""
import ctypes as C

import numpy as np
import pytest

from tests import stack_frame_model as model
from tests import stack_reject_model as reject
from tests.util import assert_biteq

F = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the model against the definition's own words
@pytest.mark.parametrize('method', ['winsorized', 'minmax'])
def test_model_equals_one_dimensional_numpy(method):
    rng = np.random.default_rng(16)
    for n in range(1, 21):
        cols = 30
        cube = rng.normal(500.0, 40.0, (n, cols)).astype(F)
        cube[rng.random(cube.shape) < 0.12] += 700.0
        cube[rng.random(cube.shape) < 0.05] = np.nan
        if n > 3:
            cube[1, 0] = np.inf
            cube[:, 1] = np.nan                               # an empty column
            cube[2, 2] = cube[0, 2]                           # ties
        a = rng.uniform(0.5, 2.0, n).astype(F)
        b = rng.uniform(-300.0, 300.0, n).astype(F)
        w = rng.uniform(0.05, 1.0, n).astype(F)
        rule = dict(kl=2.5, kh=3.0, maxiters=None) if method == 'winsorized' else dict(nlow=1, nhigh=2)
        r = model.frame_params(cube, a, b, w, method, **rule)
        for c in range(cols):
            m, sd, cnt, keep = model.column_1d(cube[:, c], a, b, w, method, **rule)
            assert keep == r['keep'][:, c].tolist(), (n, c)
            assert cnt == r['count'][c]
            assert_biteq(np.array([m, sd]), np.array([r['mean_f64'][c], r['std_f64'][c]]), 'n = %d column %d' % (n, c))


@pytest.mark.parametrize('method, rule', [('winsorized', dict(kl=3.0, kh=3.0)), ('minmax', dict(nlow=1, nhigh=1))])
def test_all_ones_parameters_are_the_existing_rule(method, rule):
    rng = np.random.default_rng(4)
    for n in (1, 2, 3, 7, 8, 9, 20):
        cube = rng.normal(100.0, 10.0, (n, 200)).astype(F)
        cube[rng.random(cube.shape) < 0.1] += 300.0
        cube[rng.random(cube.shape) < 0.03] = np.nan
        r = model.frame_params(cube, np.ones(n), np.zeros(n), np.ones(n), method, **rule)
        e = getattr(reject, method)(cube, **rule)
        assert (r['keep'] == e['keep']).all() and (r['count'] == e['count']).all()
        assert_biteq(r['std_f64'], e['std_f64'])
        # the mean is the sequential sum, the existing model's is numpy's pairwise one: equal to rounding, not in bits
        np.testing.assert_allclose(r['mean_f64'], e['mean_f64'], rtol=1e-14, equal_nan=True)


def test_weights_decide_the_mean_and_nothing_else():
    cube = np.array([[10.0], [20.0], [30.0], [1000.0]], F)
    a, b = np.ones(4), np.zeros(4)
    r1 = model.frame_params(cube, a, b, [1, 1, 1, 1], 'winsorized')
    r2 = model.frame_params(cube, a, b, [1, 0.5, 0.25, 1], 'winsorized')
    assert r1['keep'][:, 0].tolist() == r2['keep'][:, 0].tolist() == [True, True, True, False]
    assert r1['mean_f64'][0] == 20.0 and r2['mean_f64'][0] == (10.0 + 10.0 + 7.5) / 1.75
    assert r1['std_f64'][0] == r2['std_f64'][0] and r1['count'][0] == r2['count'][0] == 3
    # the map can produce -0.0, which min/max sorts below +0.0 (frame 1 goes, not frame 0)
    r = model.frame_params(np.array([[0.0], [0.0], [5.0]], F), [1, -1, 1], [0.0, -0.0, 0.0], [1, 1, 1], 'minmax', nlow=1, nhigh=0)
    assert np.signbit(r['v'][1, 0]) and r['keep'][:, 0].tolist() == [True, False, True]
    # a value the map sends out of float32's range is not finite: not part of S
    r = model.frame_params(np.array([[3e38], [1.0], [2.0]], F), [2, 1, 1], [0, 0, 0], [1, 1, 1], 'minmax', nlow=0, nhigh=0)
    assert r['keep'][:, 0].tolist() == [False, True, True]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the normalisation formulas
def test_normalisation_formulas():
    from astrophotography_amd import ops
    st = np.array([[100.0, 8.0], [200.0, 16.0], [50.0, 4.0]])
    a, b, w = ops.frame_normalization(st, 'additive', reference=0)
    assert a.tolist() == [1, 1, 1] and b.tolist() == [0, -100, 50] and w.tolist() == [1, 1, 1]
    a, b, w = ops.frame_normalization(st, 'multiplicative', reference=1)
    assert a.tolist() == [2, 1, 4] and b.tolist() == [0, 0, 0]
    a, b, w = ops.frame_normalization(st, 'additive+scaling', reference=0, weighting='noise')
    assert a.tolist() == [1, 0.5, 2] and b.tolist() == [0, 0, 0] and w.tolist() == [1, 1, 1]       # all noise 8 afterwards
    a, b, w = ops.frame_normalization(st, 'additive', reference=2, weighting='noise')
    assert b.tolist() == [-50, -150, 0] and w.tolist() == [0.25, 0.0625, 1.0]
    a, b, w = ops.frame_normalization(st, 'none', weighting='noise')
    assert a.tolist() == [1, 1, 1] and b.tolist() == [0, 0, 0] and w.tolist() == [0.25, 0.0625, 1.0]
    assert all(x.dtype == np.float64 for x in (a, b, w))
    with pytest.raises(ValueError, match='normalize'):
        ops.frame_normalization(st, 'best')
    with pytest.raises(ValueError, match='weighting'):
        ops.frame_normalization(st, 'additive', weighting='snr')
    with pytest.raises(ValueError, match='reference'):
        ops.frame_normalization(st, 'additive', reference=3)
    with pytest.raises(ValueError, match='frame 1 .*L > 0'):
        ops.frame_normalization(np.array([[1.0, 1.0], [0.0, 1.0]]), 'multiplicative')
    with pytest.raises(ValueError, match='frame 1 has no finite pixel'):
        ops.frame_normalization(np.array([[1.0, 1.0], [np.nan, np.nan]]), 'additive')
    with pytest.raises(ValueError, match='frame 0 has scale S = 0'):
        ops.frame_normalization(np.array([[1.0, 0.0], [2.0, 1.0]]), 'additive+scaling')
    with pytest.raises(ValueError, match='frame 0 has scale S = 0'):
        ops.frame_normalization(np.array([[1.0, 0.0], [2.0, 1.0]]), 'additive', weighting='noise')
    a, b, w = ops.frame_normalization(np.array([[1.0, 0.0], [2.0, 1.0]]), 'additive')            # S is not needed here
    assert b.tolist() == [0, -1]


# ---------------------------------------------------------------------------------------------------------------------------
# 3. argument checks that need no device
def test_ops_argument_errors():
    import torch
    from astrophotography_amd import ops
    from astrophotography_amd.core.ApResample import ApResample
    from astrophotography_amd.core.ApStack import ApStack
    x = torch.zeros((4, 8, 8))
    with pytest.raises(ValueError, match='scale must hold one value per frame'):
        ops.stack_reject(x, scale=[1, 1, 1])
    with pytest.raises(ValueError, match='offset must be finite'):
        ops.stack_reject(x, offset=[0, 0, np.inf, 0])
    with pytest.raises(ValueError, match='scale must be finite'):
        ops.stack_reject(x, scale=[1, 1e39, 1, 1])                           # not finite as float32
    with pytest.raises(ValueError, match='weights must be > 0'):
        ops.stack_reject(x, weights=[1, 0, 1, 1])
    with pytest.raises(ValueError, match='weights must be > 0'):
        ops.stack_reject(x, weights=[1, 1e-60, 1, 1])                        # zero as float32
    with pytest.raises(ValueError, match='weights must be finite'):
        ops.stack_reject(x, weights=[1, np.nan, 1, 1])
    with pytest.raises(ValueError, match='calib'):
        ops.stack_reject(x, weights=[1, 1, 1, 1], calib=dict(bias=x[0], dark=x[0], exp_ratio=1.0))
    blk = ops._frame_params(x, None, [1, 2, 3, 4], None, None)
    assert blk.dtype == F and blk.tolist() == [[1, 1, 1, 1], [1, 2, 3, 4], [1, 1, 1, 1]]
    assert ops._frame_params(x, None, None, None, None) is None
    with pytest.raises(ValueError, match='normalize'):
        ops.coadd(x, None, combine='WINSORIZED', normalize='best')
    with pytest.raises(ValueError, match='weighting'):
        ops.coadd(x, None, combine='WINSORIZED', weighting='snr')
    for combine in ('MEDIAN', 'AVERAGE', 'CLIPPED', 'WEIGHTED', 'SUM'):
        with pytest.raises(ValueError, match='weighting goes with'):
            ops.coadd(x, None, combine=combine, normalize='additive', weighting='noise')
    with pytest.raises(ValueError, match='fused'):
        ops.coadd(x, None, combine='CLIPPED', normalize='additive', fused=True)
    with pytest.raises(ValueError, match='normalize'):
        ApResample(loglevel='ERROR', normalize='best')
    with pytest.raises(ValueError, match='weighting'):
        ApResample(loglevel='ERROR', combine='MEDIAN', weighting='noise')
    rs = ApResample(loglevel='ERROR', combine='WINSORIZED', normalize='additive+scaling', weighting='noise', reference='b.fits')
    assert (rs.normalize, rs.weighting) == ('additive+scaling', 'noise')
    assert rs._reference_index(['/x/a.fits', '/x/b.fits']) == 1
    with pytest.raises(RuntimeError, match='reference'):
        rs._reference_index(['/x/a.fits', '/x/c.fits'])
    with pytest.raises(ValueError, match='normalize / weighting'):
        ApStack(loglevel='ERROR').stack(x, method='sigclip', normalize='additive')
    with pytest.raises(ValueError, match='fused calibration'):
        ApStack(loglevel='ERROR').stack(x, method='winsorized', normalize='additive', calib=dict())


def test_ap_coadd_options():
    from astrophotography_amd.scripts import ap_coadd
    p = ap_coadd.command_line_opts(['out.fits', 'a.fits', 'b.fits'])
    assert (p.normalize, p.reference, p.weighting) == ('none', '0', 'none')
    p = ap_coadd.command_line_opts(['out.fits', 'a.fits', 'b.fits', '--combine', 'WINSORIZED', '--normalize', 'additive+scaling',
                                    '--reference', 'b.fits', '--weighting', 'noise'])
    assert (p.normalize, p.reference, p.weighting) == ('additive+scaling', 'b.fits', 'noise')
    with pytest.raises(SystemExit):
        ap_coadd.command_line_opts(['out.fits', 'a.fits', '--normalize', 'best'])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the C ABI: the flag's rules are checked before any device work
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


def test_capi_checks_of_the_flag():
    import os
    from astrophotography_amd import _lib
    lib = _lib.load()
    W, M, FP = _lib.STACK_REJECT_WINSORIZED, _lib.STACK_REJECT_MINMAX, _lib.STACK_FRAME_PARAMS
    assert FP == 64 and lib.apgpu_version() == 130 and C.sizeof(_lib.StackArgs) == 192
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), 'include', 'apgpu.h')).read()
    assert '#define APGPU_STACK_FRAME_PARAMS 64\n' in hdr
    buf = C.create_string_buffer(256)

    def rc(a, median_only=0):
        r = (lib.apgpu_stack_median if median_only else lib.apgpu_stack_sigclip)(C.byref(a), None)
        assert lib.apgpu_stack_kernel_name(C.byref(a), median_only, buf, 256) == r
        return r

    assert rc(_args(FP, exp_ratio=0x1000)) == _lib.E_UNSUPPORTED                     # no rule: the other kernels do not serve it
    assert rc(_args(FP | 1 | 2, exp_ratio=0x1000)) == _lib.E_UNSUPPORTED
    assert rc(_args(FP, exp_ratio=0x1000, mean=None, median=0x1000), 1) == _lib.E_UNSUPPORTED
    assert rc(_args(FP | W, exp_ratio=0x1000, mean=None, median=0x1000), 1) == _lib.E_UNSUPPORTED
    assert rc(_args(FP | W | M, exp_ratio=0x1000)) == _lib.E_INVAL
    assert rc(_args(FP | W)) == _lib.E_INVAL                                          # exp_ratio NULL
    assert rc(_args(FP | M, sigma_lower=1.0, sigma_upper=1.0)) == _lib.E_INVAL
    assert rc(_args(FP | W, exp_ratio=0x1000, bias=0x1000, dark=0x1000)) == _lib.E_INVAL
    for plane in ('dark', 'nflat', 'pedestal'):
        assert rc(_args(FP | W, exp_ratio=0x1000, **{plane: 0x1000})) == _lib.E_INVAL
        assert 'FRAME_PARAMS' in lib.apgpu_last_error().decode()
    a = _args(FP | W, n_frames=4, n_pixels=64 * 64, exp_ratio=0x1000)
    r = lib.apgpu_resample_stack_sigclip(C.byref(a), 64, 64, None, 0x1000, 0, 0, None, 0x1000, 1024, 64, 64, None, 0, None)
    assert r == _lib.E_UNSUPPORTED
    a = _args(FP, n_frames=4, n_pixels=64 * 64, exp_ratio=0x1000)
    r = lib.apgpu_resample_stack_sigclip(C.byref(a), 64, 64, None, 0x1000, 0, 0, None, 0x1000, 1024, 64, 64, None, 0, None)
    assert r == _lib.E_UNSUPPORTED


def test_capi_names_the_frame_kernels():
    from astrophotography_amd import _lib
    lib = _lib.load()
    W, M, FP = _lib.STACK_REJECT_WINSORIZED, _lib.STACK_REJECT_MINMAX, _lib.STACK_FRAME_PARAMS
    buf = C.create_string_buffer(256)
    names = set()
    for dtype, tname in ((0, 'float'), (1, 'unsigned short')):
        for n, slots in ((1, 8), (8, 8), (9, 16), (16, 16), (17, 32), (33, 64), (64, 64), (65, 128), (128, 128)):
            for flag, kw in ((W, {}), (M, dict(sigma_lower=1.0, sigma_upper=1.0))):
                a = _args(flag | FP, n_frames=n, dtype=dtype, exp_ratio=0x1000, **kw)
                assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0, lib.apgpu_last_error()
                assert buf.value.decode() == 'stack_reject_kernel<%d, %s, false, true>' % (slots, tname)
                names.add(buf.value)
                a = _args(flag, n_frames=n, dtype=dtype, **kw)                # without the bit: the name as it was
                assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0
                assert buf.value.decode() == 'stack_reject_kernel<%d, %s, false>' % (slots, tname)
    assert len(names) == 10


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the experiment the feature was added for
@pytest.mark.parametrize('n', [8, 10, 16])
def test_trail_survives_unequal_sky_and_goes_after_additive_normalisation(n):
    from astrophotography_amd import ops
    cube, stars, sky = model.trail_scene(n, seed=20261019 + n)
    row, tf = model.TRAIL_ROW, list(model.TRAIL_FRAMES)
    ones, zeros = np.ones(n), np.zeros(n)
    r = model.frame_params(cube, ones, zeros, ones, 'winsorized', kl=3.0, kh=3.0, maxiters=5)
    assert r['keep'][tf, row].all(), 'without normalisation the rule removed a trail value'
    err = (r['mean_f64'][row] - (stars[row] + sky.mean())).mean()
    print('n = %d, none: trail row mean error %.1f ADU' % (n, err))
    assert err > 0.5 * 2 * model.TRAIL_ADU / n                # the trail is in the co-add (2 of n frames carry 120 ADU)
    st = np.array([model.clipped_stats(f) for f in cube])
    a, b, w = ops.frame_normalization(st, 'additive', reference=0)
    r = model.frame_params(cube, a, b, w, 'winsorized', kl=3.0, kh=3.0, maxiters=5)
    assert not r['keep'][tf, row].any(), 'after additive normalisation the rule kept a trail value'
    err = (r['mean_f64'][row] - (stars[row] + sky[0])).mean()
    good = np.ones(cube.shape, bool)
    good[tf, row] = False
    lost = (~r['keep'] & good).sum() / good.sum()
    print('n = %d, additive: trail row mean error %.2f ADU, good values lost %.4f' % (n, err, lost))
    assert abs(err) < 3 * model.SCENE_NOISE / np.sqrt(n - 2) and lost < 0.03


def test_noise_weights_lower_the_rms():
    """12 frames, equal sky, noise sigma 4 .. 32: inverse-variance weights against equal ones, on the model."""
    from astrophotography_amd import ops
    rng = np.random.default_rng(12)
    n = 12
    sig = np.linspace(4.0, 32.0, n)
    cube = (200.0 + rng.normal(0.0, 1.0, (n, 48, 64)) * sig[:, None, None]).astype(F)
    st = np.array([model.clipped_stats(f) for f in cube])
    rms = {}
    for weighting in (None, 'noise'):
        a, b, w = ops.frame_normalization(st, 'additive', reference=0, weighting=weighting)
        r = model.frame_params(cube, a, b, w, 'winsorized', kl=3.0, kh=3.0, maxiters=5)
        rms[weighting] = np.std(r['mean_f64'])
    print('rms equal weights %.3f, noise weights %.3f, ratio %.3f' % (rms[None], rms['noise'], rms['noise'] / rms[None]))
    # theory for a plain weighted mean: sqrt(1 / sum(1 / s^2)) against sqrt(sum s^2) / n
    theory = np.sqrt(1.0 / np.sum(1.0 / sig ** 2)) / (np.sqrt(np.sum(sig ** 2)) / n)
    print('theory %.3f' % theory)
    assert rms['noise'] < 0.85 * rms[None]
