"""The generalized ESD rejection rule without a GPU: its NumPy restatement (tests/stack_esd_model.py) against itself, against the
min/max rule it ends in and against Rosner's worked example; the table of critical values (ops.esd_lambda) against SciPy; the C
ABI's argument checks through the library loaded on the CPU (it validates before any device work); and what the rule is for, on
the ten-frame trail of tests/test_gpu_stack_reject.py."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import stack_esd_model as model
from tests import stack_reject_model as reject
from tests.util import assert_biteq

F = np.float32
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'g19_esd_lambda.npz')
ALPHAS = (0.05, 0.01, 0.001)

# Rosner (1983), the 54 values of the NIST/SEMATECH e-Handbook of Statistical Methods, section 1.3.5.17.3
ROSNER = [-0.25, 0.68, 0.94, 1.15, 1.20, 1.26, 1.26, 1.34, 1.38, 1.43, 1.49, 1.49, 1.55, 1.56, 1.58, 1.65, 1.69, 1.70, 1.76, 1.77,
          1.81, 1.91, 1.94, 1.96, 1.99, 2.06, 2.09, 2.10, 2.14, 2.15, 2.23, 2.24, 2.26, 2.35, 2.37, 2.40, 2.47, 2.54, 2.62, 2.64,
          2.90, 2.92, 2.92, 2.93, 3.21, 3.26, 3.30, 3.59, 3.68, 4.30, 4.64, 5.34, 5.42, 6.01]
ROSNER_R = [3.119, 2.943, 3.179, 2.810, 2.816, 2.848, 2.279, 2.310, 2.102, 2.067]
ROSNER_LAMBDA = [3.159, 3.151, 3.144, 3.136, 3.128, 3.120, 3.112, 3.103, 3.094, 3.085]


def _random_cube(rng, N, P, ties=True):
    """Noise with outliers at both ends, NaNs, and (ties) columns from a small pool of values with zeros of both signs."""
    cube = rng.normal(100.0, 5.0, (N, P)).astype(F)
    cube[rng.random((N, P)) < 0.06] += F(60.0)
    cube[rng.random((N, P)) < 0.03] -= F(80.0)
    if ties:
        pool = np.array([99.0, 100.0, 100.0, 101.0, 160.0, 20.0, -0.0, 0.0], F)
        cube[:, : P // 3] = rng.choice(pool, (N, P // 3))
    cube[rng.random((N, P)) < 0.05] = np.nan
    cube[:, -1] = np.nan
    cube[1:, -2] = np.inf
    return cube


@pytest.mark.parametrize('N', [3, 4, 7, 10, 24, 40])
def test_the_two_forms_agree_bit_for_bit_and_end_in_minmax(N):
    from astrophotography_amd import ops
    rng = np.random.default_rng(N)
    cube = _random_cube(rng, N, 240)
    pm = (rng.random(240) < 0.05).astype(np.uint8)
    for frac, relax in ((0.3, 1.5), (0.5, 1.0), (0.1, 4.0)):
        lam = ops.esd_lambda(N, frac, 0.05)
        r = model.esd(cube, lam, frac, relax, pixmask=pm)
        for p in range(cube.shape[1]):
            c = model.column_1d(cube[:, p], lam, frac, relax)
            if pm[p]:
                assert r['count'][p] == 0 and np.isnan(r['mean_f64'][p])
                continue
            assert (r['L'][p], r['H'][p], r['count'][p]) == (c['L'], c['H'], c['count']), p
            assert list(r['keep'][:, p]) == c['keep'], p
            assert_biteq(np.array([r['mean_f64'][p], r['std_f64'][p]]), np.array([c['mean_f64'], c['std_f64']]), 'column %d' % p)
        # the survivors are min/max's with that pixel's (L, H): keep, and with it every output
        for L, H in set(zip(r['L'].tolist(), r['H'].tolist())):
            sel = (r['L'] == L) & (r['H'] == H)
            m = reject.minmax(cube[:, sel], L, H, pixmask=pm[sel])
            assert (m['keep'] == r['keep'][:, sel]).all()
            for k in ('count', 'mean_f64', 'std_f64'):
                assert_biteq(r[k][sel], m[k], '(%d, %d) %s' % (L, H, k))


def test_nothing_to_remove_is_minmax_0_0():
    from astrophotography_amd import ops
    rng = np.random.default_rng(3)
    for N, frac in ((10, 0.0), (3, 0.5), (2, 0.5), (1, 0.5), (10, 0.05), (6, 0.5)):
        cube = _random_cube(rng, N, 100)
        if N == 6:                                           # three finite values at most: n - 3 <= 0
            cube[3:] = np.nan
        r = model.esd(cube, ops.esd_lambda(N, frac, 0.05), frac, 1.5)
        m = reject.minmax(cube, 0, 0)
        assert (r['L'] == 0).all() and (r['H'] == 0).all() and (r['steps'] == 0).all()
        for k in ('count', 'mean_f64', 'std_f64', 'keep'):
            assert_biteq(r[k], m[k], '%d frames frac %g: %s' % (N, frac, k))


def test_rosner_example():
    from astrophotography_amd import ops
    rng = np.random.default_rng(54)
    col = np.array(ROSNER, F)[rng.permutation(54)]
    lam = ops.esd_lambda(54, 10 / 54 + 1e-6, 0.05)
    assert lam.shape == (55, 10)
    assert np.abs(lam[54] - ROSNER_LAMBDA).max() <= 6e-4, lam[54]
    c = model.column_1d(col, lam, 10 / 54 + 1e-6, 1.0)
    assert len(c['R']) == 10
    assert np.abs(np.array(c['R']) - ROSNER_R).max() <= 6e-4, c['R']
    assert (c['L'], c['H'], c['count']) == (0, 3, 51)
    assert sorted(col[~np.array(c['keep'])].tolist()) == [F(5.34), F(5.42), F(6.01)]
    r = model.esd(col[:, None], lam, 10 / 54 + 1e-6, 1.0)
    assert (int(r['L'][0]), int(r['H'][0]), int(r['steps'][0])) == (0, 3, 10)
    assert abs(r['R'][0] - 3.179) <= 6e-4


def _scipy_lambda(n, frac, alpha, maxout):
    """The table from scipy.stats.t.ppf.  tests/golden/g19_esd_lambda.npz holds _scipy_lambda(128, 0.5, alpha, 64) for the three
    ALPHAS under the keys 'alpha_<alpha>' (np.savez_compressed), recorded with SciPy 1.15.3."""
    from scipy import stats
    lam = np.full((n + 1, maxout), np.inf)
    for k in range(4, n + 1):
        for i in range(min(int(np.floor(frac * k)), k - 3, maxout)):
            m = k - i
            t = stats.t.ppf(1 - alpha / (2 * m), m - 2)
            lam[k, i] = (m - 1) * t / np.sqrt((m - 2 + t * t) * m)
    return lam


# The largest relative difference between ops.esd_lambda and the same formula on scipy.stats.t.ppf (SciPy 1.15.3), n = 4 .. 128 and the
# three levels, measured where the table under tests/golden was recorded: 1.7e-11 - SciPy is handed p = 1 - alpha / (2 m), which has
# lost eleven digits of alpha / (2 m) by then; esd_lambda solves for the upper tail itself.  The bound is 16 times that (< 1e-9).
LAMBDA_MEASURED = 1.7e-11
LAMBDA_BOUND = min(16 * LAMBDA_MEASURED, 1e-9)


def test_lambda_table_against_scipy():
    from astrophotography_amd import ops
    gold = np.load(GOLDEN)
    worst = 0.0
    for alpha in ALPHAS:
        lam = ops.esd_lambda(128, 0.5, alpha)
        assert lam.shape == (129, 64) and lam.dtype == np.float64
        ref = gold['alpha_%g' % alpha]
        assert (np.isinf(lam) == np.isinf(ref)).all() and np.isinf(lam[:4]).all() and not np.isnan(lam).any()
        fin = np.isfinite(ref)
        worst = max(worst, np.abs(lam[fin] / ref[fin] - 1).max())
        try:
            import scipy  # noqa: F401
        except ImportError:
            continue
        live = _scipy_lambda(128, 0.5, alpha, 64)
        worst = max(worst, np.abs(lam[fin] / live[fin] - 1).max())
    print('esd_lambda against SciPy: largest relative difference %.3g (bound %.3g)' % (worst, LAMBDA_BOUND))
    assert worst <= LAMBDA_BOUND
    # the shape of the table: K_n entries per row, +inf behind them; a smaller max_outliers cuts the rows short
    lam = ops.esd_lambda(24, 0.3, 0.05)
    assert lam.shape == (25, 7) and np.isfinite(lam[24]).all() and np.isfinite(lam[10, :3]).all() and np.isinf(lam[10, 3:]).all()
    assert np.isfinite(lam[4, :1]).all() and np.isinf(lam[4, 1:]).all() and np.isinf(lam[3]).all()
    cut = ops.esd_lambda(24, 0.3, 0.05, max_outliers=2)
    assert_biteq(cut, lam[:, :2])
    assert np.isinf(ops.esd_lambda(10, 0.0, 0.05)).all() and ops.esd_lambda(10, 0.0, 0.05).shape == (11, 1)
    for bad in (dict(frac=0.6), dict(frac=-0.1), dict(alpha=0.0), dict(alpha=1.0), dict(max_outliers=65), dict(max_outliers=0)):
        with pytest.raises(ValueError):
            ops.esd_lambda(10, **bad)


# ---------------------------------------------------------------------------------------------------------------------------
# the C ABI: the flag's rules and the descriptor are checked on the host, before any device work
def _args(flags, n_frames=10, **kw):
    from astrophotography_amd._lib import StackArgs
    a = StackArgs()
    a.frames = 0x1000                                         # placeholders: never dereferenced by a call that fails its checks
    a.dtype, a.n_frames, a.n_pixels, a.frame_stride = 0, n_frames, 4096, 4096
    a.center, a.dev, a.maxiters = 0, 0, 5
    a.sigma_lower, a.sigma_upper = 0.3, 1.5
    a.mean = 0x1000
    a.flags = flags
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _esd(**kw):
    from astrophotography_amd._lib import StackEsd
    e = StackEsd()
    e.lambda_, e.max_outliers, e.reserved, e.local = 0x1000, 3, 0, None
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _local(**kw):
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
    from astrophotography_amd import _lib
    lib = _lib.load()
    W, M, E, FP, LOC = (_lib.STACK_REJECT_WINSORIZED, _lib.STACK_REJECT_MINMAX, _lib.STACK_REJECT_ESD, _lib.STACK_FRAME_PARAMS,
                        _lib.STACK_FRAME_LOCAL)
    assert E == 256 and lib.apgpu_version() == 130 and C.sizeof(_lib.StackArgs) == 192
    assert C.sizeof(_lib.StackEsd) == 24 and _lib.StackEsd.local.offset == 16
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), 'include', 'apgpu.h')).read()
    assert '#define APGPU_STACK_REJECT_ESD 256\n' in hdr and '} apgpu_stack_esd;' in hdr
    assert not any('esd' in name for name in _lib.SIGNATURES)                  # the rule rides on apgpu_stack_sigclip
    buf = C.create_string_buffer(256)

    def rc(a, median_only=0):
        r = (lib.apgpu_stack_median if median_only else lib.apgpu_stack_sigclip)(C.byref(a), None)
        assert r != 0                                                           # (a good call would launch: not here)
        assert lib.apgpu_stack_kernel_name(C.byref(a), median_only, buf, 256) == r
        return r

    def ok(a):
        assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0, lib.apgpu_last_error()
        return buf.value.decode()

    good = _esd()
    assert ok(_with(_args(E), good)) == 'stack_esd_kernel<16, float, false>'
    # the other entry points do not serve it
    assert rc(_with(_args(E, mean=None, median=0x1000), good), 1) == _lib.E_UNSUPPORTED
    a = _with(_args(E, n_frames=4, n_pixels=64 * 64), good)
    assert lib.apgpu_resample_stack_sigclip(C.byref(a), 64, 64, None, 0x1000, 0, 0, None, 0x1000, 1024, 64, 64, None, 0, None) == _lib.E_UNSUPPORTED
    # one rule at a time
    for flags in (E | W, E | M, E | W | M):
        assert rc(_with(_args(flags), good)) == _lib.E_INVAL
        assert 'exclude each other' in lib.apgpu_last_error().decode()
    # what holds for the other two rules
    assert rc(_with(_args(E, moments=0x1000), good)) == _lib.E_UNSUPPORTED
    assert rc(_with(_args(E, median=0x1000), good)) == _lib.E_UNSUPPORTED
    assert rc(_with(_args(E, center=1), good)) == _lib.E_INVAL
    assert rc(_with(_args(E, dev=1), good)) == _lib.E_INVAL
    assert rc(_with(_args(E | _lib.STACK_NONFINITE_UNCLIPPED), good)) == _lib.E_INVAL
    assert rc(_with(_args(E | 512), good)) == _lib.E_INVAL
    assert rc(_with(_args(E, n_frames=129), good)) == _lib.E_UNSUPPORTED
    assert rc(_with(_args(E, mean=None), good)) == _lib.E_INVAL
    ok(_with(_args(E | 1 | 2 | 4), good))                                       # the no-effect bits
    ok(_with(_args(E, maxiters=0), good))                                       # maxiters is unused
    ok(_with(_args(E, dtype=1, bias=0x1000, dark=0x1000, exp_ratio=0x1000, pixmask=0x1000, frame_stride=8192), good))
    # frac and relax
    for lo, hi in ((-0.01, 1.5), (0.51, 1.5), (float('nan'), 1.5), (0.3, 0.99), (0.3, float('inf')), (0.3, float('nan')), (0.3, -2.0)):
        assert rc(_with(_args(E, sigma_lower=lo, sigma_upper=hi), good)) == _lib.E_INVAL, (lo, hi)
    for lo, hi in ((0.0, 1.0), (0.5, 1e300)):
        ok(_with(_args(E, sigma_lower=lo, sigma_upper=hi), good))
    # the descriptor's place, size and contents
    assert rc(_args(E)) == _lib.E_INVAL                                         # workspace NULL
    assert 'apgpu_stack_esd' in lib.apgpu_last_error().decode()
    for nbytes in (0, 23, 25, 56):
        assert rc(_with(_args(E), good, nbytes)) == _lib.E_INVAL
    for bad in (dict(lambda_=None), dict(max_outliers=0), dict(max_outliers=65), dict(max_outliers=-1), dict(reserved=1)):
        assert rc(_with(_args(E), _esd(**bad))) == _lib.E_INVAL, bad
    for mo in (1, 64):
        ok(_with(_args(E), _esd(max_outliers=mo)))
    # the frame parameters and the local meshes combine with it; the mesh descriptor is the ESD descriptor's `local`
    assert ok(_with(_args(E | FP, exp_ratio=0x1000), good)) == 'stack_esd_kernel<16, float, false, true>'
    assert rc(_with(_args(E | FP), good)) == _lib.E_INVAL
    assert rc(_with(_args(E | FP, exp_ratio=0x1000, bias=0x1000, dark=0x1000), good)) == _lib.E_INVAL
    loc = _local()
    with_loc = _esd(local=C.addressof(loc))
    assert ok(_with(_args(E | LOC, dtype=1), with_loc)) == 'stack_esd_kernel<16, unsigned short, false, false, true>'
    assert rc(_with(_args(E | LOC), good)) == _lib.E_INVAL                      # the flag without the meshes
    assert rc(_with(_args(E), with_loc)) == _lib.E_INVAL                        # the meshes without the flag
    assert rc(_with(_args(E | LOC), loc)) == _lib.E_INVAL                       # the mesh descriptor where the ESD one belongs
    assert rc(_with(_args(E | LOC | FP, exp_ratio=0x1000), with_loc)) == _lib.E_INVAL
    assert rc(_with(_args(E | LOC, exp_ratio=0x1000), with_loc)) == _lib.E_INVAL
    for bad in (dict(width=0), dict(width=100), dict(row0=-1), dict(box_height=0), dict(box_width=32769), dict(ny=0), dict(offset=None)):
        d = _local(**bad)
        assert rc(_with(_args(E | LOC), _esd(local=C.addressof(d)))) == _lib.E_INVAL, bad


def test_capi_names_the_esd_kernels():
    from astrophotography_amd import _lib, ops
    lib = _lib.load()
    buf = C.create_string_buffer(256)
    names = set()
    for dtype, tname in ((0, 'float'), (1, 'unsigned short')):
        for n, slots in ((1, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64), (65, 128), (128, 128)):
            for calib in (False, True):
                kw = dict(bias=0x1000, dark=0x1000, exp_ratio=0x1000) if calib else {}
                a = _with(_args(_lib.STACK_REJECT_ESD, n_frames=n, dtype=dtype, **kw), _esd())
                assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0, lib.apgpu_last_error()
                assert buf.value.decode() == 'stack_esd_kernel<%d, %s, %s>' % (slots, tname, 'true' if calib else 'false')
                names.add(buf.value)
    assert len(names) == 20
    assert ops.stack_kernel_name(24, calibrated=False, rejection='esd') == 'stack_esd_kernel<32, float, false>'
    assert ops.stack_kernel_name(24, dtype='u16', calibrated=True, rejection='esd') == 'stack_esd_kernel<32, unsigned short, true>'
    assert ops.stack_kernel_name(10, calibrated=False, rejection='minmax') == 'stack_reject_kernel<16, float, false>'


def test_ops_argument_errors():
    import torch
    from astrophotography_amd import ops
    t = torch.zeros((10, 8), dtype=torch.float32)
    for kw in (dict(esd_outliers=0.6), dict(esd_outliers=-0.1), dict(esd_low_relaxation=0.5), dict(esd_low_relaxation=float('inf')),
               dict(esd_significance=0.0), dict(esd_table=np.zeros((10, 3))), dict(esd_table=np.zeros((11, 65))),
               dict(esd_table=np.full((11, 3), np.nan)), dict(outputs=('median',))):
        with pytest.raises(ValueError):
            ops.stack_reject(t, 'esd', **kw)
    with pytest.raises(ValueError, match='method must be'):
        ops.stack_reject(t, 'linear')
    with pytest.raises(ValueError):
        ops.stack_kernel_name(10, rejection='linear')
    with pytest.raises(ValueError, match='at most 128'):
        ops.stack_reject(torch.zeros((129, 8)), 'esd')


# ---------------------------------------------------------------------------------------------------------------------------
# the science: the ten-frame trail of tests/test_gpu_stack_reject.py (seed 2026, +400 ADU on 2 of 10 frames)
SKY, NOISE, TRAIL = 100.0, 5.0, 400.0


def _trail_stack(n=10, trail=TRAIL, frames=(2, 6), seed=2026):
    rng = np.random.default_rng(seed)
    shape = (48, 80)
    cube = rng.normal(SKY, NOISE, (n,) + shape).astype(F)
    on = np.zeros(shape, bool)
    for x in range(8, 72):
        y = 6 + x // 2
        on[y, x] = on[y + 1, x] = True
    for f in frames:
        cube[f][on] += trail
    return cube, on


@pytest.mark.parametrize('trail', [400.0, 120.0])
def test_trail_is_removed_and_clean_columns_are_left_alone(trail):
    from astrophotography_amd import ops
    cube, on = _trail_stack(trail=trail)
    r = model.esd(cube, ops.esd_lambda(10, 0.3, 0.05), 0.3, 1.5)
    w = reject.winsorized(cube)
    img, cnt = r['mean_f64'][on], r['count'][on]
    assert on.sum() > 60
    assert not r['keep'][[2, 6]][:, on].any()                                   # every trail value is gone
    assert (cnt <= 8).all() and (cnt >= 4).all(), (cnt.min(), cnt.max())        # _trail_checks' two conditions
    assert (np.abs(img - SKY) <= 6 * NOISE / np.sqrt(cnt)).all(), float(np.abs(img - SKY).max())
    lost = float((r['count'][~on] < 10).mean())
    lost_w = float((w['count'][~on] < 10).mean())
    print('off the trail: columns that lose a value %.3f (Winsorized %.3f), mean count %.3f (%.3f), rms about the sky %.3f (%.3f)'
          % (lost, lost_w, r['count'][~on].mean(), w['count'][~on].mean(), np.sqrt(((r['mean_f64'][~on] - SKY) ** 2).mean()),
             np.sqrt(((w['mean_f64'][~on] - SKY) ** 2).mean())))
    assert lost < lost_w


def test_masking_and_the_declared_fraction():
    from astrophotography_amd import ops
    rng = np.random.default_rng(5)
    cube = rng.normal(SKY, NOISE, (24, 2000)).astype(F)
    cube[[1, 9, 17]] += F(40.0)                                                 # three equal outliers of 24: all go, everywhere
    r = model.esd(cube, ops.esd_lambda(24, 0.3, 0.05), 0.3, 1.5)
    assert not r['keep'][[1, 9, 17]].any()
    cube = rng.normal(SKY, NOISE, (16, 500)).astype(F)
    cube[[0, 3, 6, 9, 12]] += F(400.0)                                          # 5 of 16 is beyond outliers = 0.3: by design, nothing goes
    r = model.esd(cube, ops.esd_lambda(16, 0.3, 0.05), 0.3, 1.5)
    assert (r['count'] == 16).all()
