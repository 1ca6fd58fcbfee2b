"""The rejection rules of small stacks on the CPU: what the NumPy model (tests/stack_reject_model.py) does on the data the
rules were added for, its edge columns, and the argument checks of the C ABI (which run before any device work)."""
import ctypes as C

import numpy as np
import pytest

from tests import stack_reject_model as model
from tests.util import assert_biteq

F = np.float32


def _col(*values):
    return np.array(values, F).reshape(-1, 1)


def _small_stack(n, seed, columns=3000):
    """columns x n values of N(1000, 10) with +500 on one frame (n < 8) or two frames -> (cube [n, columns], injected mask)."""
    rng = np.random.default_rng(seed)
    cube = rng.normal(1000.0, 10.0, (n, columns))
    inj = np.zeros((n, columns), bool)
    k = 1 if n < 8 else 2
    for c in range(columns):
        inj[rng.choice(n, k, replace=False), c] = True
    cube[inj] += 500.0
    return cube.astype(F), inj


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the experiment the rules were added for
@pytest.mark.parametrize('n, cap', [(5, 0.08), (8, 0.05), (10, 0.05), (12, 0.05)])
def test_small_stacks_lose_their_outliers_to_the_winsorized_rule_only(n, cap):
    from oracle import apref
    cube, inj = _small_stack(n, seed=20261019 + n)
    w = model.winsorized(cube, 3.0, 3.0)
    assert not (w['keep'] & inj).any(), 'the Winsorized rule kept an injected value'
    lost = (~w['keep'] & ~inj).sum() / (~inj).sum()
    print('n = %d: good values lost %.4f (cap %.2f)' % (n, lost, cap))
    assert lost <= cap
    clip = apref.stack_sigclip(cube, sigma=3.0, maxiters=5, want=('keep', 'count'))
    kept = (np.asarray(clip['keep'], bool) & inj).sum(0)
    assert (kept == inj.sum(0)).all(), 'the 3-sigma std clip removed an injected value in %d columns' % (kept != inj.sum(0)).sum()


@pytest.mark.parametrize('n', [64, 128])
def test_clean_columns_lose_under_one_percent(n):
    rng = np.random.default_rng(7 + n)
    cube = rng.normal(1000.0, 10.0, (n, 3000)).astype(F)
    w = model.winsorized(cube, 3.0, 3.0)
    lost = 1.0 - w['keep'].mean()
    print('n = %d: clean values lost %.4f' % (n, lost))
    assert lost < 0.01
    assert not w['capped'].any()                  # the inner cap is a matter of small stacks


# ---------------------------------------------------------------------------------------------------------------------------
# 2. edge columns
def test_vectorised_model_equals_one_dimensional_numpy():
    """The model reduces [columns, n] arrays along the last axis; the definition speaks of 1-D calls.  Same bits."""
    rng = np.random.default_rng(3)
    for n in (3, 7, 8, 9, 17, 64, 100, 128):
        cube = rng.normal(50.0, 30.0, (n, 40)).astype(F)
        cube[rng.random(cube.shape) < 0.1] += 900.0
        for r in (model.winsorized(cube, 2.5, 3.0), model.minmax(cube, 1, 2)):
            for c in range(cube.shape[1]):
                s = cube[r['keep'][:, c], c]
                if s.size == 0:
                    assert np.isnan(r['mean_f64'][c]) and np.isnan(r['std_f64'][c]) and r['count'][c] == 0
                    continue
                m, sd = model.column_stats_1d(s)
                assert_biteq(np.array([m, sd]), np.array([r['mean_f64'][c], r['std_f64'][c]]), 'n = %d column %d' % (n, c))


def test_winsorized_round_by_hand():
    """[1, 1, 1, 100]: med 1, sig 42.9 -> W = S clamped to 1 +- 64.3 -> 1.134 std(W) ... the bound falls below 100."""
    r = model.winsorized(_col(1, 1, 1, 100), 3.0, 3.0)
    assert r['keep'][:, 0].tolist() == [True, True, True, False]
    assert r['count'][0] == 3 and r['mean_f64'][0] == 1.0 and r['std_f64'][0] == 0.0


def test_winsorized_edge_columns():
    # constant columns keep everything (sig == 0: the bounds are the median itself, inclusive)
    for n in (3, 4, 9, 64):
        r = model.winsorized(np.full((n, 1), 7.25, F))
        assert r['count'][0] == n and r['mean_f64'][0] == 7.25 and r['std_f64'][0] == 0.0 and r['inner'][0] == 1
    # fewer than three values: no round
    for vals in ((5.0,), (5.0, 1e6)):
        r = model.winsorized(_col(*vals))
        assert r['count'][0] == len(vals) and r['rounds'][0] == 0
    # nothing finite, and a masked pixel: NaN and 0
    r = model.winsorized(_col(np.nan, np.inf, -np.inf))
    assert r['count'][0] == 0 and np.isnan(r['mean_f64'][0]) and np.isnan(r['std_f64'][0])
    r = model.winsorized(_col(1, 2, 3), pixmask=np.array([1], np.uint8))
    assert r['count'][0] == 0 and np.isnan(r['mean_f64'][0])
    # non-finite values are not part of S
    r = model.winsorized(_col(1, np.nan, 1, np.inf, 1, 100))
    assert r['keep'][:, 0].tolist() == [True, False, True, False, True, False]
    # zeros of both signs: a constant column in value
    r = model.winsorized(_col(0.0, -0.0, 0.0, -0.0, -0.0))
    assert r['count'][0] == 5 and r['mean_f64'][0] == 0.0 and r['std_f64'][0] == 0.0
    r = model.winsorized(_col(-0.0, 0.0, -0.0, 0.0, 50.0, -0.0, 0.0, -0.0, 0.0))
    assert r['count'][0] == 8 and r['mean_f64'][0] == 0.0
    # kl != kh: the low value goes at kl = 1, stays at kl = 6; the high one the other way round
    col = _col(10, 11, 9, 10, 12, 8, 10, 11, 9, 2, 18)
    lo = model.winsorized(col, 1.0, 6.0, maxiters=1)
    hi = model.winsorized(col, 6.0, 1.0, maxiters=1)
    assert not lo['keep'][9, 0] and lo['keep'][10, 0]
    assert hi['keep'][9, 0] and not hi['keep'][10, 0]
    # maxiters = 1 stops after one round where the free run goes on
    rng = np.random.default_rng(11)
    cube = rng.normal(0, 1, (12, 400)).astype(F)
    cube[3] += 8.0
    cube[7, ::2] += 4.0
    one, free = model.winsorized(cube, 2.0, 2.0, maxiters=1), model.winsorized(cube, 2.0, 2.0)
    assert (one['rounds'] == 1).all() and (free['rounds'] > 1).any()
    assert (free['count'] <= one['count']).all() and (free['count'] < one['count']).any()


def test_inner_cap_is_reached_and_is_not_the_rule():
    rng = np.random.default_rng(5)
    cube = rng.normal(1000.0, 10.0, (5, 3000)).astype(F)
    r = model.winsorized(cube)
    assert r['capped'].any() and (~r['capped']).any()
    assert (r['inner_max'][r['capped']] == model.MAX_INNER).all() and (r['inner_max'][~r['capped']] < model.MAX_INNER).any()
    # the estimate never collapses to zero on a column that is not constant: no column is emptied
    assert (r['count'] >= 2).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. min/max
def test_minmax_is_a_trimmed_mean():
    rng = np.random.default_rng(9)
    for n, nlow, nhigh in ((5, 1, 1), (10, 2, 3), (16, 0, 2), (16, 3, 0), (33, 1, 1)):
        cube = rng.normal(100.0, 20.0, (n, 200)).astype(F)
        r = model.minmax(cube, nlow, nhigh)
        s = np.sort(cube.astype(np.float64), axis=0)[nlow:n - nhigh]
        assert (r['count'] == n - nlow - nhigh).all()
        np.testing.assert_allclose(r['mean_f64'], s.mean(0), rtol=1e-14)
        np.testing.assert_allclose(r['std_f64'], s.std(0), rtol=1e-12)


def test_minmax_edges():
    cube = np.random.default_rng(2).normal(0, 1, (6, 50)).astype(F)
    for nlow, nhigh in ((3, 3), (6, 0), (2, 5), (127, 127)):
        r = model.minmax(cube, nlow, nhigh)                   # n <= nlow + nhigh: nothing survives
        assert (r['count'] == 0).all() and np.isnan(r['mean_f64']).all()
    r = model.minmax(cube, 0, 0)                              # nothing dropped: the plain mean of the model
    w = model.winsorized(cube, 1e30, 1e30)
    assert r['keep'].all()
    assert_biteq(r['mean_f64'], w['mean_f64'])
    assert_biteq(r['std_f64'], w['std_f64'])
    # non-finite values are not ranked
    r = model.minmax(_col(np.inf, 3, 1, np.nan, 2, 5, 4), 1, 1)
    assert r['keep'][:, 0].tolist() == [False, True, False, False, True, False, True]


def test_minmax_tie_rule_decides_the_bits():
    """Equal values go by frame index: the FIRST of the low ties and the LAST of the high ties.  Which one goes moves the
    others between the accumulators of the sum - the columns below are built so that the low bits differ."""
    rng = np.random.default_rng(4)
    n = 24
    found = 0
    for _ in range(200):
        col = (rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-8, 8, n)).astype(F)      # wide range: float64 sums that round
        lo, hi = F(-3e9), F(3e9)
        col[[2, 13]] = lo                                      # two lowest, two highest, apart
        col[[5, 20]] = hi
        r = model.minmax(col.reshape(-1, 1), 1, 1)
        keep = r['keep'][:, 0]
        assert not keep[2] and keep[13] and keep[5] and not keep[20]
        other = np.ones(n, bool)
        other[[13, 5]] = False                                 # the other choice: same values, another order
        m_other, _ = model.column_stats_1d(col[other])
        assert np.sort(col[other]).tolist() == np.sort(col[keep]).tolist()
        found += m_other != r['mean_f64'][0]
    assert found > 20, found
    # -0.0 sorts below +0.0 whatever the frame order
    r = model.minmax(_col(0.0, -0.0, 1.0, 2.0), 1, 0)
    assert r['keep'][:, 0].tolist() == [True, False, True, True]


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the C ABI: every rule is checked before any device work (no GPU here)
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


def test_capi_checks_of_the_rejection_rules():
    from astrophotography_amd import _lib
    lib = _lib.load()
    W, M = _lib.STACK_REJECT_WINSORIZED, _lib.STACK_REJECT_MINMAX
    assert (W, M, _lib.STACK_REJECT_MAX) == (16, 32, 128)
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), 'include', 'apgpu.h')).read()
    for name, val in (('APGPU_STACK_REJECT_WINSORIZED', 16), ('APGPU_STACK_REJECT_MINMAX', 32), ('APGPU_STACK_REJECT_MAX', 128),
                      ('APGPU_STACK_WINSOR_MAX_INNER', model.MAX_INNER)):
        assert '#define %s %d\n' % (name, val) in hdr
    buf = C.create_string_buffer(256)

    def rc(a):
        r = lib.apgpu_stack_sigclip(C.byref(a), None)
        assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == r      # the query runs the same checks
        return r, lib.apgpu_last_error().decode()

    bad = [
        (_args(W | M), _lib.E_INVAL, 'exclude'),
        (_args(W | _lib.STACK_NONFINITE_UNCLIPPED, dev=1), _lib.E_INVAL, 'NONFINITE'),
        (_args(M | _lib.STACK_NONFINITE_UNCLIPPED, dev=1, sigma_lower=1.0, sigma_upper=1.0), _lib.E_INVAL, 'NONFINITE'),
        (_args(W | 64), _lib.E_INVAL, 'unknown flags'),
        (_args(W, center=1), _lib.E_INVAL, 'CENTER_MEDIAN'),
        (_args(W, dev=1), _lib.E_INVAL, 'DEV_STD'),
        (_args(M, center=1, sigma_lower=1.0, sigma_upper=1.0), _lib.E_INVAL, 'CENTER_MEDIAN'),
        (_args(W, sigma_lower=-1.0), _lib.E_INVAL, 'sigma'),
        (_args(W, sigma_upper=float('nan')), _lib.E_INVAL, 'sigma'),
        (_args(W, maxiters=0), _lib.E_INVAL, 'maxiters'),
        (_args(M, sigma_lower=1.5, sigma_upper=1.0), _lib.E_INVAL, 'whole numbers'),
        (_args(M, sigma_lower=1.0, sigma_upper=128.0), _lib.E_INVAL, 'whole numbers'),
        (_args(M, sigma_lower=-1.0, sigma_upper=1.0), _lib.E_INVAL, 'whole numbers'),
        (_args(M, sigma_lower=float('nan'), sigma_upper=1.0), _lib.E_INVAL, 'whole numbers'),
        (_args(W, moments=0x1000), _lib.E_UNSUPPORTED, 'mean, std, count'),
        (_args(W, median=0x1000), _lib.E_UNSUPPORTED, 'mean, std, count'),
        (_args(M, median=0x1000, sigma_lower=1.0, sigma_upper=1.0), _lib.E_UNSUPPORTED, 'mean, std, count'),
        (_args(W, n_frames=129), _lib.E_UNSUPPORTED, 'APGPU_STACK_REJECT_MAX = 128'),
        (_args(M, n_frames=200, sigma_lower=1.0, sigma_upper=1.0), _lib.E_UNSUPPORTED, 'APGPU_STACK_REJECT_MAX = 128'),
        (_args(W, mean=None), _lib.E_INVAL, 'no output'),
    ]
    for a, want, text in bad:
        got, msg = rc(a)
        assert got == want and text in msg, (got, want, text, msg)


def test_capi_names_the_reject_kernel():
    from astrophotography_amd import _lib, ops
    lib = _lib.load()
    W, M = _lib.STACK_REJECT_WINSORIZED, _lib.STACK_REJECT_MINMAX
    buf = C.create_string_buffer(256)
    # the flags without effect, a misaligned workspace that is never looked at, maxiters = 0 under min/max (unused)
    for a in (_args(W), _args(W | 1 | 2 | 4, workspace=0x1001, workspace_bytes=1), _args(M, sigma_lower=1.0, sigma_upper=0.0, maxiters=0),
              _args(W, maxiters=-1, std=0x1000, count=0x1000, mean_f64=0x1000, std_f64=0x1000)):
        assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0, lib.apgpu_last_error()
        assert buf.value == b'stack_reject_kernel<16, float, false>'
    slots = set()
    for n in range(1, 129):
        a = _args(W, n_frames=n, dtype=1, bias=0x1000, dark=0x1000, exp_ratio=0x1000)
        assert lib.apgpu_stack_kernel_name(C.byref(a), 0, buf, 256) == 0
        name = buf.value.decode()
        assert name.startswith('stack_reject_kernel<') and name.endswith(', unsigned short, true>')
        s = int(name.split('<')[1].split(',')[0])
        assert s >= n
        slots.add(s)
    assert max(slots) == 128
    assert ops.stack_kernel_name(10, calibrated=False, rejection='winsorized') == 'stack_reject_kernel<16, float, false>'
    assert ops.stack_kernel_name(64, dtype='u16', rejection='minmax') == 'stack_reject_kernel<64, unsigned short, true>'
    assert 'reject' not in ops.stack_kernel_name(64)
    # apgpu_stack_median does not know the bits: it never read `flags`
    a = _args(W, median=0x1000)
    assert lib.apgpu_stack_kernel_name(C.byref(a), 1, buf, 256) == 0 and buf.value.startswith(b'stack_median')


def test_capi_resample_stack_refuses_the_rules():
    from astrophotography_amd import _lib
    lib = _lib.load()
    for flag in (_lib.STACK_REJECT_WINSORIZED, _lib.STACK_REJECT_MINMAX):
        a = _args(flag, n_frames=4, n_pixels=64 * 64)
        r = lib.apgpu_resample_stack_sigclip(C.byref(a), 64, 64, None, 0x1000, 0, 0, None, 0x1000, 1024, 64, 64, None, 0, None)
        assert r == _lib.E_UNSUPPORTED and 'rejection' in lib.apgpu_last_error().decode()


def test_python_surface_checks_before_the_library():
    import torch
    from astrophotography_amd import ops
    from astrophotography_amd.core.ApStack import METHODS, ApStack
    assert 'winsorized' in METHODS and 'minmax' in METHODS
    x = torch.zeros((4, 8, 8))
    with pytest.raises(ValueError, match='method'):
        ops.stack_reject(x, method='sigclip')
    with pytest.raises(ValueError, match='outputs'):
        ops.stack_reject(x, outputs=('median',))
    with pytest.raises(ValueError, match='nlow'):
        ops.stack_reject(x, 'minmax', nlow=1.5)
    with pytest.raises(ValueError, match='nhigh'):
        ops.stack_reject(x, 'minmax', nhigh=128)
    with pytest.raises(ValueError, match='128'):
        ops.stack_reject(torch.zeros((129, 2, 2)))
    with pytest.raises(ValueError, match='128'):
        ApStack(loglevel='ERROR').stack(torch.zeros((129, 2, 2)), method='winsorized')
    with pytest.raises(ValueError, match='MEDIAN, AVERAGE, WEIGHTED, SUM, CLIPPED, WINSORIZED, MINMAX'):
        ops.coadd(x, None, combine='BEST')
    from astrophotography_amd import parallel
    with pytest.raises(ValueError, match='stack_rowshard'):
        parallel.stack_nshard(x, rejection='winsorized')
    from astrophotography_amd.scripts import ap_coadd
    p = ap_coadd.command_line_opts(['out.fits', 'a.fits', '--combine', 'MINMAX', '--nlow', '0', '--nhigh', '2'])
    assert (p.combine, p.nlow, p.nhigh) == ('MINMAX', 0, 2)
    p = ap_coadd.command_line_opts(['out.fits', 'a.fits', '--combine', 'WINSORIZED', '--sigma', '2.5'])
    assert (p.combine, p.nlow, p.nhigh, p.sigma) == ('WINSORIZED', 1, 1, 2.5)
