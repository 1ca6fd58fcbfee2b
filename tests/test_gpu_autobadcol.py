"""F5 ApAutoBadcols on the MI355X: bit-exact against the reference's own numbers (G13), the script's stdout, full-size
frames, lines of thousands of values, the slab form and the round trip into ApFindBadPixels' user bad-pixel file."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from tests.util import GOLDEN, assert_biteq, load_golden, np_clip_stats as _np_clip_stats

pytestmark = pytest.mark.gpu


def _g13():
    a = load_golden('g13_autobadcol.npz')
    b = load_golden('g13_autobadcol_paths.npz')
    arrs = {**{k: a[k] for k in a.files}, **{k: b[k] for k in b.files if not k.startswith('_')}}
    names = json.loads(str(a['_cases'])) + json.loads(str(b['_cases']))
    return arrs, names, json.loads(str(a['_meta']))


G13, CASES, META = _g13()


def _data(name):
    key = name + '/data'
    if key not in G13:
        key = str(G13[name + '/data_from']) + '/data'
    return G13[key]


def _dev(a):
    import torch
    from astrophotography_amd import ops
    if a.dtype == np.uint16:
        return ops.to_device_u16(a)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('name', CASES)
def test_g13_bit_exact(name):
    from astrophotography_amd import ops
    import astrophotography_amd as ap
    data = _data(name)
    w = int(G13[name + '/window'])
    nsigma = float(G13[name + '/nsigma'])
    d = _dev(data)
    r = ops.auto_badcols(d, nsigma=nsigma, window_len=w)
    for tag in ('cols', 'rows'):
        ref_med = G13['%s/med_%s' % (name, tag)]
        assert_biteq(r[tag]['median'].cpu().numpy(), ref_med, '%s %s median' % (name, tag))
        for k in ('mean', 'std', 'nsig'):
            assert_biteq(r[tag][k].cpu().numpy(), G13['%s/%s_%s' % (name, k, tag)], '%s %s %s' % (name, tag, k))
        assert np.array_equal(r[tag]['flag'].cpu().numpy(), G13['%s/flag_%s' % (name, tag)]), (name, tag)
    badcols, badrows = ap.ApAutoBadcols('CRITICAL').process(data, nsigma, w)
    for got, key in ((badcols, 'badcols'), (badrows, 'badrows')):
        if bool(G13['%s/%s_none' % (name, key)]):
            assert got is None, (name, key, got)
        else:
            assert got is not None and got.dtype == np.int64
            assert np.array_equal(got, G13['%s/%s' % (name, key)]), (name, key)


def test_g13_sliding_stats_on_reference_medians():
    """sliding_clipped_stats alone, fed the reference's median arrays, in one batched call per case and axis."""
    import torch
    from astrophotography_amd import ops
    for name in CASES:
        w = int(G13[name + '/window'])
        for tag in ('cols', 'rows'):
            m = G13['%s/med_%s' % (name, tag)]
            r = ops.sliding_clipped_stats(torch.from_numpy(m).cuda(), w, nsigma=float(G13[name + '/nsigma']))
            for k in ('mean', 'std', 'nsig'):
                assert_biteq(r[k].cpu().numpy(), G13['%s/%s_%s' % (name, k, tag)], '%s %s %s' % (name, tag, k))


@pytest.mark.parametrize('run', range(4))
def test_script_stdout_matches_reference(run):
    from astrophotography_amd.scripts import ap_auto_badcol as s
    rec = META['runs'][run]
    path = os.path.join(GOLDEN, rec['file'])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert s.main([path, '-l', 'CRITICAL'] + rec['argv']) == 0
    assert buf.getvalue() == rec['stdout'].replace(META['placeholder'], path)


def _structured(rng, H, W, badcols, badrows, dtype=np.float32):
    """P[r] + Q[c] with integer ramps: every column median is median(P) + Q[c] and every row median P[r] + median(Q)
    exactly, so the injected lines are the only ones nsigma away from their neighbours."""
    P = 3 * np.arange(H) + rng.integers(0, 2, H)
    Q = 2 * np.arange(W) + rng.integers(0, 2, W)
    Q[badcols] += np.where(np.arange(len(badcols)) % 2 == 0, 5000, -5000)
    P[badrows] += np.where(np.arange(len(badrows)) % 2 == 0, 7000, -7000)
    return (P[:, None] + Q[None, :] + 20000).astype(dtype)


@pytest.mark.parametrize('H,W', [(2672, 4008), (4096, 4096)])
def test_full_size(H, W):
    import torch
    import astrophotography_amd as ap
    from astrophotography_amd import ops
    rng = np.random.default_rng(H + W)
    # medians of a noisy frame with NaNs, bit-exact against numpy on this machine
    noisy = (1000.0 + 15.0 * rng.standard_normal((H, W))).astype(np.float32)
    noisy[rng.integers(0, H, 2000), rng.integers(0, W, 2000)] = np.nan
    noisy[:, 77] += 40.0
    d = torch.from_numpy(noisy).cuda()
    r = ops.auto_badcols(d)
    for tag, axis in (('cols', 0), ('rows', 1)):
        med = r[tag]['median'].cpu().numpy()
        assert_biteq(med, np.nanmedian(noisy, axis=axis), 'full-size %s median' % tag)
        # sliding statistics at ~256 sampled indices per axis (edges included) against the G2-pinned global clip
        L = med.size
        idx = np.unique(np.concatenate([np.arange(6), L - 1 - np.arange(6), rng.integers(0, L, 244)]))
        mean = r[tag]['mean'].cpu().numpy()
        std = r[tag]['std'].cpu().numpy()
        for i in idx:
            win = torch.from_numpy(med[max(0, i - 5):min(L, i + 6)]).cuda()
            st = ops.sigclip_global(win, sigma=3.0, maxiters=5).cpu().numpy()
            assert_biteq(mean[i:i + 1], st[0:1], '%s mean at %d' % (tag, i))
            assert_biteq(std[i:i + 1], st[2:3], '%s std at %d' % (tag, i))
    # injected lines are found exactly
    badcols, badrows = [10, 101, 1500, W - 20], [7, 999, H - 9]      # (a line at an edge has a one-sided window)
    img = _structured(rng, H, W, badcols, badrows)
    bc, br = ap.ApAutoBadcols('CRITICAL').process(img)
    assert bc is not None and bc.tolist() == badcols
    assert br is not None and br.tolist() == badrows


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape', [(9000, 40), (40, 9000)])
def test_long_lines_exact(shape, dtype):
    import torch
    from astrophotography_amd import ops
    rng = np.random.default_rng(9000)
    a = (rng.standard_normal(shape) * 100).astype(dtype)
    a[rng.random(shape) < 0.01] = np.nan
    a[:, 3] = np.nan                                   # an all-NaN column
    a[5, :] = np.inf
    a[np.round(a) == 7] = -np.inf
    d = torch.from_numpy(a).cuda()
    for axis in (0, 1):
        assert_biteq(ops.axis_nanmedian(d, axis).cpu().numpy(), np.nanmedian(a, axis=axis), '%s axis %d' % (shape, axis))
    # windows longer than 128 values run numpy's pairwise tree: checked against the numpy restatement on samples
    m = ops.axis_nanmedian(d, 1 if shape[0] > shape[1] else 0)          # the 9000 medians
    mh = m.cpu().numpy()
    r = ops.sliding_clipped_stats(m, 301)
    mean, std = r['mean'].cpu().numpy(), r['std'].cpu().numpy()
    for i in (0, 1, 150, 151, 4000, mh.size - 1):
        x = _np_clip_stats(mh[max(0, i - 150):i + 151])
        assert_biteq(mean[i:i + 1], np.array([np.nanmean(x)], np.float64), 'mean at %d' % i)
        assert_biteq(std[i:i + 1], np.array([np.nanstd(x)], np.float64), 'std at %d' % i)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('L,window_len', [(400, 7), (400, 9), (400, 129), (400, 137), (400, 257), (1100, 2001)])
def test_window_sums_on_both_sides_of_numpys_boundaries(L, window_len, dtype):
    """sigma = 1e300 clips nothing, so every window's count is its length and mean and std are numpy's sums of exactly that
    many values: with the one-sided windows at the ends of the line the lengths run over 4 .. 9 (the leaf's short form),
    65 .. 137 (leaf against tree at 128), 129 .. 257 and 1001 .. 1100."""
    import torch
    from astrophotography_amd import ops
    rng = np.random.default_rng(L + window_len)
    v = (1000.0 + 50.0 * rng.standard_normal(L)).astype(dtype)
    r = ops.sliding_clipped_stats(torch.from_numpy(v).cuda(), window_len, sigma=1e300)
    hw = (window_len - 1) // 2
    wins = [v[max(0, i - hw):i + hw + 1] for i in range(L)]
    assert_biteq(r['mean'].cpu().numpy(), np.array([np.nanmean(x) for x in wins], np.float64), 'mean, window %d' % window_len)
    assert_biteq(r['std'].cpu().numpy(), np.array([np.nanstd(x) for x in wins], np.float64), 'std, window %d' % window_len)


def test_u16_and_integer_inputs():
    import torch
    from astrophotography_amd import ops
    rng = np.random.default_rng(16)
    a = rng.integers(0, 65536, (641, 37)).astype(np.uint16)
    for axis in (0, 1):
        ref = np.nanmedian(a, axis=axis)
        assert ref.dtype == np.float64
        assert_biteq(ops.axis_nanmedian(ops.to_device_u16(a), axis).cpu().numpy(), ref, 'u16 axis %d' % axis)
        b = a.astype(np.int32) - 30000
        assert_biteq(ops.axis_nanmedian(torch.from_numpy(b).cuda(), axis).cpu().numpy(), np.nanmedian(b, axis=axis),
                     'i32 axis %d' % axis)


def test_process_slab_equals_process_per_frame():
    import torch
    import astrophotography_amd as ap
    rng = np.random.default_rng(8)
    frames = (500.0 + 5.0 * rng.standard_normal((8, 96, 130))).astype(np.float32)
    for f in range(8):
        frames[f, :, 10 + 13 * f] += 200.0           # away from the edges (an edge line has a one-sided window)
        frames[f, 10 + 9 * f, :] -= 150.0
    ab = ap.ApAutoBadcols('CRITICAL')
    slab = ab.process_slab(torch.from_numpy(frames).cuda(), window_len=9)
    assert len(slab) == 8
    for f in range(8):
        one = ab.process(frames[f], window_len=9)
        for got, want in zip(slab[f], one):
            assert (got is None) == (want is None)
            if got is not None:
                assert np.array_equal(got, want)
        assert slab[f][0] is not None and 10 + 13 * f in slab[f][0]
        assert slab[f][1] is not None and 10 + 9 * f in slab[f][1]


def test_yaml_round_trip_into_find_badpix(tmp_path):
    """The documented workflow: ap_auto_badcol's stdout is pasted into the user bad-pixel file of ap_find_badpix."""
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio
    from astrophotography_amd.scripts import ap_auto_badcol as s
    rng = np.random.default_rng(31)
    H, W = 120, 150
    badcols, badrows = [12, 77, 130], [9, 60]
    img = _structured(rng, H, W, badcols, badrows)
    fimg = tmp_path / 'calibrated.fits'
    fitsio.write(str(fimg), img)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert s.main([str(fimg), '-l', 'CRITICAL']) == 0
    yml = tmp_path / 'user_badpix.yml'
    yml.write_text(buf.getvalue())
    dark = (100.0 + rng.standard_normal((H, W))).astype(np.float32)
    fdark = tmp_path / 'dark.fits'
    fitsio.write(str(fdark), dark)
    fb = ap.ApFindBadPixels(str(fdark), 4.0, 'CRITICAL')
    auto = fb.get_mask().astype(np.int64).copy()
    fb.add_user_badpix(str(yml))
    mask = fb.get_mask().astype(np.int64)
    want = np.zeros((H, W), np.int64)
    want[:, badcols] += ap.ApFindBadPixels.USER_BAD
    want[badrows, :] += ap.ApFindBadPixels.USER_BAD
    assert np.array_equal(mask - auto, want)


def test_debug_table_and_info_line():
    """At DEBUG the reference's diagnostics table is formatted from the same numbers (the result does not change)."""
    import logging
    import astrophotography_amd as ap
    name = 'f32_even'
    data = _data(name)
    ab = ap.ApAutoBadcols('DEBUG')
    lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    h = Keep()
    ab._logger.addHandler(h)
    try:
        badcols, badrows = ab.process(data)
    finally:
        ab._logger.removeHandler(h)
    assert np.array_equal(badcols, G13[name + '/badcols']) and np.array_equal(badrows, G13[name + '/badrows'])
    assert 'Found %d bad columns out of 96 columns.' % len(badcols) in lines
    assert 'Found %d bad rows out of 64 rows.' % len(badrows) in lines
    table = [m for m in lines if m.startswith('Diagnostics for first 40 columns')][0].split('\n')
    assert table[1] == ' col,     median, local_mean,  local_std,     nsigma, isbad?'
    c = int(badcols[0])
    m = G13[name + '/med_cols']
    row = [t for t in table if t.startswith('%04d,' % c)][0]
    assert row.startswith('%04d, %10.2f, %10.2f' % (c, m[c], G13[name + '/mean_cols'][c])) and row.endswith('True')
