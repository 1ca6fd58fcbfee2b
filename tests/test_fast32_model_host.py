"""The host model of the float32 fast path's clipped mean (tools/fast32_model.py) and the worst-case fixture G14
(tests/golden/g14_fast32_columns.npz, tools/fast32_search.py).  No GPU.

(a) columns the release guard (rms(d) <= |c| / 4) accepts, with the largest pre-rounding error the search found: the model
    keeps them within 1 ulp of the correctly rounded mean;
(b) columns the old guard (rms(d) <= |c| / 2) would have accepted with a mean 2 ulp or more off: the release guard sends them
    to the exact path.
Each for both forms of the fast path: 'calib' (a_N / b_N, tails of 4) and 'plain' (ap_N / bp_N, tails of 8)."""
import os
import sys

import numpy as np
import pytest

from tests.util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import fast32_model as fm  # noqa: E402
import fast32_search as fs  # noqa: E402

FIXTURE = os.path.join(GOLDEN, 'g14_fast32_columns.npz')


@pytest.fixture(scope='module')
def g14():
    return np.load(FIXTURE, allow_pickle=False)


FORMS = (('calib', ''), ('plain', 'p'))


def test_fixture_is_small_and_covers_every_frame_count(g14):
    assert os.path.getsize(FIXTURE) < 512 * 1024
    for _, key in FORMS:
        for N in fs.FRAME_COUNTS:
            a = g14['a%s_%d' % (key, N)]
            assert a.dtype == np.float32 and a.shape == (fs.KEEP, N), N
            assert g14['b%s_%d' % (key, N)].shape[1] == N
    # the weak spots the old guard left open: 2-ulp means at 24, 48, 64, 96 and 128 frames and the padded counts
    for N in (24, 48, 64, 96, 128, 13, 30, 61):
        assert len(g14['b_%d' % N]) > 0 and len(g14['bp_%d' % N]) > 0, N


@pytest.mark.parametrize('form,key', FORMS)
def test_fixture_b_is_two_ulp_under_the_old_guard_and_exact_path_under_the_release_guard(g14, form, key):
    for N in fs.FRAME_COUNTS:
        b = g14['b%s_%d' % (key, N)]
        if not len(b):
            continue
        old = fm.evaluate(b, guard=fm.GUARD_OLD, form=form)
        assert old['done'].all(), N
        assert (old['ulp_dist'] >= 2).all(), (N, old['ulp_dist'])
        assert (np.abs(old['err_ulp']) > 1.0).all(), N
        new = fm.evaluate(b, guard=fm.GUARD_RELEASE, form=form)
        assert not new['done'].any(), N


@pytest.mark.parametrize('form,key', FORMS)
def test_fixture_a_is_accepted_and_within_one_ulp(g14, form, key):
    for N in fs.FRAME_COUNTS:
        a = g14['a%s_%d' % (key, N)]
        e = fm.evaluate(a, guard=fm.GUARD_RELEASE, form=form)
        assert e['done'].all(), N
        assert (e['ulp_dist'] <= 1).all(), (N, e['ulp_dist'].max())
        np.testing.assert_array_equal(e['err_ulp'], g14['a%s_err_%d' % (key, N)])
        # the search did push them: most sit near the guard's edge, rms(d) / |c| in (1/8, 1/4]
        r = fm.clip_fast32(a, form=form)
        ratio = np.sqrt(r['Q'].astype(np.float64) / e['count']) / np.abs(r['cf'].astype(np.float64))
        assert (ratio <= 0.25).all() and np.median(ratio) > 0.125, (N, ratio)


def test_above_96_slots_the_guard_alone_is_not_enough():
    """Where the search found 2-ulp means under the release guard (128 frames): without the a-posteriori check of the
    > 96-slot fast kernels (finish_fast_column) the model's fast path returns them, with it not."""
    rng = np.random.default_rng(7)
    c, _ = fs.search(128, fm.GUARD_RELEASE, 1528, mean_check=False)
    cand = np.repeat(c.astype(np.float64), 200, axis=0) * (1 + rng.normal(0, 2.0 ** -18, 200 * len(c)))[:, None]
    cand = cand.astype(np.float32)
    raw = fm.evaluate(cand, mean_check=False)
    assert (raw['ulp_dist'][raw['done']] >= 2).any()
    chk = fm.evaluate(cand)
    assert (chk['ulp_dist'][chk['done']] <= 1).all()
    assert chk['done'].mean() > 0.2


def test_forms_tail_lengths():
    assert fm.slots(64, 'calib') == (64, 4, 0, 0) and fm.slots(64, 'plain') == (64, 8, 0, 0)
    assert fm.slots(16, 'plain') == (16, 6, 0, 0) and fm.slots(13, 'plain') == (16, 6, 1, 2)
    assert fm.slots(61, 'calib') == (64, 6, 1, 2) and fm.slots(125, 'calib') == (128, 8, 1, 2)


@pytest.mark.parametrize('form', fm.FORMS)
def test_model_sums_match_an_exact_reference_on_easy_columns(form):
    """Sanity of the model itself: columns whose every operation is exact (small integers) give the exact mean and count,
    full and padded slot counts, with trims."""
    rng = np.random.default_rng(3)
    for N in (16, 13, 30, 64, 61, 96, 128):
        cols = rng.integers(1000, 1010, (64, N)).astype(np.float32)
        cols[:8, 0] = 5000.0                                     # one outlier: trimmed
        e = fm.evaluate(cols, form=form)
        keep = np.ones_like(cols, bool)
        keep[:8, 0] = False
        want = np.where(keep, cols.astype(np.float64), 0).sum(1) / keep.sum(1)
        assert (e['count'][e['done']] == keep.sum(1)[e['done']]).all(), N
        if fm.exact_model(N):
            assert np.array_equal(e['mean'][e['done']], want.astype(np.float32)[e['done']]), N


def test_fma32_rounds_once():
    a = np.float32(1 + 2.0 ** -12)
    # a * a = 1 + 2^-11 + 2^-24: a single rounding keeps the 2^-24 as the tie breaker a double rounding loses
    assert fm.fma32(a, a, np.float32(-1.0)) == np.float32(2.0 ** -11 + 2.0 ** -24)
    x = np.float32(1 + 2.0 ** -23)
    got = fm.fma32(x, x, np.float32(0.0))                        # 1 + 2^-22 + 2^-46: rounds to 1 + 2^-22
    assert got == np.float32(1 + 2.0 ** -22)


def test_search_regenerates_the_fixture():
    """tools/fast32_search.py is deterministic: the committed fixture is what it writes (~20 s)."""
    arrays, _ = fs.build()
    with open(FIXTURE, 'rb') as f:
        assert f.read() == fs.to_bytes(arrays)
