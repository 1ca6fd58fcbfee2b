"""tests/fixbadpix_model.py checked without a GPU: the packed catalogue of tests/orderstat_cases.py keeps every line's
median (the model at a centre is the median by construction, NaN for a line with a NaN), the CPU oracle's repair
(oracle/apref.c, apref_fix_badpix_f32 / _f64: qsort and its own mean of the middle) equals the model at every bad pixel of
every packed image with equal stats, and the packed cases tell np.median from two subtly wrong medians.  That is the evidence
that tests/test_gpu_fixbadpix.py, which runs the same images through csrc/fixbadpix.hip, would notice such a kernel.

Found with this module: the oracle returned -0.0 where np.median returns +0.0, for a window whose middle value(s) are -0.0
with no +0.0 among the good pixels.  Before the fix test_oracle_equals_the_model_at_every_bad_pixel failed at the centres of
exactly these lines, at every deltapix and in float32 and float64 alike, and nowhere else:
    zero_neg_alone/{spread,single_bin,two_valued}   at every length (the middle pair is -0.0, every filler is non-zero)
    zeros_neg_pair/{spread,single_bin,two_valued}   at lengths 1 and 2 (the line is [-0.0] or [-0.0, -0.0]; longer lines
                                                    hold a +0.0 and are compared by value)
and at the filler bad pixels whose partial line has the same property.  The oracle now sums the middle element(s) from +0
as numpy does."""
import numpy as np
import pytest

from tests import fixbadpix_model as fm
from tests import orderstat_cases as oc

pytestmark = pytest.mark.filterwarnings('ignore::RuntimeWarning')     # the crafted lines overflow and mix infinities

PARAMS = list(fm.params())
IDS = ['%s-d%d-n%d%s' % (dt, d, n, '-border' if b else '') for dt, d, n, b in PARAMS]


def test_the_table_holds_what_the_kernel_paths_need():
    """Both parities around each sort width (16, 32, 64 slots) and its middle, the full windows, and border cuts that fit."""
    for d, widths in ((1, (8,)), (2, (16, 24)), (3, (32, 48)), (4, (64,))):
        ns = fm.LENGTHS[('float32', d)]
        for w in widths:
            assert w in ns and (w - 1 in ns or w + 1 in ns), (d, w)
        assert {n % 2 for n in ns} == {0, 1} and max(ns) == fm.capacity(d, 'inside') and min(ns) > fm.capacity(d - 1, 'inside')
        corner, edge = fm.capacity(d, 'corner'), fm.capacity(d, 'edge')
        assert (corner, edge) == ((d + 1) ** 2 - 1, (d + 1) * (2 * d + 1) - 1)
        assert fm.BORDER_LENGTHS[d] == (corner - 1, corner, edge - 1, edge)
    assert {d for dt, d in fm.LENGTHS if dt == 'float64'} == {1, 2, 3, 4}


def test_packer_puts_each_line_into_its_window_in_order():
    rng = np.random.default_rng(3)
    for d in (1, 2, 4):
        for border in (False, True):
            n = fm.capacity(d, 'corner' if border else 'inside') - 1
            lines = [rng.normal(size=n).astype(np.float32) for _ in range(11)]
            for slots in fm.SLOTS:
                data, mask, centres = fm.pack(lines, d, slots, border, mask_value=255)
                assert set(np.unique(mask)) == {0, 255} and len({tuple(c) for c in centres}) == len(lines)
                for j, (r, c) in enumerate(centres):
                    assert mask[r, c] and np.array_equal(fm.good_values(data, mask != 0, r, c, d), lines[j]), (d, border, slots, j)
                if border:
                    H, W = data.shape
                    assert all(r in (0, H - 1) or c in (0, W - 1) for r, c in centres)
                    assert sum(r in (0, H - 1) and c in (0, W - 1) for r, c in centres) == 4
    # first and last slots differ where the block has room to spare
    a = fm.pack([np.arange(3, dtype=np.float32)], 1, 'first')
    b = fm.pack([np.arange(3, dtype=np.float32)], 1, 'last')
    assert np.flatnonzero(a[1] == 0).tolist() == [0, 1, 2] and np.flatnonzero(b[1] == 0).tolist() == [6, 7, 8]
    with pytest.raises(ValueError):
        fm.pack([np.zeros(9, np.float32)], 1)


def test_rule_takes_nan_before_the_zero_rule():
    z = np.array([0.0], np.float32)
    nan = np.array([np.nan], np.float32)
    t, f = np.array([True]), np.array([False])
    assert not fm.same(z, z, t, t)[0][0] and fm.same(nan, z, t, t)[0][0]          # a NaN window asks for NaN, zeros or not
    assert fm.same(-z, z, f, t)[0][0] and fm.same(-z, z, f, t)[1][0]              # mixed zeros: by value
    assert not fm.same(-z, z, f, f)[0][0] and not fm.same(z + 1, z, f, t)[0][0]   # otherwise the sign counts
    assert fm.same(nan, nan, f, f)[0][0] and not fm.same(nan, nan, f, f)[1][0]


@pytest.mark.parametrize('dt,d,n,border', PARAMS, ids=IDS)
def test_model_at_the_centres_is_the_median_by_construction(dt, d, n, border):
    p = fm.packed(dt, d, n, border)
    assert len(p.cases) == (1 if border else 2) * len(list(oc.cases(np.dtype(dt).type, n)))
    got = p.out[p.centres[:, 0], p.centres[:, 1]]
    for g, c, (r, col) in zip(got, p.cases, p.centres):
        assert p.mask[r, col] != 0 and p.nan_window[r, col] == c.has_nan
        if c.has_nan:
            assert np.isnan(g), (c.name, g)
        else:
            assert oc.same_median(g, c), (c.name, g, c.expected)
            assert p.zeros_mixed[r, col] == c.zero_sign_free or c.expected != 0, c.name
    # and the array form of the rule agrees with the catalogue's
    want, nan_line, zsf = fm.centre_expectations(p)
    ok, by_value = fm.same(got, want, nan_line, zsf)
    assert ok.all() and by_value.sum() == (zsf & ~nan_line).sum()
    assert p.stats[0] == int((p.mask != 0).sum()) and p.stats[1] + p.stats[2] == p.stats[0]


def _oracle_diff(p, apref):
    """Names of what differs between the oracle's repair of a packed image and the model's."""
    ref, st = apref.fix_badpix(p.data, p.mask, p.deltapix, p.min_valid)
    assert ref.dtype == p.out.dtype
    ok, _ = fm.same(ref, p.out, p.nan_window, p.zeros_mixed)
    assert ok[p.mask == 0].all(), 'a good pixel changed'
    names = {(int(r), int(c)): '%s[%s]' % (case.name, s) for (r, c), case, s in zip(p.centres, p.cases, p.slots)}
    bad = [names.get((int(r), int(c)), 'filler(%d,%d)' % (r, c)) for r, c in np.argwhere(~ok)]
    return bad, (st['nbad'], st['nfix'], st['nrem'])


@pytest.mark.parametrize('dt,d,n,border', PARAMS, ids=IDS)
def test_oracle_equals_the_model_at_every_bad_pixel(dt, d, n, border):
    from oracle import apref
    p = fm.packed(dt, d, n, border)
    bad, stats = _oracle_diff(p, apref)
    assert stats == p.stats
    assert not bad, '%d of %d bad pixels differ: %s' % (len(bad), p.stats[0], sorted(set(bad))[:12])


# -- the packed cases catch a wrong median ------------------------------------------------------------------------------
def _upper_middle(good):
    """np.median, but the upper middle element alone for an even count."""
    s = np.sort(good)
    return np.nan if np.isnan(good).any() else good.dtype.type(0) + s[good.size // 2]


def _no_plus_zero(good):
    """np.median, but the middle element(s) not summed from +0."""
    if np.isnan(good).any():
        return np.nan
    s = np.sort(good)
    k = good.size // 2
    return s[k] if good.size % 2 else good.dtype.type(s[k - 1] + s[k]) / good.dtype.type(2)


MUTANTS = {_upper_middle: ('lower_pos/', 'lower_neg/', 'boundary_b0_pos/', 'overflow_pos/', 'inf_opposite/'),
           _no_plus_zero: ('zero_neg_alone/',)}


@pytest.mark.parametrize('dt,d,n', [('float32', 1, 4), ('float32', 1, 5), ('float32', 2, 16), ('float32', 3, 33),
                                    ('float32', 4, 80), ('float64', 1, 4), ('float64', 2, 23), ('float64', 4, 80)])
def test_each_wrong_median_fails_named_cases(dt, d, n, capsys):
    """The mutant x failing-case table.  The upper middle alone shows only at an even count; the missing +0 at every count."""
    p = fm.packed(dt, d, n)
    lines = []
    for mutant, must in MUTANTS.items():
        out, stats = fm.repair(p.data, p.mask, d, p.min_valid, median=mutant)
        assert stats == p.stats
        got = out[p.centres[:, 0], p.centres[:, 1]]
        want, nan_line, zsf = fm.centre_expectations(p)
        ok, _ = fm.same(got, want, nan_line, zsf)
        failed = sorted({c.name for c, o in zip(p.cases, ok) if not o})
        lines.append('%-14s %s d=%d n=%2d: %3d cases fail, e.g. %s' % (mutant.__name__, dt, d, n, len(failed), failed[:3]))
        if mutant is _upper_middle and n % 2:
            assert not failed, failed[:5]                        # an odd count has one middle: the variant is np.median there
            continue
        for prefix in must:
            assert any(f.startswith(prefix) for f in failed), (mutant.__name__, prefix, failed[:8])
        # and through the whole-image rule, as the GPU test applies it
        ok_all, _ = fm.same(out, p.out, p.nan_window, p.zeros_mixed)
        assert not ok_all.all()
    with capsys.disabled():
        print('\n' + '\n'.join(lines))
