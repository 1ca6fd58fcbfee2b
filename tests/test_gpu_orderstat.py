"""Every exact median and quantile of the library on the crafted lines of tests/orderstat_cases.py (the conformance table:
middle pairs on every key-bit boundary, repeated middle values, lower-bin pairs, subnormals, overflowing pairs, infinities,
zeros of both signs, NaNs that set the parity; tests/test_orderstat_cases_host.py shows that the table catches a subtly wrong
selection).  One parametrised test per op; each op is held to the reference its own tests use.

Which branch each group of cases exists for (the lower middle element of an even count: (a) the same key, (b) a lower bin
of the last digit, (c) a key under another prefix):

axis_nanmedian - csrc/autobadcol.hip, axis_median_kernel, 8-bit digits
    (a) :127 `s.k >= 1`            same_*_x2 / x3 / xhalf / xall (the upper middle is not the first of its key)
    (b) :128 `lo_digit >= 0`       lower_pos, lower_neg, boundary_b0 .. b7 (the pair differs inside the last digit)
    (c) :132-142 `need_below`      boundary_b8 .. b31: lo lives under another prefix of the first three digits; b31 is the
                                   sign pair (-denorm_min, +denorm_min); with 'single_bin' fillers every earlier histogram
                                   is one bin
    :153 odd, `len < 600`          overflow_pos / overflow_neg at 599 and at 601 with two NaNs (x + x overflows: inf), at 601
                                   and at 600 with one NaN (np.median: finite); :87 NaN dropped: */nan1_*, */nan2_*
    :156 `(0 + lo + hi) / 2`       subnormal_pos / _neg, boundary_b31_sign (no flush to zero), overflow_* (inf),
                                   inf_opposite (NaN), zero_neg_alone (+0.0, see below)
sliding_clipped_stats - csrc/autobadcol.hip, select_key :200 `n <= 24` rank counting / :213-220 bitwise search
    windows 3, 11, 23 and the one-sided windows of 24 values (lengths 47, 49; NaN cases of 25) count ranks; 25, 47, 49, 129,
    301 and the one-sided windows of 25 search bitwise.  Both regimes: (a) same_* (`less <= k < less + eq` with eq >= 2; the
    search returns the same key for ranks n/2 - 1 and n/2), (b) lower_*, (c) boundary_b*: the two ranks differ in bit b, the
    bit at which the search's `less <= k` decision separates them.  A window has an odd length, so every case also runs as
    window - 1 values next to one inf, which the op drops: the even count that takes the lower middle.  From 22 values on every line with a finite std gets one
    value planted on the first clip bound of the line that contains it (orderstat_cases.plant: the last value the bound
    keeps or the first it removes, asserted here against the reference's own bound), so a median off by an ulp or two
    changes who survives; tests/test_orderstat_cases_host.py shows that on named lower_* and boundary_b* lines of 23 and 25
    values.  Windows of 3 and 11 cannot hold a value 3 std out, nothing is planted there.  (median_of's own zero sign is
    not observable: the median only feeds the bounds.)
sigclip_global - csrc/sigclip_global.hip, median_of_pick, 11-bit digits (float32: last digit 10 bits)
    (a) :392 `pk.newk >= 1`        same_first256_x2 in four orders, every same_*/single_bin
    (b) :393 `pk.dlow >= 0`        lower_pos in four orders, boundary_b0_pos, boundary_b8_pos (float32: inside the last
                                   10 bits), every boundary_b0 .. b9 / single_bin
    (c) :394 `below`               boundary_b11_pos, boundary_b21_pos (float32), boundary_b53_pos (float64), boundary_b31_sign,
                                   every boundary_b10 .. b31 / single_bin (level 0's histogram has one occupied bin)
    and the special values (subnormal_*, overflow_*, inf_*, zeros_*), at one piece, one piece + 1 and 3 pieces + 10.  The
    plain pairs in random fillers are in test_sigclip_global_median_neighbours.  The zero sign of this op's median is not
    pinned: the values are compared with ==, as that test does, and median_of_pick returns -0.0 for a median of -0.0.
box_clipped_stats - csrc/background.hip, box_stats_kernel's key1 :463-469
    (a) `kk - pk.cum > 0`: same_*; (b) :464 `pk.dlow >= 0`: lower_*, boundary_b0 .. b9; (c) :466-468 the largest key below
    the 22-bit prefix: boundary_b10 .. b31.  The speculated second level (:425 `prefix == g0`) hits with 'single_bin'
    fillers and misses with 'spread' ones.  8 x 8 and 64 x 64: 256-thread resident; 100 x 100: 1024-thread resident;
    200 x 200: non-resident.
quantile_levels - csrc/composite.hip, level_pick_kernel :138-150
    the two targets are ranks n/2 - 1 and n/2: (a) same_* (both targets end in one bin of every level), (b) lower_*,
    boundary_b0 .. b7 (they part at the last level), (c) boundary_b8 .. b31 (they part at an earlier level, b >= 24 at the
    first, whose histogram they share :110).
aperture_photometry - csrc/findstars.hip, block_select :226-241, block_median :244-250
    ranks n/2 and n/2 - 1 by two searches: (a) same_*, (b) lower_*, (c) boundary_b*; 144 (even) and 123 (odd) annulus pixels.
stack_median / stack_sigclip - csrc/stack_sort.h networks, csrc/stack_reduce.h pick_middle :653, median :809 / :1060,
    csrc/stack_chunks.hip rank chunks: a sort has no (a) / (b) / (c); the cases are ties (same_*), neighbours in the last bit
    (boundary_b0), sign and zero order (boundary_b31_sign, zeros_*), inf and NaN padding.  Largest distance of an even-count
    median from the oracle over all kernels: 0 ulp (float32 and uint16; the family allows 1).
sepmedfilt - csrc/lacosmic.hip medians of 5 / 7 / 9: same_* (ties), zeros_*, subnormal_*, boundary_b* in every window position.
fix_badpix - csrc/fixbadpix.hip, repair_window<1 / 2 / 3> (sort + pick_at) and repair_pixel<float / double> (rank counting):
    the same catalogue laid into repair windows, in a module of its own with its own reference (np.median through
    tests/fixbadpix_model.py): tests/test_gpu_fixbadpix.py, which lists its branches the same way.

Found and fixed with this module: axis_median_kernel and block_median returned -0.0 for a median of -0.0 (a line whose
middle values are -0.0, no +0.0 in it) where np.nanmedian and np.median return +0.0 - numpy's mean of the middle element(s)
starts its sum from +0.  Exposed by zeros_neg_pair at lengths 1 and 2 (axis_nanmedian, both axes, float32 and float64) and by
inf_both_pos / inf_both_neg (annulus: the finite rest of the line has -0.0 as its median); zero_neg_alone now states the case
at every length.  Both kernels add the middle element(s) to +0 as numpy does; sigclip_global's median (compared by value
here) and the stack's (held to its own oracle) are left as they are.  Also found: tests/util.np_clip_stats formed the
clip bounds in the data's dtype, where astropy under the reference's numpy - and the kernels, csrc/autobadcol.hip :269 -
forms them in float64 and demotes them; with sigma = 1e300 a constant float32 window gave 0 * inf = NaN bounds in the
restatement.  It now forms them as tests/findstars_model.annulus_clip does.

On one MI355X the module ran in 22.5 s (66 tests, the slowest 1.1 s) next to 108 s for the rest of `-m gpu`, which is the suite of
the parent commit.
"""
import warnings

import numpy as np
import pytest

from tests import composite_model as cm
from tests import findstars_model as fm
from tests import orderstat_cases as oc
from tests.util import assert_biteq, np_clip_stats, ulp_diff

# the crafted lines overflow and mix infinities on purpose: numpy's warnings about that are no finding
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings('ignore::RuntimeWarning')]

torch = pytest.importorskip('torch')

# Cases an op cannot take, each with its reason.  Nothing else is left out: every test counts the (case, shape) pairs it
# compared and asserts the count against the catalogue's minus this table.  (The catalogue has no NaN or inf case for
# uint16: the type holds neither.)
EXCLUDED = {
    'sepmedfilt': (lambda c: c.has_nan, "astroscrappy's median filter defines no result for a window holding NaN "
                                        '(ApFixCosmicRays zeroes and masks non-finite pixels first)'),
}


# How many cases the catalogue holds, written down here and not derived from it: (without NaN, with NaN) per dtype for lines
# of 3 or more values.  A line of 2 has half the NaN cases (one NaN only), a line of 1 none.  A case that vanishes from the
# catalogue, or from an op's loop, fails the op's count.
CATALOGUE = {np.float32: (345, 54), np.float64: (279, 54), np.uint16: (66, 0)}


def _expected(op, dtype, n):
    plain, nan = CATALOGUE[dtype]
    nan = {1: 0, 2: nan // 2}.get(n, nan)
    return plain + (0 if op == 'sepmedfilt' else nan)                       # the one row of EXCLUDED


def _catalogue(op, dtype, n):
    """(cases the op runs, how many it must compare): the whole catalogue but for the op's row of EXCLUDED."""
    drop = EXCLUDED.get(op, (lambda c: False, ''))[0]
    return [c for c in oc.cases(dtype, n) if not drop(c)], _expected(op, dtype, n)


def _dev(a):
    from astrophotography_amd import ops
    if a.dtype == np.uint16:
        return ops.to_device_u16(a)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(got, want):
    """Elementwise: the same bits, or both NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    v = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(v) == want.view(v)) | (np.isnan(got) & np.isnan(want))


def _same(got, want, zsf):
    """The catalogue's comparison rule for arrays: bits, but a zero_sign_free case (zsf) only has to return a zero."""
    return _bits_equal(got, want) | (zsf & (got == 0) & (want == 0))


def _report(ok, cases, got, want, what):
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, '%s: %d of %d cases differ: %s' % (
        what, bad.size, ok.size, [(cases[i].name, got.ravel()[i], want.ravel()[i]) for i in bad[:6]])


# ---- axis_nanmedian -----------------------------------------------------------------------------------------------------
AXIS_LENGTHS = (1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 599, 600, 601, 1200)
LINES = 37                  # neither a multiple of the 32 columns nor of the 4 rows a workgroup owns


@pytest.mark.parametrize('axis', (0, 1))
@pytest.mark.parametrize('dtype', (np.float32, np.float64, np.uint16))
def test_axis_nanmedian(dtype, axis):
    """One case per line, 37 lines per frame, the frames of one length in one slab; np.nanmedian of the same slab, bit-equal.
    Lengths on both sides of numpy's 600-value switch; the NaN cases of length 601 have 600 and 599 valid values."""
    from astrophotography_amd import ops
    ran = expect = 0
    for n in AXIS_LENGTHS:
        cases, count = _catalogue('axis_nanmedian', dtype, n)
        expect += count
        lines = cases + cases[:-len(cases) % LINES]                        # the last frame is filled up from the start
        slab = np.stack([c.values for c in lines]).reshape(-1, LINES, n)    # [frames, 37 lines, n]
        if axis == 0:
            slab = np.ascontiguousarray(slab.transpose(0, 2, 1))            # lines are columns
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            want = np.nanmedian(slab, axis=1 + axis).ravel()
        got = ops.axis_nanmedian(_dev(slab), axis).cpu().numpy().ravel()
        zsf = np.array([c.zero_sign_free for c in lines])
        ok = _same(got, want, zsf)
        _report(ok, lines, got, want, '%s axis %d length %d' % (np.dtype(dtype).name, axis, n))
        ran += len({c.name for c in lines[:ok.size]})                         # distinct cases compared
        if n in (599, 600, 601) and dtype != np.uint16:
            assert any(c.has_nan and c.n_valid == n - 1 for c in cases) and any(c.has_nan and c.n_valid == n - 2 for c in cases)
    assert ran == expect


# ---- sliding_clipped_stats ----------------------------------------------------------------------------------------------
WINDOWS = (3, 11, 23, 25, 47, 49, 129, 301)
PER_LINE = 3


# windows -> lines (odd and even counts together) that get a value planted on their first clip bound (orderstat_cases.plant),
# float32 / float64.  One value among
# n lies at most (n - 1) / sqrt(n) standard deviations out: 1.15 for 3 values and 3.015 for 11, so a 3-sigma bound can hold a
# planted value only in the longer windows; there every line with a finite std and a filler on the planted side gets one
# (not: the constant lines, the +-inf pairs, the 'spread_inf' lines, whose std overflows).
PLANTED = {3: (0, 0), 11: (0, 0), 23: (640, 508), 25: (640, 508), 47: (640, 508), 49: (640, 508), 129: (640, 508), 301: (640, 508)}


def _window_ref(x, sigma, maxiters):
    s = np_clip_stats(x, sigma, maxiters)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        if s.size == 0:
            return np.nan, np.nan
        return np.float64(np.nanmean(s)), np.float64(np.nanstd(s))


@pytest.mark.parametrize('window', WINDOWS)
@pytest.mark.parametrize('dtype', (np.float32, np.float64))
def test_sliding_clipped_stats(dtype, window):
    """Lines of three cases end to end, all lines in one batched call: every case as a line of `window` values (an odd
    count) and as a line of `window` - 1 values with one inf among them, which the op drops (an even count: the window
    takes the lower middle element too).  Checked against the numpy
    restatement of astropy's clip (tests/util.np_clip_stats): the window centred on every case (it holds exactly that case),
    the first and last window of every line, and the one-sided windows of 24 and of 25 values at both ends of every line
    (window lengths 47 and 49 have them; 25 is also the full window of 25, and its NaN cases leave 24 values inside the
    line).  mean, std and flag bit-equal, sigma 3 / maxiters 5, and window 25 once more with sigma 1e300."""
    from astrophotography_amd import ops
    hw = (window - 1) // 2
    planted, names, count, nplanted = [], [], 0, 0
    for n in (window, window - 1):                                          # an odd count, and an even one next to one inf
        cases, c_n = _catalogue('sliding_clipped_stats', dtype, n)
        count += c_n
        for i, c in enumerate(cases):
            v, j = oc.plant(c, oc.PLANT_KINDS[i & 3])
            if j is not None:
                # the planted value sits on the first bound the reference forms for this very line: the bound keeps an
                # '_in' value and not the next value of the dtype, removes an '_out' value and not the one before
                up, inside = i & 3 < 2, i & 1 == 1
                other = v.copy()
                other[j] = np.nextafter(v[j], dtype(np.inf if up == inside else -np.inf))
                keeps = [(lambda b, x: b[0] <= x <= b[1])(oc.first_bounds(w), w[j]) for w in (v, other)]
                assert keeps == [inside, not inside], (c.name, n, oc.PLANT_KINDS[i & 3], v[j], oc.first_bounds(v))
                nplanted += 1
            planted.append(v if n == window else np.insert(v, i % window, dtype(np.inf)))
            names.append('%s (%d values)' % (c.name, n))
    assert nplanted == PLANTED[window][dtype == np.float64], (nplanted, PLANTED[window])
    planted += planted[:-len(planted) % PER_LINE]                              # the last line is filled up from the start
    names += names[:len(planted) - len(names)]
    lines = np.stack(planted).reshape(-1, PER_LINE * window)
    B, L = lines.shape
    pos = {t * window + hw for t in range(PER_LINE)} | {0, L - 1}
    for size in (24, 25):                                                  # window [0, i + hw] has i + hw + 1 values
        if hw + 1 <= size < window:
            pos |= {size - hw - 1, L - 1 - (size - hw - 1)}
    pos = sorted(pos)
    d = _dev(lines)
    for sigma in (3.0, 1e300) if window == 25 else (3.0,):
        r = {k: t.cpu().numpy() for k, t in ops.sliding_clipped_stats(d, window, sigma=sigma, maxiters=5).items()}
        want_mean, want_std = np.empty((B, len(pos))), np.empty((B, len(pos)))
        for b in range(B):
            for j, i in enumerate(pos):
                want_mean[b, j], want_std[b, j] = _window_ref(lines[b, max(0, i - hw):i + hw + 1], sigma, 5)
        with np.errstate(all='ignore'):
            nsig = np.abs(lines[:, pos].astype(np.float64) - want_mean) / want_std
        what = '%s window %d sigma %g' % (np.dtype(dtype).name, window, sigma)
        assert_biteq(r['mean'][:, pos], want_mean, what + ' mean')
        assert_biteq(r['std'][:, pos], want_std, what + ' std')
        assert_biteq(r['nsig'][:, pos], nsig, what + ' nsig')
        assert np.array_equal(r['flag'][:, pos], (nsig >= 5.0).astype(np.uint8)), what + ' flag'
        centres = [pos.index(t * window + hw) for t in range(PER_LINE)]
        compared = len(set(names[:want_mean[:, centres].size]))               # distinct cases whose own window was compared
    assert compared == count, (compared, count)


# ---- sigclip_global -----------------------------------------------------------------------------------------------------
GLOBAL_SIZES = (2, 3, 6, 8192, 8193, 3 * 8192 + 10)
# cases of the subset below, written down: lines of 3 or more values; a line of 2 has only the one-NaN half of the NaN cases
GLOBAL_SUBSET = {np.float32: 235, np.float64: 213, np.uint16: 66}
GLOBAL_NAN_HALF = {np.float32: 27, np.float64: 27, np.uint16: 0}


def _global_subset(c):
    """The special-value, single-bin-filler and order cases (test_sigclip_global_median_neighbours has the plain pairs)."""
    return c.kind == 'special' or '/single_bin/' in c.name or c.core or c.values.dtype == np.uint16


@pytest.mark.parametrize('n', GLOBAL_SIZES)
@pytest.mark.parametrize('dtype', (np.float32, np.float64, np.uint16))
def test_sigclip_global(dtype, n):
    """mean / median / std / survivors / iterations equal to the oracle's, as test_sigclip_global_median_neighbours asserts
    them (values compared with ==, so the zero rule holds by itself; NaN equals NaN), without and with clipping."""
    from astrophotography_amd import ops
    from oracle import apref
    cases, count = _catalogue('sigclip_global', dtype, n)
    sub = [c for c in cases if _global_subset(c)]
    assert len(cases) == count
    ran = 0
    cast = np.float32 if dtype == np.float32 else np.float64
    for c in sub:
        d = _dev(c.values)
        for sigma, maxiters in ((1e300, 1), (3.0, 5)):
            with np.errstate(all='ignore'):
                ref = apref.sigclip_global(c.values, sigma=sigma, maxiters=maxiters)
            s = ops.sigclip_global(d, sigma=sigma, maxiters=maxiters).cpu().numpy()
            got = [cast(v) for v in s[:3]]
            want = [cast(ref[k]) for k in ('mean', 'median', 'std')]
            same = [g == w or (np.isnan(g) and np.isnan(w)) for g, w in zip(got, want)]
            assert all(same), (c.name, n, sigma, got, want)
            assert int(s[6]) == ref['nkeep'] and int(s[5]) == ref['niter'], (c.name, n, sigma, s[5:7], ref)
        ran += 1
    assert ran == GLOBAL_SUBSET[dtype] - (GLOBAL_NAN_HALF[dtype] if n == 2 else 0), ran


# ---- box_clipped_stats --------------------------------------------------------------------------------------------------
# box -> (odd count, even count) of the interior boxes; the half boxes of the ragged last row and column hold 7 and 8 values
BOXES = {(8, 8): (61, 60), (64, 64): (1501, 1500), (100, 100): (2601, 2600), (200, 200): (33001, 33000)}
BOX_SETTINGS = ((3.0, 5), (1e30, 0), (2.0, 10))
RAGGED_COUNTS = (7, 8)


def _box_image(cases_by_count, bh, bw):
    """An image of whole boxes, one case each (its values first, in row-major order, the rest of the box masked), with a
    ragged last row and column of half boxes that hold the short cases.  Returns (image, mask, [(case, by, bx)])."""
    (n1, whole), (n3, c3), (n4, c4) = cases_by_count
    nx = 24 if bh <= 64 else 12
    ny = -(-len(whole) // nx)
    short = [c for pair in zip(c3, c4) for c in pair]
    H, W = ny * bh + bh // 2, nx * bw + bw // 2
    img = np.full((H, W), 1.0, np.float32)
    mask = np.ones((H, W), np.uint8)
    placed = []

    def put(c, by, bx, h, w):
        box = np.full(h * w, 1.0, np.float32)
        m = np.ones(h * w, np.uint8)
        box[:c.values.size] = c.values
        m[:c.values.size] = 0
        img[by * bh:by * bh + h, bx * bw:bx * bw + w] = box.reshape(h, w)
        mask[by * bh:by * bh + h, bx * bw:bx * bw + w] = m.reshape(h, w)
        placed.append((c, by, bx))

    for i, c in enumerate(whole):
        put(c, i // nx, i % nx, bh, bw)
    edge = [(ny, bx, bh // 2, bw) for bx in range(nx)] + [(by, nx, bh, bw // 2) for by in range(ny)] + [(ny, nx, bh // 2, bw // 2)]
    for (by, bx, h, w), c in zip(edge, short):
        assert h * w >= c.values.size
        put(c, by, bx, h, w)
    return img, mask, placed


@pytest.mark.parametrize('parity', (1, 0))
@pytest.mark.parametrize('box', sorted(BOXES))
def test_box_clipped_stats(box, parity):
    """One case per box, the mask trimming the box to the case's count; all cases at an odd (parity 1) or an even count in the
    whole boxes, and as many short cases as there are ragged boxes at the image's lower and right edge.  Survivor count,
    masked count and median exact, std to 1e-12 (tests/test_gpu_boxstats_golden.py)."""
    from astrophotography_amd import ops
    from oracle import background_ref as br
    bh, bw = box
    counts = (BOXES[box][1 - parity],) + RAGGED_COUNTS
    by_count = [(n,) + _catalogue('box_clipped_stats', np.float32, n) for n in counts]
    img, mask, placed = _box_image([(n, cs) for n, cs, _ in by_count], bh, bw)
    assert sum(1 for c, _, _ in placed if c.values.size == counts[0]) == by_count[0][2]
    d, m = _dev(img), _dev(mask)
    for sigma, maxiters in BOX_SETTINGS:
        with np.errstate(all='ignore'):
            med, std, nfin, nm0 = br.box_clipped_stats(img, mask, bh, bw, sigma, maxiters)
        st = ops.box_clipped_stats(d, m, bh, bw, sigma=sigma, maxiters=maxiters).cpu().numpy()
        what = 'boxes %dx%d sigma %g maxiters %d' % (bh, bw, sigma, maxiters)
        assert np.array_equal(st[..., 2].astype(np.int64), nfin), what + ': survivor counts'
        assert np.array_equal(st[..., 3].astype(np.int64), nm0), what + ': masked counts'
        zsf = np.zeros(med.shape, bool)
        for c, by, bx in placed:
            zsf[by, bx] = c.zero_sign_free
        ok = _same(st[..., 0], med, zsf)
        assert ok.all(), '%s: medians differ: %s' % (what, [(c.name, st[by, bx, 0], med[by, bx]) for c, by, bx in placed if not ok[by, bx]][:6])
        assert np.array_equal(np.isnan(st[..., 1]), np.isnan(std)), what + ': NaN std'
        f = np.isfinite(std)
        assert np.array_equal(st[..., 1][~f & ~np.isnan(std)], std[~f & ~np.isnan(std)]), what + ': infinite std'
        err = np.abs(st[..., 1][f] - std[f])
        assert np.all(err <= 1e-12 * std[f]), '%s: std off by %.3e (relative)' % (what, float(np.max(err / np.maximum(std[f], 1e-300))))


# ---- quantile_levels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (2, 3, 1024, 1025, 4097))
def test_quantile_levels(n):
    """Planes [3, 1, n], one case per channel; both targets the median's upper element (q = 0.5), and the two middle elements
    as the two targets, which share the first histogram.  tests/composite_model.quantile_levels, bit-equal (the model sorts
    the same keys, so -0.0 and +0.0 are told apart on both sides and no zero rule is needed)."""
    from astrophotography_amd import ops
    cases, count = _catalogue('quantile_levels', np.float32, n)
    fill = cases + cases[:-len(cases) % 3]
    ran = 0
    for i in range(0, len(fill), 3):
        planes = np.stack([c.values for c in fill[i:i + 3]]).reshape(3, 1, n)
        d = _dev(planes)
        for q in ((0.5, 0.5), ((n // 2 - 1) / (n - 1), (n // 2) / (n - 1))):
            want, want_n = cm.quantile_levels(planes, [q] * 3)
            levels, nf = ops.quantile_levels(d, [q] * 3)
            got = levels.cpu().numpy()
            assert _bits_equal(got, want).all() and np.array_equal(nf.cpu().numpy(), want_n), (
                [c.name for c in fill[i:i + 3]], n, q, got, want)
        ran += 3
    assert ran - (len(fill) - len(cases)) == count


# ---- aperture_photometry ------------------------------------------------------------------------------------------------
# (fwhm, xc, yc, annulus pixels): radii (6, 6, 9) about the centre pixel, and (5, 5, 8) about a point a little off it; the
# counts are findstars_model.annulus_values' on a 41 x 41 image, an even and an odd one (the fractions are dyadic, so that
# the centre 41 t rows further down is the same point of its field exactly)
APERTURES = ((3.0, 20.0, 20.0, 144), (2.5, 20.25, 20.125, 123))
SIDE = 41


@pytest.mark.parametrize('fwhm,xc,yc,n', APERTURES)
def test_aperture_photometry_annulus(fwhm, xc, yc, n):
    """A 41 x 41 field per case with the source in the middle, the case's values in its annulus pixels in row-major order, the
    fields stacked into one tall image (41 rows apart: no annulus or aperture reaches a neighbour).  bkg_median and the
    annulus count exact against the model, the aperture sum to the bound of tests/test_gpu_findstars.py where it is finite."""
    from astrophotography_amd import ops
    from tests.test_gpu_findstars import SKY, phot_bound
    r, r_in, r_out = fm.aperture_radii(fwhm)
    index = np.arange(SIDE * SIDE, dtype=np.float32).reshape(SIDE, SIDE)
    member = fm.annulus_values(index, xc, yc, r_in, r_out).astype(np.int64)
    assert member.size == n
    cases, count = _catalogue('aperture_photometry', np.float32, n)
    tall = np.full((len(cases), SIDE * SIDE), SKY, np.float32)
    for t, c in enumerate(cases):
        tall[t, member] = c.values
    tall = tall.reshape(len(cases) * SIDE, SIDE)
    got = {k: v.cpu().numpy() for k, v in ops.aperture_photometry(_dev(tall), [xc] * len(cases),
                                                                  [yc + SIDE * t for t in range(len(cases))], fwhm).items()}
    assert np.all(got['n_annulus'] == n)
    want = np.empty(len(cases), np.float32)
    ran = 0
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        for t, c in enumerate(cases):
            sub = tall[t * SIDE:(t + 1) * SIDE]
            ref = fm.aperture_photometry(sub, [xc], [yc], fwhm)
            want[t] = ref['bkg_median'][0]
            assert ref['n_annulus'][0] == n
            s, g = ref['aperture_sum_raw'][0], got['aperture_sum_raw'][t]
            assert np.isfinite(s) == np.isfinite(g), (c.name, s, g)
            if np.isfinite(s):
                assert abs(g - s) <= phot_bound(sub, [xc], [yc], r, ref)[0], (c.name, s, g)
            ran += 1
    zsf = np.array([c.zero_sign_free for c in cases])
    _report(_same(got['bkg_median'], want, zsf), cases, got['bkg_median'], want, 'bkg_median, %d annulus pixels' % n)
    assert ran == count


# ---- stack_median, stack_sigclip(cenfunc='median') ----------------------------------------------------------------------
STACK_PARTS = ((1, 32), (33, 64), (65, 128), (129, 512))


def _stack_names(ops, dtype, calibrated, N):
    tag = 'f32' if dtype == np.float32 else 'u16'
    return (ops.stack_kernel_name(N, tag, calibrated, median_only=True),
            ops.stack_kernel_name(N, tag, calibrated, outputs=('median', 'count'), maxiters=1))


def _check_stack_median(got, want64, cases, what, worst):
    """Odd counts exact, even counts to the 1 ulp the family documents; a zero_sign_free case by value."""
    want = want64.astype(np.float32)
    d = ulp_diff(got, want)                                                 # asserts that NaN sits where NaN is expected
    odd = np.array([c.n_valid % 2 == 1 for c in cases])[None, :]
    zsf = np.array([c.zero_sign_free for c in cases])[None, :]
    assert np.all(d <= np.where(odd, 0, 1)), '%s: %s' % (what, [(cases[j].name, got[i, j], want[i, j]) for i, j in np.argwhere(d > np.where(odd, 0, 1))[:6]])
    exact = odd & ~zsf & ~np.isnan(want)
    assert np.all(_bits_equal(got, want) | ~exact), what + ': an odd count returned the other zero'
    worst[0] = max(worst[0], int(d.max(initial=0)))


@pytest.mark.parametrize('part', STACK_PARTS)
@pytest.mark.parametrize('dtype', (np.float32, np.uint16))
def test_stack_medians(dtype, part):
    """A cube [N, 3, ncases], one case per pixel column (the three rows hold it in three rotations), ncases odd, so that the
    uint16 pair kernels get a lone last pixel; plain and with a unit calibration; one N for every distinct kernel name
    ops.stack_kernel_name returns for N = 1 .. 512, each asserted to have run.  The oracle is apref.stack_median /
    apref.stack_sigclip.  The overflow pairs: the stack forms the mean of the middle pair in float64 (stack_reduce.h:809) and
    so does its oracle, so their median is finite here where numpy's float32 median is inf; the stack is held to its oracle,
    not to numpy."""
    from astrophotography_amd import ops
    from oracle import apref
    first, last = part
    every, seen = {}, {}
    for cal in (False, True):
        for N in range(1, 513):
            for nm in _stack_names(ops, dtype, cal, N):
                every.setdefault((cal, nm), N)
    todo = sorted({N for N in every.values() if first <= N <= last})
    worst = [0]
    ran = expect = 0
    for N in todo:
        cases, count = _catalogue('stack_median', dtype, N)
        expect += count
        cols = cases if len(cases) % 2 else cases + cases[:1]
        line = np.stack([c.values for c in cols], axis=1)                   # [N, ncases]
        cube = np.ascontiguousarray(np.stack([np.roll(line, r, axis=0) for r in range(3)], axis=1))
        d = _dev(cube)
        shape = cube.shape[1:]
        zero, one, e = np.zeros(shape, np.float32), np.ones(shape, np.float32), np.zeros(N, np.float32)
        for cal in (False, True):
            calib = dict(bias=_dev(zero), dark=_dev(zero), nflat=_dev(one), exp_ratio=_dev(e)) if cal else None
            with np.errstate(all='ignore'):
                ref_in = apref.calibrate(cube, zero, zero, one, e) if cal else cube
                want = apref.stack_median(ref_in)
                wclip = apref.stack_sigclip(ref_in, sigma=1e30, maxiters=1, want=('median', 'count'))
            what = '%s N=%d %s' % (np.dtype(dtype).name, N, 'calibrated' if cal else 'plain')
            _check_stack_median(ops.stack_median(d, calib=calib).cpu().numpy(), want, cols, what + ' stack_median', worst)
            r = ops.stack_sigclip(d, sigma=1e30, maxiters=1, cenfunc='median', calib=calib, outputs=('median', 'count'))
            assert np.array_equal(r['count'].cpu().numpy(), wclip['count']), what + ' stack_sigclip count'
            _check_stack_median(r['median'].cpu().numpy(), wclip['median'], cols, what + ' stack_sigclip median', worst)
            for nm in _stack_names(ops, dtype, cal, N):
                seen[(cal, nm)] = N
        ran += len(cases)
    print('%s N %d..%d: %d stacks, largest distance of an even-count median from the oracle: %d ulp' % (
        np.dtype(dtype).name, first, last, len(todo), worst[0]))
    assert ran == expect
    missed = [k for k, N in every.items() if first <= N <= last and k not in seen]
    assert not missed, missed


# ---- sepmedfilt ---------------------------------------------------------------------------------------------------------
SEP_CASES_PER_IMAGE = 37


@pytest.mark.parametrize('size', (5, 7, 9))
def test_sepmedfilt(size):
    """Images 11 x (9 k) whose rows are all one line of cases of `size` values end to end (the row pass takes the median of
    each case in the window centred on it; the column pass then sees 11 equal rows), and their transposes (the column pass
    takes the medians).  oracle.lacosmic_ref.sepmedfilt, bit-equal in every pixel; the images that hold a zero_sign_free
    case are kept apart, and there a zero may have either sign."""
    from astrophotography_amd import ops
    from oracle import lacosmic_ref as L
    cases, count = _catalogue('sepmedfilt', np.float32, size)
    cases = sorted(cases, key=lambda c: c.zero_sign_free)                   # the zero_sign_free cases share their images
    ran = 0
    for i in range(0, len(cases), SEP_CASES_PER_IMAGE):
        group = cases[i:i + SEP_CASES_PER_IMAGE]
        row = np.full(9 * SEP_CASES_PER_IMAGE, 1.0, np.float32)
        row[:size * len(group)] = np.concatenate([c.values for c in group])
        free = any(c.zero_sign_free for c in group)
        for img in (np.tile(row, (11, 1)), np.ascontiguousarray(np.tile(row, (11, 1)).T)):
            with np.errstate(all='ignore'):
                want = L.sepmedfilt(img, size)
            got = ops.sepmedfilt(_dev(img), size).cpu().numpy()
            ok = _bits_equal(got, want) | (free & (got == 0) & (want == 0))
            assert ok.all(), ('sepmedfilt %d' % size, img.shape, [c.name for c in group][:3], np.argwhere(~ok)[:4].tolist(),
                              got[~ok][:4], want[~ok][:4])
            # the window centred on a case holds exactly that case: its median by construction
            centre = np.array([size * t + size // 2 for t in range(len(group))])
            mid = got[5, centre] if img.shape[0] == 11 else got[centre, 5]
            for t, c in enumerate(group):
                assert mid[t] == c.hi or (np.isnan(c.hi) and np.isnan(mid[t])), (c.name, mid[t], c.hi)
        ran += len(group)
    assert ran == count
