"""The catalogue of tests/orderstat_cases.py, checked without a GPU: every case's median is what its construction says (against
numpy itself), every boundary pair straddles its key bit, and the catalogue tells a right selection from a subtly wrong one:
plain Python models of the library's selections (digit-wise radix select with 8-bit digits, 11-bit digits and the 11/11/10
split; the rank-counting / bitwise search) pass every case, and each mutant of them fails at least one named case.  That is
the evidence that tests/test_gpu_orderstat.py, which runs the same cases through the kernels, would notice such a kernel."""
import warnings

import numpy as np
import pytest

from tests import orderstat_cases as oc

DTYPES = (np.float32, np.float64, np.uint16)
SIZES = (1, 2, 3, 4, 5, 24, 25, 33, 599, 600, 601)
MA_PATH_LEN = 600                   # numpy's _nanmedian: lines shorter than this go through np.ma.median
RANK_SLOTS = 24                     # the rank-counting regime of the bitwise model holds this many values


@pytest.fixture(scope='module')
def catalogue():
    return {(dt, n): list(oc.cases(dt, n)) for dt in DTYPES for n in SIZES}


# -- the catalogue against numpy ------------------------------------------------------------------------------------
def test_every_median_is_the_one_the_construction_predicts(catalogue):
    total = 0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)          # inf - inf in the +-inf pair, overflow in the FLT_MAX pairs
        for (dt, n), cs in catalogue.items():
            names = [c.name for c in cs]
            assert len(set(names)) == len(names), 'case names repeat'
            for c in cs:
                name, values = c
                assert values.size == n and values.dtype == dt
                if dt is np.uint16:
                    assert not c.has_nan and not c.has_inf
                assert c.n_valid == n - int(np.isnan(values).sum() if c.has_nan else 0)
                got = np.nanmedian(values) if c.has_nan else np.median(values)
                assert oc.same_median(got, c), (dt.__name__, n, name, got, c.expected)
                # by construction, in key order: n_valid // 2 - 1 values at or below lo, then lo, hi, the rest at or above hi
                v = values[~np.isnan(values)] if c.has_nan else values
                if c.n_valid > 1:
                    key = (lambda a: a.astype(np.int64)) if dt is np.uint16 else oc.order_key
                    kv, klo, khi = key(v), key(np.array([c.lo]))[0], key(np.array([c.hi]))[0]
                    nb, na = c.n_valid // 2 - 1, c.n_valid - c.n_valid // 2 - 1
                    assert (kv < klo).sum() <= nb and (kv > khi).sum() <= na
                    if c.strict:
                        assert (kv < klo).sum() == nb and (kv > khi).sum() == na
                total += 1
    assert total > 5000


def test_overflow_pairs_and_the_600_value_switch_as_numpy_has_them():
    """numpy returns inf for a middle pair whose sum overflows, and np.nanmedian along an axis also for an odd line shorter
    than 600 (np.ma.median forms (x + x) / 2); from 600 values on the odd line's median is the finite middle value."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        for dt in (np.float32, np.float64):
            for n, want_inf in ((2, True), (3, True), (599, True), (600, True), (601, False)):
                c = [c for c in oc.cases(dt, n) if c.name.startswith('overflow_pos/spread/')][0]
                got = np.nanmedian(c.values[None, :], axis=1)[0]
                assert np.isinf(got) == want_inf, (dt.__name__, n, got)
                assert np.isinf(c.expected) == (n % 2 == 0)


def _py_key(x):
    """OrderKey restated: the bits, inverted for a negative value, the sign bit set for the others."""
    bits = x.dtype.itemsize * 8
    b = int(x.view({32: np.uint32, 64: np.uint64}[bits]))
    return (~b) & ((1 << bits) - 1) if b >> (bits - 1) else b | (1 << (bits - 1))


def test_boundary_pairs_straddle_their_bit():
    for dt in (np.float32, np.float64):
        bits = np.dtype(dt).itemsize * 8
        seen = set()
        for c in oc.cases(dt, 4):
            if c.kind != 'boundary':
                continue
            klo, khi = _py_key(c.lo), _py_key(c.hi)
            assert klo < khi and (klo >> c.bit) != (khi >> c.bit), c.name
            if c.bit == bits - 1:
                assert c.lo == -np.finfo(dt).smallest_subnormal and c.hi == np.finfo(dt).smallest_subnormal
                assert not (c.values == 0).any(), 'the sign pair has no zero in its line'
            else:
                assert khi - klo == 1 and khi & ((1 << c.bit) - 1) == 0 and (khi >> c.bit) & 1, c.name
                assert np.isfinite(c.lo) and np.isfinite(c.hi) and c.lo != 0 and c.hi != 0
            assert int(oc.order_key(np.array([c.hi], dt))[0]) == khi
            seen.add(c.bit)
        assert seen == set(oc.boundary_bits(dt))
    assert set(oc.boundary_bits(np.float32)) == set(range(32))
    # every digit boundary of the 8-bit, the 11-bit and the 11/11/10 selections of both key widths
    for bits, dt in ((32, np.float32), (64, np.float64)):
        need = set(range(0, bits, 8)) | set(range(bits - 11, 0, -11)) | ({10, 21} if bits == 32 else set())
        assert need <= set(oc.boundary_bits(dt)), (bits, sorted(need - set(oc.boundary_bits(dt))))
    for c in oc.cases(np.uint16, 4):
        if c.kind == 'boundary':
            assert int(c.lo) + 1 == int(c.hi) == 1 << c.bit


# -- models of the selections ---------------------------------------------------------------------------------------
def _model_keys(values, mut):
    """(keys as uint64, bits, float dtype) of the values a selection ranks; uint16 is widened to float64 as the kernels do."""
    v = values.astype(np.float64) if values.dtype == np.uint16 else values
    if mut != 'nan_counted':
        v = v[~np.isnan(v)]
    bits = v.dtype.itemsize * 8
    keys = oc.order_key(v).astype(np.uint64)
    if mut == 'sign_not_flipped':                                  # a negative value keeps its sign bit
        keys = np.where(np.signbit(v), keys | np.uint64(1 << (bits - 1)), keys)
    if mut == 'signed_compare':                                    # the unsigned order of k ^ sign is the signed order of k
        keys = keys ^ np.uint64(1 << (bits - 1))
    return keys, bits, v.dtype.type


def _finish(khi, klo, n, bits, dt, mut, line_len=None, ma_len=None):
    """numpy's arithmetic on the selected keys: the mean of the middle element(s), summed from +0."""
    if mut == 'signed_compare':
        khi, klo = khi ^ (1 << (bits - 1)), klo ^ (1 << (bits - 1))
    hi, lo = oc.key_values([khi, klo], dt)
    with np.errstate(over='ignore', invalid='ignore'):
        if n % 2:
            if ma_len is not None and line_len < ma_len:
                return dt(dt(0) + hi + hi) / dt(2)
            return dt(0) + hi
        return dt(dt(0) + lo + hi) / dt(2)


def radix_median(values, widths, mut=None, ma_len=None):
    """Median by a digit-wise radix select on the keys, digits of `widths` bits from the top: the upper middle element by
    histogram and rank, the lower one of an even count from (a) the same key when the rank left in the last bin is >= 1,
    (b) the highest occupied lower bin of the last digit, (c) the largest key below, searched over the whole line."""
    keys, bits, dt = _model_keys(values, mut)
    n = keys.size
    if n == 0:
        return dt(np.nan)
    assert sum(widths) == bits
    k = n // 2
    if mut == 'odd_rank_low' and n % 2:
        k = max(n // 2 - 1, 0)
    sel, prefix, used, lo_digit = keys, 0, 0, -1
    for w in widths:
        shift = np.uint64(bits - used - w)
        digits = ((sel >> shift) & np.uint64((1 << w) - 1)).astype(np.int64)
        hist = np.bincount(digits, minlength=1 << w)
        cum = np.cumsum(hist)
        pick = int(np.searchsorted(cum, k, side='right'))
        occupied = np.flatnonzero(hist[:pick])
        lo_digit = int(occupied[-1]) if occupied.size else -1
        k -= int(cum[pick - 1]) if pick else 0
        prefix = (prefix << w) | pick
        sel = sel[digits == pick]
        used += w
    khi, last = prefix, widths[-1]
    klo = khi
    if n % 2 == 0:
        if k >= 1 or mut == 'upper_again':
            klo = khi
        elif lo_digit >= 0 and mut != 'lower_bin_skipped':
            klo = (khi & ~((1 << last) - 1)) | lo_digit
        else:
            below = keys[keys < np.uint64(khi)]
            if mut == 'lower_bin_skipped':                         # only keys under a lower prefix are looked at
                below = below[(below >> np.uint64(last)) < np.uint64(khi >> last)]
            if mut == 'below_under_prefix':                        # only keys under the current prefix are looked at
                below = below[(below >> np.uint64(last)) == np.uint64(khi >> last)]
            klo = int(below.max()) if below.size else khi
    return _finish(khi, klo, n, bits, dt, mut, values.size, ma_len)


def _select_bitwise(keys, k, bits, mut):
    """select_key: rank counting while the values fit its RANK_SLOTS slots, a bitwise search on the key above that."""
    n = keys.size
    if n <= RANK_SLOTS + (1 if mut == 'switch_at_25' else 0):
        held = keys[:RANK_SLOTS]
        for ki in held:
            less, eq = int((held < ki).sum()), int((held == ki).sum())
            if less <= k < less + eq:
                return int(ki)
        return 0
    ans = 0
    for b in range(bits - 1, -1, -1):
        cand = ans | (1 << b)
        if int((keys < np.uint64(cand)).sum()) <= k:
            ans = cand
    return ans


def bitwise_median(values, mut=None):
    keys, bits, dt = _model_keys(values, mut)
    n = keys.size
    if n == 0:
        return dt(np.nan)
    k = n // 2
    if mut == 'odd_rank_low' and n % 2:
        k = max(n // 2 - 1, 0)
    khi = _select_bitwise(keys, k, bits, mut)
    klo = khi if n % 2 or mut == 'upper_again' else _select_bitwise(keys, n // 2 - 1, bits, mut)
    return _finish(khi, klo, n, bits, dt, mut)


def _widths(bits):
    return {'radix8': (8,) * (bits // 8),
            'radix11': (11,) * (bits // 11) + ((bits % 11,) if bits % 11 else ()),
            'radix11_11_10': (11, 11, 10) if bits == 32 else (11,) * 4 + (10, 10)}


def _models(mut=None):
    """name -> callable(values): every model the mutant applies to."""
    out = {}
    if mut not in ('switch_at_25', 'ma_switch_599', 'ma_switch_601'):
        for name in ('radix8', 'radix11', 'radix11_11_10'):
            out[name] = lambda v, name=name: radix_median(v, _widths(64 if v.dtype != np.float32 else 32)[name], mut)
    if mut not in ('lower_bin_skipped', 'below_under_prefix', 'ma_switch_599', 'ma_switch_601'):
        out['bitwise'] = lambda v: bitwise_median(v, mut)
    return out


def _axis_model(values, ma_len):
    """The axis median: the 8-bit radix select with numpy's np.ma.median arithmetic for lines shorter than ma_len."""
    return radix_median(values, _widths(64 if values.dtype != np.float32 else 32)['radix8'], None, ma_len)


def _numpy_axis(values):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return np.nanmedian(values[None, :], axis=1)[0]


def test_models_pass_every_case(catalogue):
    bad = []
    for (dt, n), cs in catalogue.items():
        for c in cs:
            for name, f in _models().items():
                got = f(c.values)
                if not oc.same_median(got, c):
                    bad.append((dt.__name__, n, c.name, name, got, c.expected))
            if n >= 599 or n <= 4:
                got = _axis_model(c.values, MA_PATH_LEN)
                want = _numpy_axis(c.values)
                if not oc.same_median(got, c, want):
                    bad.append((dt.__name__, n, c.name, 'axis', got, want))
    assert not bad, bad[:10]


MUTANTS = {
    'upper_again': 'lower middle taken as the upper one again whenever the rank opens its bin',
    'lower_bin_skipped': 'lower-bin lookup skipped: straight to the largest key under a lower prefix',
    'below_under_prefix': '"largest key below" searched only under the current prefix',
    'odd_rank_low': 'rank n // 2 - 1 used for odd n',
    'signed_compare': 'keys compared as signed integers',
    'sign_not_flipped': 'sign bit not flipped for negatives',
    'nan_counted': 'NaN counted as a value',
    'switch_at_25': 'rank counting (24 slots) still used for 25 values',
    'ma_switch_599': 'np.ma.median arithmetic below 599 values instead of 600',
    'ma_switch_601': 'np.ma.median arithmetic below 601 values instead of 600',
}


def _first_catch(mut, catalogue):
    for (dt, n), cs in catalogue.items():
        for c in cs:
            if mut.startswith('ma_switch'):
                got = _axis_model(c.values, int(mut[-3:]))
                if not oc.same_median(got, c, _numpy_axis(c.values)):
                    return 'axis', dt.__name__, n, c.name
                continue
            for name, f in _models(mut).items():
                if not oc.same_median(f(c.values), c):
                    return name, dt.__name__, n, c.name
    return None


def test_every_mutant_fails_a_named_case(catalogue, capsys):
    """The mutant x first-catching-case table.  (A switch to the bitwise search one value early, at 23, computes the same
    medians and is no fault; the switch one value late drops the 25th value from the 24 slots.  Likewise the np.ma.median
    arithmetic differs from np.median's only for an odd count, so the 601 mutant shows on a line of 600 values with one NaN.)"""
    caught = {m: _first_catch(m, catalogue) for m in MUTANTS}
    lines = ['%-20s %-10s %-8s %5s  %s' % ('mutant', 'model', 'dtype', 'n', 'first case that fails')]
    for m, hit in caught.items():
        lines.append('%-20s %-10s %-8s %5s  %s' % ((m,) + (hit if hit else ('-', '-', '-', 'SURVIVES'))))
    with capsys.disabled():
        print('\n' + '\n'.join(lines))
    assert all(caught.values()), [m for m, hit in caught.items() if not hit]
    # and per model: each mutant is caught in every model it applies to, not only in the first
    for m in MUTANTS:
        if m.startswith('ma_switch'):
            continue
        for name in _models(m):
            hit = any(not oc.same_median(_models(m)[name](c.values), c) for cs in catalogue.values() for c in cs)
            assert hit, (m, name)


# -- a wrong median inside a sigma clip -----------------------------------------------------------------------------
def _clip_survivors(x, median, sigma=3.0, maxiters=5):
    """tests/util.np_clip_stats with the median as a parameter."""
    x = x[np.isfinite(x)]
    for _ in range(maxiters):
        if x.size == 0:
            break
        with np.errstate(all='ignore'):
            med, sd = median(x), np.nanstd(x)
            lo = x.dtype.type(np.float64(med) - np.float64(sd) * sigma)
            hi = x.dtype.type(np.float64(med) + np.float64(sd) * sigma)
        y = x[(x >= lo) & (x <= hi)]
        if y.size == x.size:
            break
        x = y
    return x


CLIP_MUTANTS = {'upper_again': lambda v: bitwise_median(v, 'upper_again'),          # both regimes of select_key
                'lower_bin_skipped': lambda v: radix_median(v, (8,) * (v.dtype.itemsize), 'lower_bin_skipped'),
                'lower_again': lambda v: v.dtype.type(0) + np.sort(v)[v.size // 2 - 1]}  # the lower middle element taken twice
# A boundary pair above bit 0 is two neighbouring values whose mean rounds to the even one, hi: there 'upper_again' IS numpy's
# median, and the lower-bin mutant is not reached (8-bit digits: lo lies under another prefix); 'lower_again' is one ulp off.
CLIP_MUST_CHANGE = {'lower_pos': ('upper_again', 'lower_bin_skipped', 'lower_again'),
                    'lower_neg': ('upper_again', 'lower_bin_skipped', 'lower_again'),
                    'boundary_b0_pos': ('upper_again', 'lower_bin_skipped'),          # the even one is lo here
                    'boundary_b8_pos': ('lower_again',)}


@pytest.mark.parametrize('window', (22, 24, 48))
def test_a_planted_value_makes_the_clip_depend_on_the_median(window, capsys):
    """The sliding statistics return mean, std and flag, not the median.  orderstat_cases.plant puts one value on the first
    clip bound of its own line; with it a median that takes the upper or the lower middle element twice, or skips the lower bin, keeps
    other survivors on named lower_* and boundary_b* lines of an even count - 22 and 24 values (select_key counts ranks; 24
    is the last count that does) and 48 (it searches bitwise); the upper_again mutant runs through the model of both
    regimes.  These are the counts the windows of 23, 25 and 49 of tests/test_gpu_orderstat.py hold next to one inf."""
    from tests.util import np_clip_stats
    lines = []
    for dt in (np.float32, np.float64):
        cs = {c.name.rsplit('/', 1)[0]: c for c in oc.cases(dt, window) if not c.has_nan}
        for pair in ('lower_pos/two_valued', 'lower_neg/two_valued', 'boundary_b0_pos/two_valued', 'boundary_b8_pos/two_valued',
                     'boundary_b8_pos/single_bin'):
            c = cs[pair]
            for mut, median in CLIP_MUTANTS.items():
                changed = []
                for kind in oc.PLANT_KINDS:
                    v, p = oc.plant(c, kind)
                    assert p is not None, (pair, kind)
                    right = _clip_survivors(v, np.median)
                    assert np.array_equal(right, np_clip_stats(v))
                    assert np.array_equal(right, _clip_survivors(v, lambda x: bitwise_median(x)))
                    wrong = _clip_survivors(v, median)
                    if wrong.size != right.size:
                        changed.append('%s %d -> %d' % (kind, right.size, wrong.size))
                lines.append('%-8s %-28s %-18s %s' % (dt.__name__, c.name, mut, ', '.join(changed) or 'UNCHANGED'))
                assert bool(changed) == (mut in CLIP_MUST_CHANGE[pair.split('/')[0]]), (dt.__name__, window, c.name, mut, changed)
    with capsys.disabled():
        print('\nwindow %d: survivors with the right median -> with the mutant\n' % window + '\n'.join(lines))
