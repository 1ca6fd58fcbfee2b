"""The conformance table of the exact order statistics: crafted lines whose median is known by construction (numpy only).

Every exact median or quantile of the library selects on the order-preserving key of csrc/np_exact.h (OrderKey) or sorts.
For an even count the lower middle element is (a) the same key again, (b) a lower bin of the last digit or (c) a key under
another prefix; continuous random data practically never takes (a) or (b) and never puts the pair across a high digit
boundary.  cases(dtype, n) yields lines built around a chosen middle pair instead.

A case is the tuple (name, values) with values.size == n, and carries as attributes what the construction knows:

    lo, hi          the middle pair (odd valid count: hi alone is the median; lo is then the value just below it)
    expected        the median by construction, in numpy's arithmetic: 0 + hi for an odd count, dtype(0 + lo + hi) / 2 for an
                    even one (float64 for uint16; numpy's mean of the middle elements starts from +0, so a median of -0.0
                    is +0.0).  np.median / np.nanmedian of the 1-D line return exactly this.
    n_valid         values that are not NaN (sets the parity)
    has_nan, has_inf
    bit             the key bit the pair straddles (boundary pairs), else None
    kind            'boundary' | 'same' | 'lower' | 'special'
    pair, core      the pair's name; core: one of the few pairs that meet every order, the +-inf fillers and the NaNs
    strict          True: every filler lies strictly below lo or strictly above hi.  False only where no such value exists
                    (-inf, 0 or 65535 as part of the pair) or where the middle value is repeated on purpose.
    zero_sign_free  the median is a zero and the line holds zeros of both signs.  numpy's partition compares -0.0 == +0.0,
                    so which zero it returns depends on the element order (np.median([0., -0., -0.]) is +0.0), while the key
                    order puts -0.0 below +0.0.  Such a case is compared by value (the result must be a zero); every other
                    case is compared bit for bit.  This is the only place the rule is stated.

Layout of a line (ascending): n // 2 - 1 fillers below lo, lo, hi, n - n // 2 - 1 fillers above hi; for an odd n that makes
hi the element of rank n // 2.  n = 1 is [hi].

Floating-point pairs, all derived in key space from the bit position alone (no kernel constant appears here):
    boundary  hi = the key near 1.5 (and near -1.5) whose b low bits are zero and whose bit b is set, lo = key(hi) - 1, for
              every bit of the float32 key and for every multiple of 8 and of 11, plus 64 - 11 j, 10, 21 and 63, of the float64 key:
              every digit boundary of an 8-bit, an 11-bit and an 11/11/10 radix select.  The sign bit is the pair
              (-denorm_min, +denorm_min), no zero in the line.
    same      the middle value occurs 2, 3, n // 2 and n times; positive, negative, first and last key of its 256-group and of
              its 2048-group
    lower     lo is 5 keys below hi inside one 256-group
    special   subnormal pairs on both sides of zero, pairs whose sum overflows the dtype, +-inf as the middle pair, zeros of
              both signs around the middle, and -0.0 (+0.0) as the middle pair of a line without the other zero
Fillers: 'spread' (evenly spaced keys over -2^40 .. 2^40: many binades, both signs, a finite std), 'single_bin' (inside the top 11
key bits of the pair, so a first-level histogram of 8 or 11 bits has one occupied bin), 'two_valued' (one value below, one
above) and, for the core pairs, 'spread_inf' (the whole finite range, -inf and +inf at its ends).  Orders: ascending, descending, a seeded
permutation and 'above_first'; every pair meets each layout, the order rotates, and the core pairs meet every order.
NaN cases: the core pairs with 1 and 2 NaNs at the start, in the middle or at the end of the line, so that n_valid and not n
sets the parity.

uint16 pairs: (2^b - 1, 2^b) for b = 0 .. 15, equal pairs, the extremes 0 and 65535; layouts 'spread', 'two_valued' and the
constant line."""
import numpy as np

ORDERS = ('asc', 'desc', 'perm', 'above_first')
FLOAT_LAYOUTS = ('spread', 'single_bin', 'two_valued')
SPREAD_MAX = 2.0 ** 40            # 'spread' fillers: 80 binades and the subnormals of both signs, squares that stay finite
TOP_BITS = 11                       # the widest first digit of the selections: 'single_bin' fills one such bin


class Case(tuple):
    """(name, values) with the construction's knowledge as attributes."""

    def __new__(cls, name, values, **attrs):
        self = super().__new__(cls, (name, values))
        self.name, self.values = name, values
        for k, v in attrs.items():
            setattr(self, k, v)
        return self


# -- keys -----------------------------------------------------------------------------------------------------------
def _spec(dtype):
    dtype = np.dtype(dtype).type
    return {np.float32: (32, np.uint32), np.float64: (64, np.uint64)}[dtype]


def order_key(x):
    """OrderKey<T>::to: the unsigned key with a < b <=> key(a) < key(b); -0.0 just below +0.0.  Returns an unsigned array."""
    x = np.ascontiguousarray(x)
    bits, U = _spec(x.dtype)
    b = x.view(U)
    sign = U(1 << (bits - 1))
    return np.where(b & sign, ~b, b | sign)


def key_values(keys, dtype):
    """OrderKey<T>::from for a sequence of keys (Python ints or an unsigned array)."""
    bits, U = _spec(dtype)
    k = keys.astype(U) if isinstance(keys, np.ndarray) else np.array([int(v) for v in keys], dtype=U)
    sign = U(1 << (bits - 1))
    return np.where(k & sign, k & ~sign, ~k).astype(U).view(dtype)


def _key1(x, dtype):
    return int(order_key(np.array([x], dtype))[0])


# -- floating-point pairs -------------------------------------------------------------------------------------------
def boundary_bits(dtype):
    bits, _ = _spec(dtype)
    if bits == 32:
        return list(range(32))
    # 11-bit digits counted from the bottom (0, 11, ..) and from the top (53, 42, 31, 20, 9)
    return sorted(set(range(0, 64, 8)) | set(range(0, 64, 11)) | set(range(53, 0, -11)) | {10, 21, 63})


def _float_pairs(dtype):
    """dicts: name, klo, khi, kind, bit, core, dup (how often the middle value occurs: int, 'half' or 'all'), pad_below /
    pad_above (keys placed next to the pair before the fillers)."""
    bits, _ = _spec(dtype)
    fi = np.finfo(dtype)
    off = 0x2AAAAA if bits == 32 else 0x2AAAAAAAAAAAA            # low bits of every kind, still inside [1.5, 2)
    base_p = _key1(1.5, dtype) + off
    base_n = _key1(-1.5, dtype) - off
    kz_n, kz_p = _key1(-0.0, dtype), _key1(0.0, dtype)

    def pair(name, klo, khi, kind, bit=None, core=False, dup=2, pad_below=(), pad_above=()):
        return dict(name=name, klo=klo, khi=khi, kind=kind, bit=bit, core=core, dup=dup, pad_below=tuple(pad_below),
                    pad_above=tuple(pad_above))

    core_bits = (0, 8, 11, 21) if bits == 32 else (0, 8, 11, 53)
    for b in boundary_bits(dtype):
        if b == bits - 1:
            yield pair('boundary_b%d_sign' % b, kz_n - 1, kz_p + 1, 'boundary', b, core=True)
            continue
        for tag, base in (('pos', base_p), ('neg', base_n)):
            khi = (base & ~((1 << (b + 1)) - 1)) | (1 << b)
            yield pair('boundary_b%d_%s' % (b, tag), khi - 1, khi, 'boundary', b, core=(b in core_bits and tag == 'pos'))
    keys = (('pos', base_p), ('neg', base_n), ('first256', base_p & ~0xFF), ('last256', base_p | 0xFF),
            ('first2048', base_p & ~0x7FF), ('last2048', base_p | 0x7FF))
    for tag, k in keys:
        for dup in (2, 3, 'half', 'all'):
            yield pair('same_%s_x%s' % (tag, dup), k, k, 'same', dup=dup, core=(tag == 'first256' and dup == 2))
    for tag, base in (('pos', base_p), ('neg', base_n)):
        khi = (base & ~0xFF) + 7
        yield pair('lower_%s' % tag, khi - 5, khi, 'lower', core=(tag == 'pos'))
    # special values
    yield pair('subnormal_pos', kz_p + 1, kz_p + 2, 'special')
    yield pair('subnormal_neg', kz_n - 2, kz_n - 1, 'special')
    big, mid = dtype(fi.max) * dtype(0.75), dtype(fi.max) * dtype(0.625)
    yield pair('overflow_pos', _key1(mid, dtype), _key1(big, dtype), 'special', core=True)
    yield pair('overflow_neg', _key1(-big, dtype), _key1(-mid, dtype), 'special')
    kinf_n, kinf_p = _key1(-np.inf, dtype), _key1(np.inf, dtype)
    yield pair('inf_hi', _key1(mid, dtype), kinf_p, 'special')
    yield pair('inf_lo', kinf_n, _key1(-mid, dtype), 'special')
    yield pair('inf_both_pos', kinf_p, kinf_p, 'special')
    yield pair('inf_both_neg', kinf_n, kinf_n, 'special')
    yield pair('inf_opposite', kinf_n, kinf_p, 'special')
    yield pair('zeros_mixed', kz_n, kz_p, 'special', core=True, pad_below=(kz_n, kz_n), pad_above=(kz_p, kz_p))
    yield pair('zero_neg_alone', kz_n, kz_n, 'special')           # no +0.0 in the line: numpy's median of -0.0 is +0.0
    yield pair('zero_pos_alone', kz_p, kz_p, 'special')
    yield pair('zeros_neg_pair', kz_n, kz_n, 'special', pad_below=(kz_n,), pad_above=(kz_p, kz_p))
    yield pair('zeros_pos_pair', kz_p, kz_p, 'special', pad_below=(kz_n, kz_n), pad_above=(kz_p,))


def _span(k0, k1, count):
    """count keys (uint64, ascending) spread evenly over [k0, k1]; repeats when the range is shorter than count.  The spacing
    is worked out in float64, good enough for fillers: every key is clamped into the range."""
    if count <= 0:
        return np.zeros(0, np.uint64)
    if count == 1:
        return np.array([(k0 + k1) // 2], np.uint64)
    width = k1 - k0
    off = np.floor(float(width) * (np.arange(count) / (count - 1)))
    off = np.minimum(off, np.nextafter(float(width), 0.0) if width >= 2 ** 53 else float(width)).astype(np.uint64)
    return np.uint64(k0) + off


def _fillers(p, layout, nb, na, dtype):
    """Keys of nb fillers below klo and na above khi; where no finite value lies beyond the pair, copies of it."""
    bits, _ = _spec(dtype)
    fi = np.finfo(dtype)
    kmin, kmax = _key1(-fi.max, dtype), _key1(fi.max, dtype)
    klo, khi = p['klo'], p['khi']
    low = (1 << (bits - TOP_BITS)) - 1
    if layout == 'spread_inf':
        b0, b1, a0, a1 = kmin, klo - 1, khi + 1, kmax
    elif layout == 'spread':                                     # -2^40 .. 2^40, or out to the pair where it lies beyond
        b0, b1 = min(_key1(-SPREAD_MAX, dtype), klo - 1), klo - 1
        a0, a1 = khi + 1, max(_key1(SPREAD_MAX, dtype), khi + 1)
        if b0 < kmin or a1 > kmax:                               # an infinite pair: no value beyond it
            b0, a1 = max(b0, kmin), min(a1, kmax)
    elif layout == 'single_bin':
        b0, b1, a0, a1 = max(klo & ~low, kmin), klo - 1, khi + 1, min(khi | low, kmax)
    elif layout == 'two_valued':
        b0 = b1 = max(klo - 4099, kmin)
        a0 = a1 = min(khi + 4099, kmax)
    else:
        raise ValueError(layout)
    kz_n, kz_p = _key1(-0.0, dtype), _key1(0.0, dtype)
    if khi == kz_n and a0 == kz_p:                               # the zero of the other sign is no filler: only a pair's
        a0 += 1                                                  # pads bring it in
    if klo == kz_p and b1 == kz_n:
        b1 -= 1
    below = _span(b0, b1, nb) if b0 <= b1 < klo else np.full(max(nb, 0), klo, np.uint64)
    above = _span(a0, a1, na) if khi < a0 <= a1 else np.full(max(na, 0), khi, np.uint64)
    if layout == 'spread_inf':
        if below.size:
            below[0] = _key1(-np.inf, dtype)
        if above.size:
            above[-1] = _key1(np.inf, dtype)
    return below, above


def _arrange(below, lo, hi, above, order, seed):
    # below and above arrive in ascending key order (np.sort would not do: it may hand back either zero for the other)
    asc = np.concatenate([below, [lo, hi], above]).astype(below.dtype)
    if order == 'asc':
        return asc
    if order == 'desc':
        return asc[::-1].copy()
    if order == 'perm':
        return np.random.default_rng(seed).permutation(asc)
    if order == 'above_first':
        return np.concatenate([above, [hi], below, [lo]]).astype(below.dtype)
    raise ValueError(order)


def _median_by_construction(lo, hi, n_valid, dtype):
    # np.median is np.mean of the middle element(s), and numpy's sum of fewer than 8 values starts from +0: a median of
    # -0.0 comes out as +0.0
    if n_valid % 2:
        return dtype(0) + dtype(hi)
    with np.errstate(over='ignore', invalid='ignore'):
        return dtype(dtype(0) + dtype(lo) + dtype(hi)) / dtype(2)


def _make(name, vals, lo, hi, p, strict, out_dtype=None):
    dtype = vals.dtype.type
    valid = vals[~np.isnan(vals)] if vals.dtype.kind == 'f' else vals
    exp = _median_by_construction(lo, hi, valid.size, out_dtype or dtype)
    zeros = valid[valid == 0]
    zsf = bool(exp == 0 and zeros.size and vals.dtype.kind == 'f' and np.signbit(zeros).any() and not np.signbit(zeros).all())
    return Case(name, vals, lo=lo, hi=hi, expected=exp, n_valid=int(valid.size), has_nan=bool(valid.size != vals.size),
                has_inf=bool(vals.dtype.kind == 'f' and np.isinf(vals).any()), bit=p['bit'], kind=p['kind'], strict=strict,
                zero_sign_free=zsf, pair=p['name'], core=bool(p.get('core')))


def _float_line(p, layout, order, n, dtype, seed):
    """The line of n values (no NaN) for pair p; returns (values, lo, hi, strict)."""
    lo, hi = key_values([p['klo'], p['khi']], dtype)
    if n == 1:
        return np.array([hi], dtype), lo, hi, True
    nb, na = n // 2 - 1, n - n // 2 - 1
    dup = {'half': max(n // 2, 2), 'all': n}.get(p['dup'], p['dup'])
    dup = min(dup, n)
    extra = dup - 2                                              # further copies of the middle value: above first, then below
    pad_above = ([p['khi']] * min(na, (extra + 1) // 2) if extra > 0 else list(p['pad_above'][:na]))
    pad_below = ([p['klo']] * min(nb, extra - len(pad_above)) if extra > 0 else list(p['pad_below'][:nb]))
    if extra > 0 and len(pad_above) + len(pad_below) < extra:   # one side is full: the rest goes to the other
        pad_above += [p['khi']] * min(na - len(pad_above), extra - len(pad_above) - len(pad_below))
    fb, fa = _fillers(p, layout, nb - len(pad_below), na - len(pad_above), dtype)
    kb = np.concatenate([fb, np.array(pad_below, np.uint64)])
    ka = np.concatenate([np.array(pad_above, np.uint64), fa])
    strict = bool((kb < np.uint64(p['klo'])).all() and (ka > np.uint64(p['khi'])).all())
    below, above = key_values(kb, dtype), key_values(ka, dtype)
    return _arrange(below, lo, hi, above, order, seed), lo, hi, strict


def _nan_positions(n, k, where):
    if where == 'start':
        return list(range(k))
    if where == 'end':
        return list(range(n - k, n))
    return [n // 2 - 1 + i for i in range(k)] if n >= 2 else [0]


def _float_cases(dtype, n):
    pairs = list(_float_pairs(dtype))
    for i, p in enumerate(pairs):
        for j, layout in enumerate(FLOAT_LAYOUTS):
            order = ORDERS[(i + j) % 4]
            vals, lo, hi, strict = _float_line(p, layout, order, n, dtype, seed=1000 * i + j)
            yield _make('%s/%s/%s' % (p['name'], layout, order), vals, lo, hi, p, strict)
        if not p['core']:
            continue
        for order in ORDERS:
            if order != ORDERS[i % 4]:                           # that one is the 'spread' case above
                vals, lo, hi, strict = _float_line(p, 'spread', order, n, dtype, seed=1000 * i + 7)
                yield _make('%s/spread/%s' % (p['name'], order), vals, lo, hi, p, strict)
        vals, lo, hi, strict = _float_line(p, 'spread_inf', 'perm', n, dtype, seed=1000 * i + 8)
        yield _make('%s/spread_inf/perm' % p['name'], vals, lo, hi, p, strict)
        # NaNs: the count of valid values, n - k, sets the parity
        for k in (1, 2):
            if n - k < 1:
                continue
            for w, where in enumerate(('start', 'middle', 'end')):
                layout = FLOAT_LAYOUTS[(i + w) % 3]
                v, lo, hi, strict = _float_line(p, layout, 'perm', n - k, dtype, seed=1000 * i + 10 * k + w)
                vals = np.empty(n, dtype)
                pos = _nan_positions(n, k, where)
                keep = np.ones(n, bool)
                keep[pos] = False
                vals[~keep] = np.nan
                vals[keep] = v
                yield _make('%s/%s/nan%d_%s' % (p['name'], layout, k, where), vals, lo, hi, p, strict)


# -- uint16 ---------------------------------------------------------------------------------------------------------
def _u16_pairs():
    for b in range(16):
        yield dict(name='u16_b%d' % b, klo=(1 << b) - 1, khi=1 << b, kind='boundary', bit=b, dup=2)
    for v in (0, 1, 255, 256, 32768, 65535):
        for dup in (2, 'half', 'all'):
            yield dict(name='u16_same_%d_x%s' % (v, dup), klo=v, khi=v, kind='same', bit=None, dup=dup)
    yield dict(name='u16_top', klo=65534, khi=65535, kind='special', bit=None, dup=2)
    yield dict(name='u16_extremes', klo=0, khi=65535, kind='special', bit=None, dup=2)


def _u16_cases(n):
    for i, p in enumerate(_u16_pairs()):
        for j, layout in enumerate(('spread', 'two_valued')):
            if p['dup'] == 'all' and j:
                continue                                         # the constant line has no fillers
            order = ORDERS[(i + j) % 4]
            lo, hi = np.uint16(p['klo']), np.uint16(p['khi'])
            if n == 1:
                vals, strict = np.array([hi], np.uint16), True
            else:
                nb, na = n // 2 - 1, n - n // 2 - 1
                dup = min({'half': max(n // 2, 2), 'all': n}.get(p['dup'], p['dup']), n)
                extra = dup - 2
                pa = min(na, (extra + 1) // 2)
                pb = min(nb, extra - pa)
                pa += min(na - pa, extra - pa - pb)
                klo, khi = p['klo'], p['khi']
                if layout == 'spread':
                    fb = _span(0, klo - 1, nb - pb) if klo > 0 else np.full(nb - pb, klo, np.uint64)
                    fa = _span(khi + 1, 65535, na - pa) if khi < 65535 else np.full(na - pa, khi, np.uint64)
                else:
                    fb = np.full(nb - pb, max(klo - 3, 0), np.uint64)
                    fa = np.full(na - pa, min(khi + 3, 65535), np.uint64)
                below = np.concatenate([fb, np.full(pb, klo, np.uint64)]).astype(np.uint16)
                above = np.concatenate([np.full(pa, khi, np.uint64), fa]).astype(np.uint16)
                strict = bool((below < klo).all() and (above > khi).all())
                vals = _arrange(below, lo, hi, above, order, seed=500 + 10 * i + j)
            yield _make('%s/%s/%s' % (p['name'], layout, order), vals, lo, hi, p, strict, out_dtype=np.float64)


# -- the catalogue --------------------------------------------------------------------------------------------------
def cases(dtype, n):
    """Yield every case of the catalogue as a line of n values of dtype (float32, float64 or uint16), n >= 1."""
    dtype = np.dtype(dtype).type
    if n < 1:
        raise ValueError('n must be >= 1')
    gen = _u16_cases(n) if dtype is np.uint16 else _float_cases(dtype, n)
    for c in gen:
        assert c.values.size == n and c.values.dtype == dtype, (c.name, c.values.size, c.values.dtype)
        yield c


def same_median(got, case, want=None):
    """The comparison rule: bit-equal (NaN equals NaN), except that a zero_sign_free case only has to return a zero.
    want defaults to the median by construction."""
    want = case.expected if want is None else want
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype:
        return False
    if case.zero_sign_free:
        return bool(got == 0 and want == 0)
    if np.isnan(want):
        return bool(np.isnan(got))
    return got.tobytes() == want.tobytes()


# -- a value on the clip bound ------------------------------------------------------------------------------------------
PLANT_KINDS = ('up_out', 'up_in', 'down_out', 'down_in')


def first_bounds(v, sigma=3.0):
    """The first bounds astropy's clip forms for the finite values of v: median -+ sigma std in float64, demoted to the dtype."""
    x = v[np.isfinite(v)]
    with np.errstate(all='ignore'):
        med, sd = np.float64(np.median(x)), np.float64(np.std(x))
        return v.dtype.type(med - sd * sigma), v.dtype.type(med + sd * sigma)


def plant(case, kind, sigma=3.0):
    """The case's line with its largest value (kind 'up_*') or its smallest ('down_*') replaced by the value that sits on the
    first clip bound of the line that contains it: '*_in' is the last value of the dtype the bound keeps, '*_out' the first
    it removes.  A clip whose median is off by an ulp or two keeps or removes the other way.  The value is found by
    bisection over the dtype's keys (the bound moves with it: the line's std contains the planted value), and it stays
    beyond the middle pair, so the median by construction holds.  Returns (line, index of the planted value) or (line unchanged, None)
    where no such value exists: fewer than 12 finite values (one value among n lies at most (n - 1) / sqrt(n) std from
    the median's side of the mean, 3.015 for n = 11), a std that is not finite, no filler on that side."""
    v = case.values.copy()
    dt = v.dtype.type
    fin = np.isfinite(v)
    up = kind.startswith('up')
    if fin.sum() < 12 or v.dtype.kind != 'f':
        return v, None
    j = int(np.argmax(np.where(fin, v, -np.inf))) if up else int(np.argmin(np.where(fin, v, np.inf)))
    if not (v[j] > case.hi if up else v[j] < case.lo):
        return v, None

    def kept(k):                                                 # the bound of the line holding key k keeps that value
        v[j] = key_values([k], dt)[0]
        lo, hi = first_bounds(v, sigma)
        return np.isfinite(lo) and np.isfinite(hi) and (v[j] <= hi if up else v[j] >= lo)

    # bisect between a key next to the pair (kept) and one far out (removed); keys grow with the value
    near = int(order_key(np.array([case.hi if up else case.lo], dt))[0]) + (1 if up else -1)
    with np.errstate(all='ignore'):
        scale = max(abs(float(case.hi)), abs(float(case.lo)), float(np.std(v[fin])), float(np.finfo(dt).tiny))
    far = _key1(dt((1 if up else -1) * min(scale * 2.0 ** 30, float(np.finfo(dt).max) / 2.0 ** 40)), dt)
    ok = kept(near) and not kept(far)
    while ok and abs(far - near) > 1:
        mid = (near + far) // 2
        near, far = (mid, far) if kept(mid) else (near, mid)
    if not ok:
        v[j] = case.values[j]
        return v, None
    v[j] = key_values([near if kind.endswith('in') else far], dt)[0]
    return v, j
