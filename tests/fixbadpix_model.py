"""The bad-pixel repair (A5, ApFixBadPixels.fix_bad_pixels) restated in plain numpy, and the packer that lays the lines of
tests/orderstat_cases.py into repair windows (numpy only).

repair() is core/ApFixBadPixels.py:388-407 and nothing else: for every pixel with mask != 0 the window
[r - d, r + d] x [c - d, c + d] is clipped to the image, the good values of the ORIGINAL data are taken in row-major order
(data_co[good_mask]) and, if there are at least min_valid of them, the pixel becomes np.median(good) in the image's dtype;
otherwise it stays.  There is no sort and no selection here: np.median is the truth, and with it numpy's arithmetic (the
mean of the middle element(s) summed from +0: a median of -0.0 is +0.0; NaN if any good value is NaN).

pack() gives every line of the catalogue one block of (2d + 1) x (2d + 1) pixels with a bad centre: the line's n values go
into n of the other slots in row-major order (the first n or the last n), so the catalogue's element order is the order
np.median sees, and the remaining slots are bad.  Those filler bad pixels see parts of their own and of the neighbouring
lines; they are repaired and compared as well.  With border=True the blocks stand against the image's corners and edges,
centre on the outermost row or column, so the window is cut: an edge block keeps (d + 1)(2d + 1) - 1 slots, a corner block
(d + 1)^2 - 1.

The comparison rule, stated here once (same()): bit for bit, NaN equal to NaN, with two exceptions taken in this order:
  1. a window whose good values hold a NaN must give NaN (this op is np.median, not np.nanmedian: the catalogue's
     expected value of a NaN line, the median of the rest, does not apply);
  2. an expected zero from a window whose good values hold zeros of both signs is compared by value
     (orderstat_cases: zero_sign_free - which zero numpy's partition hands back depends on the element order).
Taken the other way round, a line of mixed zeros with a NaN in it would be asked for a zero."""
import functools
import types

import numpy as np

from tests import orderstat_cases as oc

SLOTS = ('first', 'last')
INTERIOR = 1.5                       # good pixels that belong to no line (the inside of a border image)


# -- the reference ---------------------------------------------------------------------------------------------------
def good_values(data, bad, r, c, deltapix):
    """data_co[good_mask] of core/ApFixBadPixels.py:391-406: the window clipped to the image, good values in row-major order."""
    H, W = data.shape
    r0, r1 = max(0, r - deltapix), min(H, r + deltapix + 1)
    c0, c1 = max(0, c - deltapix), min(W, c + deltapix + 1)
    return data[r0:r1, c0:c1][~bad[r0:r1, c0:c1]]


def repair(data, mask, deltapix=1, min_valid=4, median=np.median, flags=False):
    """-> (repaired image, (nbad, nfixed, nremaining)).  median: np.median, or a wrong variant of it for the mutation check.
    flags=True appends what the comparison rule needs to know about every pixel's window: boolean maps nan_window (a good
    value is NaN) and zeros_mixed (the good values hold +0.0 and -0.0), both False where the pixel is good or not repaired."""
    data = np.asarray(data)
    assert data.ndim == 2 and data.dtype in (np.float32, np.float64) and np.shape(mask) == data.shape
    out, bad = data.copy(), np.asarray(mask) != 0
    nan_window, zeros_mixed = np.zeros(data.shape, bool), np.zeros(data.shape, bool)
    nbad = nfixed = 0
    with np.errstate(all='ignore'):
        for r, c in zip(*np.nonzero(bad)):                        # the reference's order, row-major
            good = good_values(data, bad, r, c, deltapix)
            nbad += 1
            if good.size < min_valid:
                continue
            nfixed += 1
            out[r, c] = median(good)
            if flags:
                nan_window[r, c] = np.isnan(good).any()
                sign = np.signbit(good[good == 0])
                zeros_mixed[r, c] = sign.any() and not sign.all()
    stats = (nbad, nfixed, nbad - nfixed)
    return (out, stats, nan_window, zeros_mixed) if flags else (out, stats)


# -- the comparison rule ---------------------------------------------------------------------------------------------
def bits_equal(got, want):
    v = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(v) == want.view(v)) | (np.isnan(got) & np.isnan(want))


def same(got, want, nan_window, zeros_mixed):
    """Elementwise -> (ok, by_value).  by_value marks the elements that rule 2 compared by value."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    nan_window, zeros_mixed = np.broadcast_to(nan_window, got.shape), np.broadcast_to(zeros_mixed, got.shape)
    by_value = ~nan_window & zeros_mixed & (want == 0)
    ok = np.where(nan_window, np.isnan(got), np.where(by_value, got == 0, bits_equal(got, want)))
    return ok, by_value


# -- the packer ------------------------------------------------------------------------------------------------------
def capacity(deltapix, where):
    """Slots of a block besides its centre: where = 'inside', 'edge' or 'corner'."""
    side = 2 * deltapix + 1
    return {'inside': side * side, 'edge': (deltapix + 1) * side, 'corner': (deltapix + 1) ** 2}[where] - 1


def _fill(data, mask, r0, r1, c0, c1, centre, values, slots):
    """One block: rows r0..r1-1, cols c0..c1-1, all bad but n slots (row-major, the centre left out) that hold the values."""
    rr, cc = np.mgrid[r0:r1, c0:c1]
    keep = (rr != centre[0]) | (cc != centre[1])
    rr, cc = rr[keep], cc[keep]
    n = values.size
    if n > rr.size:
        raise ValueError('a line of %d values does not fit the %d slots of the block at %s' % (n, rr.size, centre))
    assert mask[r0:r1, c0:c1].all(), 'blocks overlap'
    sel = slice(0, n) if slots == 'first' else slice(rr.size - n, rr.size)
    data[rr[sel], cc[sel]] = values
    mask[rr[sel], cc[sel]] = 0


def pack(lines, deltapix, slots='first', border=False, mask_value=1):
    """Lay the lines (1-D arrays of one dtype and one length) into one image -> (data, mask uint8, centres as an (L, 2) array
    of (row, col)); line i stands in the window of centres[i].  slots: 'first' or 'last', or one of them per line.
    border=True: the first four lines stand in the corners if they fit there, the rest by turns against the top, bottom,
    left and right edge; the inside of the image is good."""
    lines = [np.asarray(v) for v in lines]
    d, side, L = deltapix, 2 * deltapix + 1, len(lines)
    dtype, n = lines[0].dtype, lines[0].size
    slots = [slots] * L if isinstance(slots, str) else list(slots)
    assert len(slots) == L and set(slots) <= set(SLOTS) and all(v.dtype == dtype and v.shape == (n,) for v in lines)
    centres = np.zeros((L, 2), np.int64)
    if not border:
        per_row = int(np.ceil(np.sqrt(L)))
        H, W = -(-L // per_row) * side, per_row * side
        data, mask = np.zeros((H, W), dtype), np.full((H, W), mask_value, np.uint8)
        for i, v in enumerate(lines):
            r0, c0 = (i // per_row) * side, (i % per_row) * side
            centres[i] = (r0 + d, c0 + d)
            _fill(data, mask, r0, r0 + side, c0, c0 + side, centres[i], v, slots[i])
        return data, mask, centres
    corners = 4 if n <= capacity(d, 'corner') else 0
    per_edge = max(-(-(L - corners) // 4), 1)
    S = 2 * (d + 1) + per_edge * side                             # corner block, per_edge edge blocks, corner block
    data, mask = np.full((S, S), INTERIOR, dtype), np.full((S, S), mask_value, np.uint8)
    mask[d + 1:S - d - 1, d + 1:S - d - 1] = 0
    for i, v in enumerate(lines):
        if i < corners:
            top, left = i < 2, i % 2 == 0
            centres[i] = (0 if top else S - 1, 0 if left else S - 1)
            r0, c0 = (0 if top else S - d - 1), (0 if left else S - d - 1)
            _fill(data, mask, r0, r0 + d + 1, c0, c0 + d + 1, centres[i], v, slots[i])
            continue
        e, j = (i - corners) % 4, (i - corners) // 4
        a0 = d + 1 + j * side                                     # the block's first pixel along its edge
        if e < 2:                                                 # top, bottom
            r0 = 0 if e == 0 else S - d - 1
            centres[i] = (0 if e == 0 else S - 1, a0 + d)
            _fill(data, mask, r0, r0 + d + 1, a0, a0 + side, centres[i], v, slots[i])
        else:                                                     # left, right
            c0 = 0 if e == 2 else S - d - 1
            centres[i] = (a0 + d, 0 if e == 2 else S - 1)
            _fill(data, mask, a0, a0 + side, c0, c0 + d + 1, centres[i], v, slots[i])
    return data, mask, centres


def min_valid_for(n):
    """The reference's 4, or the line's length where that is shorter."""
    return min(4, n)


@functools.lru_cache(maxsize=None)
def packed(dtype_name, deltapix, n, border=False):
    """The whole catalogue at length n as one image, with its repair by the model, computed once and shared read-only:
    every case with both slot choices (border=False: 2 L blocks), or against the corners and edges (border=True: the slot
    choice alternates from line to line, and the catalogue is rotated by n so that other lines reach the corners).
    Fields: data, mask, centres, cases (one per centre), slots (one per centre), min_valid, out, stats, nan_window,
    zeros_mixed."""
    dtype = np.dtype(dtype_name).type
    cs = list(oc.cases(dtype, n))
    if not border:
        cases, slots = cs + cs, ['first'] * len(cs) + ['last'] * len(cs)
    else:
        k = n % len(cs)
        cases = cs[k:] + cs[:k]
        slots = [SLOTS[i % 2] for i in range(len(cases))]
    data, mask, centres = pack([c.values for c in cases], deltapix, slots, border)
    mv = min_valid_for(n)
    out, stats, nan_window, zeros_mixed = repair(data, mask, deltapix, mv, flags=True)
    for a in (data, mask, centres, out, nan_window, zeros_mixed):
        a.setflags(write=False)
    return types.SimpleNamespace(data=data, mask=mask, centres=centres, cases=cases, slots=slots, min_valid=mv, out=out,
                                 stats=stats, nan_window=nan_window, zeros_mixed=zeros_mixed, deltapix=deltapix, n=n)


def centre_expectations(p):
    """What the catalogue says about the centres of a packed image -> (want, nan_line, zero_sign_free), one per centre."""
    dtype = p.data.dtype.type
    want = np.array([c.expected for c in p.cases], dtype)
    return want, np.array([c.has_nan for c in p.cases]), np.array([c.zero_sign_free for c in p.cases])


# -- the cases of tests/test_fixbadpix_model_host.py and tests/test_gpu_fixbadpix.py -----------------------------------
# (dtype, deltapix) -> good pixels per window.  The float32 lengths straddle each sort width of the kernel's windows and its
# middle; the float64 ones are both parities at the small, a middle and the largest count of each window.
LENGTHS = {
    ('float32', 1): (1, 2, 3, 4, 5, 7, 8),
    ('float32', 2): (9, 15, 16, 17, 23, 24),
    ('float32', 3): (25, 31, 32, 33, 47, 48),
    ('float32', 4): (49, 63, 64, 65, 80),
    ('float64', 1): (4, 5, 8),
    ('float64', 2): (23, 24),
    ('float64', 3): (47, 48),
    ('float64', 4): (79, 80),
}
# Windows cut by the border: the two largest counts a corner window holds, (d + 1)^2 - 1 and one less (all four corners
# and the edges carry lines), and the two largest an edge window holds, (d + 1)(2d + 1) - 1 and one less (edges only).
BORDER_LENGTHS = {d: (capacity(d, 'corner') - 1, capacity(d, 'corner'), capacity(d, 'edge') - 1, capacity(d, 'edge'))
                  for d in (1, 2, 3, 4)}


def params():
    """Every (dtype name, deltapix, n, border) of the table."""
    for (dt, d), ns in LENGTHS.items():
        for n in ns:
            yield dt, d, n, False
        for n in BORDER_LENGTHS[d]:
            yield dt, d, n, True
