"""The generalized ESD rejection rule on the GPU (csrc/stack_esd.hip) against its NumPy restatement (tests/stack_esd_model.py):
count, mean_f64 and std_f64 bit for bit, mean and std their float32 roundings - on every slot count's edge, ragged pixel counts,
both dtypes, the fused calibration, a pixel mask, row stripes, non-finite values, ties, the crafted lines of
tests/orderstat_cases.py and columns crafted for the test's own branches; with the per-frame parameters and the local meshes;
under the guard bands of tests/guard.py; and end to end on the ten-frame stack with a trail."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import orderstat_cases as oc
from tests import stack_esd_model as model
from tests import stack_frame_model as frame
from tests import stack_local_model as local
from tests.guard import current, guarded, intact, place, unchanged
from tests.util import assert_biteq, synth_cube, synth_masters

pytestmark = pytest.mark.gpu
F = np.float32
OUTPUTS = ('mean', 'std', 'count', 'mean_f64', 'std_f64')
FRAC, ALPHA, RELAX = 0.3, 0.05, 1.5


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _compare(got, ref, what):
    with np.errstate(over='ignore', invalid='ignore'):
        want = dict(count=ref['count'], mean_f64=ref['mean_f64'], std_f64=ref['std_f64'], mean=ref['mean_f64'].astype(F),
                    std=ref['std_f64'].astype(F))
    for k in OUTPUTS:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert_biteq(g, want[k].reshape(g.shape), '%s: %s' % (what, k))
        if k in ('mean', 'std'):                             # the NaN of a pixel without data: quiet, positive, no payload
            assert (g.view(np.uint32)[np.isnan(g)] == 0x7fc00000).all(), what


def _check(raw, what, frac=FRAC, relax=RELAX, alpha=ALPHA, table=None, values=None, calib=None, pixmask=None):
    """raw: what the library is given (host array or device tensor); values: the float32 values of its columns (default: raw)."""
    from astrophotography_amd import ops
    values = np.asarray(raw, F) if values is None else values
    N = values.shape[0]
    lam = ops.esd_lambda(N, frac, alpha) if table is None else table
    ref = model.esd(values.reshape(N, -1), lam, frac, relax, None if pixmask is None else pixmask.reshape(-1))
    t = raw if torch.is_tensor(raw) else _dev(raw)
    got = ops.stack_reject(t, 'esd', calib=calib, pixmask=None if pixmask is None else _dev(pixmask), outputs=OUTPUTS,
                           esd_outliers=frac, esd_significance=alpha, esd_low_relaxation=relax, esd_table=table)
    _compare(got, ref, what)
    return ref


def _outliers(rng, cube, high=0.05, low=0.02):
    """Bright and dark outliers on a cube of small spread: the rule has something to find at either end."""
    span = F(np.nanmax(cube) - np.nanmin(cube) + 1)
    out = cube.astype(np.float64)
    out[rng.random(cube.shape) < high] += 4 * span
    out[rng.random(cube.shape) < low] -= 6 * span
    if cube.dtype == np.uint16:
        return np.clip(out, 0, 65535).astype(np.uint16)
    return out.astype(F)


def _slot_counts():
    from astrophotography_amd import ops
    return sorted({int(ops.stack_kernel_name(n, calibrated=False, rejection='esd').split('<')[1].split(',')[0]) for n in range(1, 129)})


def _calibrated(rng, raw, still_biased=True):
    """Masters for raw[N, P] and the float32 values the fused calibration forms (the oracle's ApCalibrate arithmetic)."""
    from oracle import apref
    N, P = raw.shape
    bias, dark, flat = synth_masters(rng, (P,))
    flat[0] = 0.0                                            # a zero in the flat: no division there
    if P > 1:
        flat[1] = np.nan                                     # a NaN: the whole column is not finite
    nflat, _ = apref.flat_normalize(flat)
    e = rng.uniform(0.3, 0.5, N).astype(F)
    ped = np.where(rng.random(N) < 0.3, -50.0, 0.0).astype(F)
    cal = apref.calibrate(raw.reshape(N, 1, P), bias, dark, nflat, [float(v) for v in e], [float(v) for v in ped], still_biased)
    calib = dict(bias=_dev(bias), dark=_dev(dark), nflat=_dev(nflat), exp_ratio=e, pedestal=ped, dark_still_biased=still_biased)
    return calib, np.asarray(cal, F).reshape(N, P)


@pytest.mark.parametrize('dtype', [F, np.uint16], ids=['f32', 'u16'])
def test_every_slot_count_at_its_edges(dtype):
    slots = _slot_counts()
    assert slots == [8, 16, 32, 64, 128]
    frames = sorted({1, 2, 3, 4} | {n for s in slots for n in (s - 1, s, s + 1) if 1 <= n <= 128})
    rng = np.random.default_rng(1)
    P = 257
    removed = 0
    for n in frames:
        raw = _outliers(rng, synth_cube(rng, n, (P,), dtype=dtype))
        if dtype == F:
            raw[rng.random(raw.shape) < 0.02] = np.nan
        ref = _check(raw, '%d frames' % n)
        removed += int((ref['L'] + ref['H'] > 0).sum())
    assert removed > 1000                                    # the rule was at work


@pytest.mark.parametrize('P', [1, 63, 64, 65, 257])
def test_pixel_counts_calibration_and_mask(P):
    rng = np.random.default_rng(100 + P)
    n = 12
    for dtype in (F, np.uint16):
        raw = _outliers(rng, synth_cube(rng, n, (P,), dtype=dtype))
        _check(raw, 'plain P = %d' % P)
        if dtype == F:
            raw = (raw + 1000.0).astype(F)
            raw[n // 2, P // 3] = np.inf
        calib, cal = _calibrated(rng, raw)
        pm = (rng.random(P) < 0.1).astype(np.uint8)
        _check(raw, 'fused P = %d %s' % (P, np.dtype(dtype).name), values=cal, calib=calib)
        _check(raw, 'fused + mask P = %d %s' % (P, np.dtype(dtype).name), values=cal, calib=calib, pixmask=pm)
        _check(raw, 'mask P = %d %s' % (P, np.dtype(dtype).name), pixmask=pm)


def test_row_stripes():
    """frames[:, r0:r1] of a contiguous slab is reduced in place (frame_stride > n_pixels)."""
    rng = np.random.default_rng(5)
    n, H, W = 10, 19, 67
    for dtype in (F, np.uint16):
        cube = _outliers(rng, synth_cube(rng, n, (H, W), dtype=dtype))
        if dtype == F:
            cube[rng.random(cube.shape) < 0.01] = np.nan
        t = _dev(cube)
        for r0, r1 in ((0, 5), (5, 6), (7, 19)):
            stripe = t[:, r0:r1]
            assert stripe.stride(0) == H * W
            _check(stripe, 'rows %d:%d' % (r0, r1), values=cube[:, r0:r1].astype(F))


def test_nonfinite_values_and_ties():
    rng = np.random.default_rng(8)
    n, P = 20, 300
    cube = synth_cube(rng, n, (P,), nan_frac=0.15)
    cube[:, 0] = np.nan                                      # nothing finite
    cube[:, 1] = np.inf
    cube[:, 2] = [np.nan, np.inf, -np.inf, 1.0] * 5          # few finite values
    cube[1:, 3] = np.nan                                     # one value
    cube[2:, 4] = -np.inf                                    # two
    cube[:, 5] = 3.5                                         # constant
    cube[:, 6] = [0.0, -0.0] * 10                            # zeros of both signs
    cube[:, 7] = -0.0
    for frac in (0.0, 0.1, 0.3, 0.5):
        for relax in (1.0, 1.5, 4.0):
            _check(cube, 'non-finite frac %g relax %g' % (frac, relax), frac=frac, relax=relax)
    # low-range integer data full of ties: which of the equal values goes decides the bits of the sum
    pool = np.array([1e-7, 0.3, 1.0000001, 7e6, -7e6, 3e13, -3e13, -0.0, 0.0], F)     # few values, float64 sums that round
    for n in (9, 24, 31, 100):
        ties = rng.integers(0, 4, (n, 500)).astype(F) * F(0.1) + F(1e4)
        ties[rng.random(ties.shape) < 0.1] = -0.0
        ties[rng.random(ties.shape) < 0.1] = 0.0
        wide = rng.choice(pool, (n, 500))
        for frac, relax, alpha in ((0.3, 1.5, 0.05), (0.5, 1.0, 0.4)):
            ref = _check(wide, 'wide ties n = %d frac %g' % (n, frac), frac=frac, relax=relax, alpha=alpha)
            assert (ref['L'] + ref['H'] > 0).any()
            ref = _check(ties, 'ties n = %d frac %g' % (n, frac), frac=frac, relax=relax, alpha=alpha)
            assert (ref['L'] > 0).any()
        _check(ties.astype(np.uint16), 'uint16 ties n = %d' % n, frac=0.5, relax=1.0, alpha=0.4)


@pytest.mark.parametrize('n', [5, 8, 12, 33, 64])
def test_orderstat_lines_as_columns(n):
    """The conformance table's lines, one per pixel: repeated values, zeros of either sign, infinities, digit boundaries."""
    lines = [c.values for c in oc.cases(np.float32, n)]
    cube = np.ascontiguousarray(np.stack(lines, 1))
    with np.errstate(all='ignore'):
        for frac, relax, alpha in ((0.3, 1.5, 0.05), (0.5, 1.0, 0.5), (0.5, 4.0, 0.9)):
            _check(cube, 'lines n = %d frac %g relax %g' % (n, frac, relax), frac=frac, relax=relax, alpha=alpha)


def test_crafted_columns():
    """Columns that take the test's own branches, mixed into wavefronts with clean, short and empty ones."""
    from astrophotography_amd import ops
    rng = np.random.default_rng(11)
    n = 10
    base = np.array([-1.5, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0, 1.5, 0.125], F)
    cols, tags = [], []

    def add(tag, values, frac, relax, expect=None, lam=None):
        cols.append((tag, np.asarray(values, F), frac, relax, expect, lam))

    # removals that alternate between the two ends: outliers of growing size on alternating sides, relax 1
    alt = np.array([-40.0, 30.0, -20.0, 0.0, 0.1, -0.1, 0.2, -0.2, 0.05, -0.05], F)
    add('alternating', alt, 0.3, 1.0, (2, 1))
    # dh == dl exactly (a symmetric column, relax 1: the mean is 0): the high end goes
    sym = np.array([-8.0, 8.0, -1.0, 1.0, -0.5, 0.5, -0.25, 0.25, 0.0, 0.0], F)
    add('dh == dl', sym, 0.3, 1.0)
    # two equal outliers of ten: step 0 is not significant (they mask each other), step 1 is - both go
    two = base.copy()
    two[[2, 6]] = 400.0
    add('two equal outliers', two, 0.3, 1.5, (0, 2))
    # every one of the K steps significant
    three = base.copy()
    three[[0, 4, 8]] = [1e3, 1e5, 1e7]
    add('every step significant', three, 0.3, 1.5, (0, 3))
    # a window that turns constant mid-way: sd == 0 ends the test
    add('constant after one', np.array([7.0] * 9 + [9.0], F), 0.3, 1.5, (0, 1))
    add('constant', np.full(n, 7.0, F), 0.5, 1.0, (0, 0))
    # a dark outlier that the low relaxation saves, and one that it does not
    dark = base.copy()
    dark[3] = -9.0
    add('dark, relax 4', dark, 0.3, 4.0)
    add('dark, relax 1', dark, 0.3, 1.0)
    lam10 = ops.esd_lambda(n, 0.3, ALPHA)
    for tag, v, frac, relax, expect, _ in cols:
        c = model.column_1d(v, ops.esd_lambda(n, frac, ALPHA), frac, relax)
        if expect is not None:
            assert (c['L'], c['H']) == expect, (tag, c['L'], c['H'], c['R'])
    c = model.column_1d(two, lam10, 0.3, 1.5)
    assert not c['R'][0] > lam10[n][0] and c['R'][1] > lam10[n][1]
    c = model.column_1d(three, lam10, 0.3, 1.5)
    assert all(r > lam10[n][i] for i, r in enumerate(c['R'])) and len(c['R']) == 3
    assert model.column_1d(alt, lam10, 0.3, 1.0)['sides'] == ['l', 'h', 'l']
    c = model.column_1d(sym, lam10, 0.3, 1.0)
    assert c['sides'][:2] == ['h', 'l'] and 2.0 < c['R'][0] < lam10[n][0]
    assert model.column_1d(dark, lam10, 0.3, 1.0)['L'] == 1 and model.column_1d(dark, lam10, 0.3, 4.0)['L'] == 0
    # one slab per (frac, relax): the crafted columns between noise, with lanes of every n (NaNs from the top: K = 0 below n = 4)
    for frac, relax in sorted({(c[2], c[3]) for c in cols}):
        mine = [c[1] for c in cols if (c[2], c[3]) == (frac, relax)]
        P = 200
        cube = rng.normal(0.0, 1.0, (n, P)).astype(F)
        cube[rng.random(cube.shape) < 0.05] += F(50.0)
        for j, v in enumerate(mine):
            cube[:, 3 + 17 * j] = v
            cube[:, 64 + 3 + 17 * j] = v[::-1]               # the same values in another frame order
        for p in range(100, 164):                            # a wavefront whose lanes hold 0 .. 10 finite values
            cube[(p - 100) % (n + 1):, p] = np.nan
        ref = _check(cube, 'crafted frac %g relax %g' % (frac, relax), frac=frac, relax=relax)
        assert len(set(ref['count'][100:164].tolist())) >= 8
    # a table with fewer steps than floor(frac n) allows: the three outliers of `three` need three steps, two are there
    cube = np.repeat(three[:, None], 70, 1)
    cube[:, 1::2] = two[:, None]
    short = ops.esd_lambda(n, 0.3, ALPHA, max_outliers=2)
    ref = _check(cube, 'max_outliers 2', table=short)
    assert (ref['H'][0::2] == 2).all() and (ref['H'][1::2] == 2).all()
    ref = _check(cube, 'max_outliers 1', table=ops.esd_lambda(n, 0.3, ALPHA, max_outliers=1))
    assert (ref['H'][1::2] == 0).all()                       # the two equal outliers mask each other in one step
    # the tie dh == dl decides the result where one step is allowed and is significant: a table of one column at 2.0
    cube = rng.normal(0.0, 1.0, (n, 70)).astype(F)
    cube[:, ::3] = sym[:, None]
    cube[:, 1::3] = sym[::-1, None]
    ref = _check(cube, 'dh == dl, one step', relax=1.0, table=np.full((n + 1, 1), 2.0))
    assert (ref['H'][0::3] == 1).all() and (ref['L'][0::3] == 0).all() and (ref['H'][1::3] == 1).all() and (ref['L'][1::3] == 0).all()
    # 24 and 40 frames (32 and 64 slots): lanes that differ in n and in K
    for n2 in (24, 40):
        cube = rng.normal(100.0, 5.0, (n2, 192)).astype(F)
        cube[[1, 9, 17]] += F(40.0)
        for p in range(192):
            cube[rng.permutation(n2)[:p % (n2 + 1)], p] = np.nan
        ref = _check(cube, 'ragged %d frames' % n2, frac=0.5, relax=1.0)
        assert (ref['steps'] > 0).any() and (ref['steps'] == 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# the per-frame parameters and the local meshes
H_, W_ = 48, 64


def _weighted_check(raw, v, w, what, pixmask=None, **kw):
    from astrophotography_amd import ops
    N = raw.shape[0]
    ref = model.esd_weighted(v.reshape(N, -1), np.ones(N, F) if w is None else w, ops.esd_lambda(N, FRAC, ALPHA), FRAC, RELAX,
                             None if pixmask is None else pixmask.reshape(-1))
    got = ops.stack_reject(kw.pop('t', None) if 't' in kw else _dev(raw), 'esd', outputs=OUTPUTS, weights=w,
                           pixmask=None if pixmask is None else _dev(pixmask), **kw)
    _compare(got, ref, what)
    return ref


@pytest.mark.parametrize('dtype', [F, np.uint16], ids=['f32', 'u16'])
def test_frame_params(dtype):
    rng = np.random.default_rng(21)
    for n in (7, 10, 24, 65):
        raw = _outliers(rng, synth_cube(rng, n, (H_, W_), dtype=dtype))
        if dtype == F:
            raw[rng.random(raw.shape) < 0.01] = np.nan
        a = rng.uniform(0.5, 2.0, n).astype(F)
        b = rng.uniform(-300.0, 300.0, n).astype(F)
        w = rng.uniform(0.05, 1.0, n).astype(F)
        pm = (rng.random((H_, W_)) < 0.05).astype(np.uint8)
        ref = _weighted_check(raw, frame.frame_map(raw, a, b), w, 'frame params %d frames' % n, pixmask=pm, scale=a, offset=b)
        assert (ref['count'] < n).any()
    _weighted_check(raw, frame.frame_map(raw, np.ones(n, F), b), None, 'offset only', offset=b)


@pytest.mark.parametrize('box', [8, 16])
def test_frame_local(box):
    rng = np.random.default_rng(22 + box)
    n = 12
    ny, nx = -(-H_ // box), -(-W_ // box)
    for dtype in (F, np.uint16):
        raw = _outliers(rng, synth_cube(rng, n, (H_, W_), dtype=dtype))
        if dtype == F:
            raw[rng.random(raw.shape) < 0.01] = np.nan
        A = rng.uniform(0.5, 2.0, (n, ny, nx)).astype(F)
        B = rng.uniform(-300.0, 300.0, (n, ny, nx)).astype(F)
        w = rng.uniform(0.05, 1.0, n).astype(F)
        pm = (rng.random((H_, W_)) < 0.05).astype(np.uint8)
        t = _dev(raw)
        ref = _weighted_check(raw, local.local_values(raw, A, B, box), w, 'local box %d' % box, pixmask=pm, scale=A, offset=B, box=box, t=t)
        assert (ref['count'] < n).any()
        _weighted_check(raw, local.local_values(raw, None, B, box), None, 'local, scale None', offset=B, box=box, t=t)
        r0, r1 = 13, 40                                      # a row stripe of the slab, reduced in place
        stripe = t[:, r0:r1]
        assert stripe.stride(0) == H_ * W_
        _weighted_check(raw[:, r0:r1], local.local_values(raw[:, r0:r1], A, B, box, row0=r0), w, 'local stripe', scale=A, offset=B,
                        box=box, row0=r0, t=stripe)


# ---------------------------------------------------------------------------------------------------------------------------
# guard bands
def test_guard_bands(monkeypatch):
    """Two poisons, inputs one element off alignment, a side stream: no load outside an input reaches a result, no store leaves
    an output, no input is written, and the call runs on the current stream; then the C ABI itself with the frames, the meshes,
    the weights, the table of critical values and the outputs inside poisoned surrounds."""
    from astrophotography_amd import _lib, ops
    from oracle import apref
    rng = np.random.default_rng(77)
    n, P = 13, 1031
    raw = _outliers(rng, synth_cube(rng, n, (P,), dtype=np.uint16))
    bias, dark, flat = synth_masters(rng, (P,))
    nflat, _ = apref.flat_normalize(flat)
    e = rng.uniform(0.3, 0.5, n).astype(F)
    cal = np.asarray(apref.calibrate(raw.reshape(n, 1, P), bias, dark, nflat, [float(v) for v in e], None, True), F).reshape(n, P)
    pm = (rng.random(P) < 0.05).astype(np.uint8)
    f32 = _outliers(rng, synth_cube(rng, n, (P,)))
    f32[rng.random(f32.shape) < 0.02] = np.nan
    lam = ops.esd_lambda(n, FRAC, ALPHA)
    refs = [model.esd(cal, lam, FRAC, RELAX, pm), model.esd(f32, lam, FRAC, RELAX)]
    G = 64 * 1024

    def run(poison, shift):
        with guarded(monkeypatch, G) as g:
            toks = []

            def dev(a):
                t, tok = place(a, poison, shift * a.dtype.itemsize, G)
                toks.append(tok)
                return t
            calib = dict(bias=dev(bias), dark=dev(dark), nflat=dev(nflat), exp_ratio=e, dark_still_biased=True)
            r1 = ops.stack_reject(dev(raw), 'esd', calib=calib, pixmask=dev(pm), outputs=OUTPUTS)
            r2 = ops.stack_reject(dev(f32), 'esd', outputs=OUTPUTS)
            torch.cuda.current_stream().synchronize()
            for tok in toks:
                unchanged(tok)
            out = [{k: v.cpu().numpy() for k, v in r.items()} for r in (r1, r2)]
        return out, g.lib.streams()

    default = torch.cuda.default_stream().cuda_stream
    Ar, sa = run(0xFF, 0)
    assert sa and all(s == default for _, s in sa)
    Br, _ = run(0x00, 1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Cr, sc = run(0xFF, 1)
    assert sc and all(s == side.cuda_stream for _, s in sc)
    for i in range(2):
        _compare(Ar[i], refs[i], 'run A %d' % i)
        for other, tag in ((Br, 'poison 0x00, shifted'), (Cr, 'side stream')):
            for k in OUTPUTS:
                assert_biteq(other[i][k], Ar[i][k], '%s: %s' % (tag, k))

    # the C ABI: local meshes, weights and the table in poisoned slabs
    lib = _lib.load()
    Hh, Ww, box = 37, 83, (16, 24)
    ny, nx = 3, 4
    Pp = Hh * Ww
    img = _outliers(rng, synth_cube(rng, n, (Hh, Ww)))
    A = rng.uniform(0.5, 2.0, (n, ny, nx)).astype(F)
    B = rng.uniform(-300.0, 300.0, (n, ny, nx)).astype(F)
    w = rng.uniform(0.05, 1.0, n).astype(F)
    ref = model.esd_weighted(local.local_values(img, A, B, box).reshape(n, -1), w, lam, FRAC, RELAX)
    for poison in (0xFF, 0x00):
        frames, ftok = place(img, poison, 4, G)
        sc_, stok = place(A, poison, 4, G)
        of_, otok = place(B, poison, 4, G)
        wt_, wtok = place(w, poison, 4, G)
        lm_, ltok = place(lam, poison, 8, G)
        mean, mtok = place(np.zeros(Pp, F), poison, 4, G, what='mean')
        m64, dtok = place(np.zeros(Pp, np.float64), poison, 0, G, what='mean_f64')
        s64, qtok = place(np.zeros(Pp, np.float64), poison, 8, G, what='std_f64')
        cnt, ctok = place(np.zeros(Pp, np.int32), poison, 4, G, what='count')
        d = _lib.StackLocal()
        d.width, d.row0, d.box_height, d.box_width, d.ny, d.nx = Ww, 0, box[0], box[1], ny, nx
        d.scale, d.offset, d.weight = sc_.data_ptr(), of_.data_ptr(), wt_.data_ptr()
        es = _lib.StackEsd()
        es.lambda_, es.max_outliers, es.reserved, es.local = lm_.data_ptr(), lam.shape[1], 0, C.addressof(d)
        a = _lib.StackArgs()
        a.frames, a.dtype, a.n_frames, a.n_pixels, a.frame_stride = frames.data_ptr(), 0, n, Pp, Pp
        a.center, a.dev, a.maxiters = 0, 0, -1
        a.sigma_lower, a.sigma_upper = FRAC, RELAX
        a.flags = _lib.STACK_REJECT_ESD | _lib.STACK_FRAME_LOCAL
        a.workspace, a.workspace_bytes = C.addressof(es), C.sizeof(es)
        a.mean, a.mean_f64, a.std_f64, a.count = mean.data_ptr(), m64.data_ptr(), s64.data_ptr(), cnt.data_ptr()
        _lib.check(lib.apgpu_stack_sigclip(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        for tok in (ftok, stok, otok, wtok, ltok):
            unchanged(tok)
        for tok in (mtok, dtok, qtok, ctok):
            intact(tok)
        assert_biteq(current(dtok).view(np.float64), ref['mean_f64'].reshape(-1), 'ABI mean_f64')
        assert_biteq(current(qtok).view(np.float64), ref['std_f64'].reshape(-1), 'ABI std_f64')
        assert_biteq(current(ctok).view(np.int32), ref['count'].reshape(-1), 'ABI count')
        assert_biteq(current(mtok).view(F), ref['mean_f64'].astype(F).reshape(-1), 'ABI mean')


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: ten frames, a trail on two of them (the fixture of tests/test_gpu_stack_reject.py)
SKY, NOISE, TRAIL = 100.0, 5.0, 400.0


@pytest.fixture(scope='module')
def trail_stack():
    from astrophotography_amd import ops
    rng = np.random.default_rng(2026)
    n, shape = 10, (48, 80)
    cube = rng.normal(SKY, NOISE, (n,) + shape).astype(F)
    on = np.zeros(shape, bool)
    for x in range(8, 72):
        y = 6 + x // 2
        on[y, x] = on[y + 1, x] = True
    for f in (2, 6):
        cube[f][on] += TRAIL
    ref = model.esd(cube.reshape(n, -1), ops.esd_lambda(n, FRAC, ALPHA), FRAC, RELAX)
    return cube, on, ref


def _trail_checks(image, count, on, interior=None):
    """No trace of the trail: a trail pixel's result is the mean of m of its 8 clean values, each N(SKY, NOISE); its deviation
    from SKY has a standard deviation of at most NOISE / sqrt(m), m >= 4; 6 standard deviations over the ~130 trail pixels are
    exceeded with probability 130 * 2e-9."""
    sel = on if interior is None else (on & interior)
    assert sel.sum() > 60
    img, cnt = image[sel].astype(np.float64), count[sel]
    assert (cnt <= 8).all() and (cnt >= 4).all(), (cnt.min(), cnt.max())
    assert (np.abs(img - SKY) <= 6 * NOISE / np.sqrt(cnt)).all(), float(np.abs(img - SKY).max())


def test_trail_ops_and_apstack(trail_stack, tmp_path):
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio, ops
    cube, on, ref = trail_stack
    t = _dev(cube)
    r = ops.stack_reject(t, 'esd', outputs=('mean', 'count'))
    _trail_checks(r['mean'].cpu().numpy(), r['count'].cpu().numpy(), on)
    assert_biteq(r['mean'].cpu().numpy().reshape(-1), ref['mean_f64'].astype(F))
    assert_biteq(r['count'].cpu().numpy().reshape(-1), ref['count'])
    st = ap.ApStack('CRITICAL')
    s = st.stack(t, method='esd', outputs=('mean', 'count', 'std'))
    assert_biteq(s['mean'].cpu().numpy(), r['mean'].cpu().numpy())
    assert_biteq(s['std'].cpu().numpy().reshape(-1), ref['std_f64'].astype(F))
    # a stricter level keeps more: the constructor's keywords reach the kernel
    strict = ap.ApStack('CRITICAL', esd_outliers=0.2, esd_significance=0.001, esd_low_relaxation=2.0)
    s2 = strict.stack(t, method='esd', outputs=('mean', 'count'))
    ref2 = model.esd(cube.reshape(10, -1), ops.esd_lambda(10, 0.2, 0.001), 0.2, 2.0)
    assert_biteq(s2['count'].cpu().numpy().reshape(-1), ref2['count'])
    assert_biteq(s2['mean'].cpu().numpy().reshape(-1), ref2['mean_f64'].astype(F))
    # files
    names = []
    for i in range(cube.shape[0]):
        names.append(str(tmp_path / ('f%d.fits' % i)))
        fitsio.write(names[-1], cube[i], fitsio.Header())
    st.stack_files(names, str(tmp_path / 'e.fits'), method='esd')
    img, h = fitsio.read(str(tmp_path / 'e.fits'))
    assert_biteq(img.reshape(-1), ref['mean_f64'].astype(F))
    assert h['STACKMET'] == 'esd' and h['STACKESO'] == 0.3 and h['STACKESS'] == 0.05 and h['STACKESR'] == 1.5
    assert any('ESD' in str(v) for v in h.history())


def test_trail_coadd_and_script(trail_stack, tmp_path):
    import yaml
    from astrophotography_amd import fitsio, ops
    from astrophotography_amd.scripts import ap_coadd
    cube, on, _ = trail_stack
    n = cube.shape[0]
    ident = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * n
    t = _dev(cube)
    res, _ = ops.resample_affine(t, ident, weight=False)
    res_h = res.cpu().numpy()
    interior = np.isfinite(res_h).all(0)
    assert interior[8:-8, 8:-8].all()
    r = ops.coadd(t, ident, combine='ESD')
    _trail_checks(r['image'].cpu().numpy(), r['count'].cpu().numpy(), on, interior)
    want = model.esd(res_h.reshape(n, -1), ops.esd_lambda(n, FRAC, ALPHA), FRAC, RELAX)
    assert_biteq(r['image'].cpu().numpy().reshape(-1), want['mean_f64'].astype(F))
    # normalize and weighting go with it as with WINSORIZED
    rn = ops.coadd(t, ident, combine='esd', normalize='additive', weighting='noise')
    _trail_checks(rn['image'].cpu().numpy(), rn['count'].cpu().numpy(), on, interior)
    assert rn['scale'].shape == (n,)
    rb = ops.coadd(t, ident, combine='ESD', normalize='additive', norm_box=16)
    _trail_checks(rb['image'].cpu().numpy(), rb['count'].cpu().numpy(), on, interior)
    assert rb['norm_box'] == (16, 16)
    # the script: frames of one exposure, identity transforms
    names = []
    for i in range(n):
        names.append(str(tmp_path / ('c%d.fits' % i)))
        h = fitsio.Header()
        h['EXPOSURE'] = 1.0
        fitsio.write(names[-1], cube[i], h)
    with open(tmp_path / 't.yml', 'w') as fh:
        yaml.safe_dump({'transforms': {'c%d.fits' % i: ident[i] for i in range(n)}}, fh)
    out, wout = str(tmp_path / 'esd.fits'), str(tmp_path / 'esd_w.fits')
    assert ap_coadd.main([out, *names, '--transforms', str(tmp_path / 't.yml'), '--combine', 'ESD', '--weight_image', wout, '-l', 'CRITICAL',
                          '--esd_outliers', '0.25', '--esd_significance', '0.01', '--esd_low_relaxation', '2']) == 0
    img, h = fitsio.read(out)
    cnt, _ = fitsio.read(wout)
    assert h['COMBINET'] == 'ESD' and h['COMBESO'] == 0.25 and h['COMBESS'] == 0.01 and h['COMBESR'] == 2.0
    _trail_checks(img, cnt.astype(np.int32), on, interior)
