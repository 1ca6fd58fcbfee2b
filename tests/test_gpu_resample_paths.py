"""F3 (GPU): the resample kernels on the limits between their tile paths, held to three things at once - the oracle bit for bit,
the exact defined plane of the independent model (tests/resample_model.py), and the model's float64 value within the derived
bound c * 2^-24 * S (c = 11, 12 under conserve_flux: resample_model.rounding_count).  Every case asserts with classify_tiles -
a restatement of the tile rule, used for coverage only - that it reaches the tile classes it was built for, at least 8 tiles
each.  The oversampled and the fused resample + clip kernels run on the footprint-limit, border and orientation sets."""
import numpy as np
import pytest

from tests import resample_model as rm
from tests.util import assert_biteq, assert_ulp

pytestmark = pytest.mark.gpu

IN, OUT = (150, 280), (96, 192)
MIN_TILES = 8


@pytest.fixture(scope='module')
def ops():
    import torch  # noqa: F401
    from astrophotography_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def apref():
    from oracle import apref as _a
    return _a


def _frames(n, shape, seed=1):
    return np.random.default_rng(seed).normal(300, 30, (n,) + tuple(shape)).astype(np.float32)


def _need(tiles, what, **want):
    n = rm.count_tiles(tiles, **want)
    assert n >= MIN_TILES, '%s: %d tiles of %r, at least %d wanted' % (what, n, want, MIN_TILES)
    return n


def _check(ops, apref, frames, A, what, mask=None, out_shape=OUT, n_phases=1024, fscale=None, conserve_flux=False, want_model=False):
    """resample_affine against oracle (bits), model (defined plane, bound) -> largest ratio to 2^-24 S"""
    import torch
    kw = dict(out_shape=out_shape, n_phases=n_phases, fscale=fscale, conserve_flux=conserve_flux)
    ref, wref = apref.resample_affine(frames, A, mask=mask, **kw)
    got, wgot = ops.resample_affine(torch.from_numpy(frames).cuda(), A, mask=None if mask is None else torch.from_numpy(mask).cuda(), **kw)
    torch.cuda.synchronize()
    got, wgot = got.cpu().numpy(), wgot.cpu().numpy()
    assert_biteq(got, ref, what)
    assert np.array_equal(wgot, wref), what
    model = rm.resample_model(frames, A, mask=mask, lut=ops.lanczos3_table(n_phases).cpu().numpy(), **kw)
    assert np.array_equal(wgot == 1, model[0]), what
    ratio = rm.compare(got, model, conserve_flux=conserve_flux, what=what)
    print('%s: largest |kernel - model| = %.2f x 2^-24 S over %d defined pixels' % (what, ratio, int(model[0].sum())))
    return (ratio, model) if want_model else ratio


def _check_oversampled(ops, apref, frames, A, what, mask=None, out_shape=OUT, ns=(2, 3, 4), per_tile=False):
    """resample_oversampled against its oracle (bits) and the model (the bound + one rounding of the mean); per_tile: the fine
    transforms handed over one per output tile (16-row workgroups)"""
    import torch
    t = torch.from_numpy(frames).cuda()
    mk = None if mask is None else torch.from_numpy(mask).cuda()
    for n in ns:
        fine = rm.fine_affines(A, n)
        assert np.array_equal(fine, ops.oversampled_affines(A, n, out_shape)[0].numpy())
        if per_tile:
            fine = rm.per_tile_copies(fine, out_shape)
            got = ops.resample_oversampled(t, None, n, mask=mk, out_shape=out_shape, fine_affines=fine).cpu().numpy()
        else:
            got = ops.resample_oversampled(t, A, n, mask=mk, out_shape=out_shape).cpu().numpy()
        ref, _ = apref.resample_oversampled(frames, fine, n, mask=mask, out_shape=out_shape)
        assert_biteq(got, ref, '%s, oversampling %d' % (what, n))
        model = rm.resample_model(frames, fine, mask=mask, out_shape=out_shape, lut=ops.lanczos3_table(1024).cpu().numpy(), oversampling=n)
        ratio = rm.compare(got, model, what='%s, oversampling %d' % (what, n), mean_rounding=True)
        print('%s, oversampling %d: %.2f x 2^-24 S over %d defined pixels' % (what, n, ratio, int(model[0].sum())))


def _check_fused(ops, apref, frames, A, what, mask=None, out_shape=OUT):
    """both fused kernels (<= 1024 phases and above) against 'oracle resample, then oracle stack', as tests/test_gpu_resample_stack.py"""
    import torch
    from tests.test_gpu_resample_stack import _check as stack_check
    for k in range(0, frames.shape[0], 16):
        fr, a = np.ascontiguousarray(frames[k:k + 16]), A[k:k + 16]
        stack_check(ops, apref, fr, a, mask=mask, out_shape=out_shape)
        t = torch.from_numpy(fr).cuda()
        mk = None if mask is None else torch.from_numpy(mask).cuda()
        r = ops.resample_stack_sigclip(t, a, mask=mk, out_shape=out_shape, n_phases=2048, outputs=('mean', 'count'))
        res_ref, _ = apref.resample_affine(fr, a, mask=mask, out_shape=out_shape, n_phases=2048)
        st = apref.stack_sigclip(res_ref, sigma=3.0, maxiters=5)
        assert np.array_equal(r['count'].cpu().numpy(), st['count']), what + ' (2048 phases): count planes differ'
        assert_ulp(r['mean'].cpu().numpy(), st['mean'].astype(np.float32), 1, what + ' (2048 phases)')


def _sparse_mask(shape, seed=2):
    m = (np.random.default_rng(seed).random(shape) < 0.002).astype(np.uint8)
    m[0, 0] = m[-1, -1] = 1
    return m


def _dense_mask(shape, seed=3):
    """more than 1 / 64 of the pixels: the bad-pixel list overflows and every tile applies the mask itself"""
    m = (np.random.default_rng(seed).random(shape) < 0.03).astype(np.uint8)
    assert np.count_nonzero(m) > max(256, shape[0] * shape[1] // 64)
    return m


def _limits_present(tiles, th):
    """the footprint limits of the fast path are in the set: 79 / 80 / 81 columns, th + 9 / th + 10 / th + 11 rows, fast up to 80 and th + 10"""
    inner = [t for t in tiles if t['cls'] in (rm.FAST, rm.STAGED_INTERIOR)]
    assert {79, 80, 81} <= {t['w'] for t in inner}, sorted({t['w'] for t in inner})
    assert {th + 9, th + 10, th + 11} <= {t['h'] for t in inner}, sorted({t['h'] for t in inner})
    for wv in (79, 80):
        assert any(t['cls'] == rm.FAST and t['w'] == wv for t in tiles), wv
    assert any(t['cls'] == rm.FAST and t['h'] == th + 10 for t in tiles)
    assert all(t['cls'] != rm.FAST for t in tiles if t['w'] > 80 or t['h'] > th + 10)
    _need(tiles, 'footprint limits', cls=rm.FAST, th=th)
    _need(tiles, 'footprint limits', cls=rm.STAGED_INTERIOR, th=th)


# ---- footprint limits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('per_tile', [False, True], ids=['th32', 'th16'])
def test_fast_staged_switch(ops, apref, per_tile):
    """Footprints 79 / 80 / 81 columns wide and th + 9 / th + 10 / th + 11 rows tall: rotations of both signs, shears and pure x scales
    picked by classify_tiles from fine sweeps; 32-row workgroups (one transform per frame) and 16-row (per tile).  Without a mask,
    with a mask by scatter (th32 only: per-tile transforms apply it inline) and with an overflowing list (inline)."""
    th = 16 if per_tile else 32
    A = rm.footprint_limit_set(IN, OUT, per_tile, limit=5)
    At = rm.per_tile_copies(A, OUT) if per_tile else A
    frames = _frames(len(A), IN)
    frames[:, 70, 140] = np.nan
    tiles = rm.classify_tiles(At, IN, OUT)
    _limits_present(tiles, th)
    _need(tiles, 'switch', cls=rm.FAST, steady=False)
    _check(ops, apref, frames, At, 'fast/staged switch th%d' % th)
    sparse, dense = _sparse_mask(IN), _dense_mask(IN)
    ts = rm.classify_tiles(At, IN, OUT, mask=sparse)
    _need(ts, 'switch, sparse mask', inline_mask=per_tile, cls=rm.FAST)
    _check(ops, apref, frames, At, 'fast/staged switch th%d, sparse mask' % th, mask=sparse)
    td = rm.classify_tiles(At, IN, OUT, mask=dense)
    _need(td, 'switch, dense mask', inline_mask=True, cls=rm.FAST)
    _need(td, 'switch, dense mask', inline_mask=True, cls=rm.STAGED_INTERIOR)
    _check(ops, apref, frames, At, 'fast/staged switch th%d, dense mask' % th, mask=dense)
    if per_tile:
        # the fused resample + clip kernels work on 16-row tiles whatever the form of the transforms: this set, whose limits are
        # those of 16-row tiles, one transform per frame and one per tile, every frame of it (16 at a time)
        _limits_present(rm.classify_tiles(A, IN, OUT, th=16), 16)
        _check_fused(ops, apref, frames, A, 'fast/staged switch', mask=sparse)
        _check_fused(ops, apref, frames, At, 'fast/staged switch, per tile')


SMALL_IN, SMALL_OUT = (110, 200), (64, 128)


@pytest.mark.parametrize('per_tile', [False, True], ids=['th32', 'th16'])
@pytest.mark.parametrize('n', [2, 3, 4])
def test_fast_staged_switch_oversampled(ops, apref, n, per_tile):
    """The oversampled kernel on the same limits: the sets are picked anew from the FINE grid's footprints (the sub-pixel centres
    reach further than the pixel centres), for 32-row workgroups and - fine transforms per output tile - 16-row ones."""
    th = 16 if per_tile else 32
    A = rm.footprint_limit_set(SMALL_IN, SMALL_OUT, per_tile, oversampling=n, limit=3)
    fine = rm.fine_affines(A, n)
    tiles = rm.classify_tiles(rm.per_tile_copies(fine, SMALL_OUT) if per_tile else fine, SMALL_IN, SMALL_OUT, oversampling=n)
    _limits_present(tiles, th)
    frames = _frames(len(A), SMALL_IN, seed=20 + n)
    frames[:, 50, 90] = np.nan
    _check_oversampled(ops, apref, frames, A, 'fast/staged switch th%d' % th, out_shape=SMALL_OUT, ns=(n,), per_tile=per_tile)
    _check_oversampled(ops, apref, frames, A, 'fast/staged switch th%d, mask' % th, mask=_sparse_mask(SMALL_IN), out_shape=SMALL_OUT, ns=(n,),
                       per_tile=per_tile)


def test_bad_pixels_on_the_rim_of_a_fast_footprint(ops, apref):
    """Non-finite and masked pixels on the first and last row and column of fast footprints - column 79 of an 80-wide one and row
    th + 9 included: every frame gets its own bad pixels at the corners of one of its fast tiles' footprints."""
    A = rm.footprint_limit_set(IN, OUT, False, limit=5)
    tiles = rm.classify_tiles(A, IN, OUT)
    frames = _frames(len(A), IN, seed=9)
    mask = np.zeros(IN, np.uint8)
    n80 = n42 = 0
    for t in tiles:
        if t['cls'] != rm.FAST or not (t['w'] == 80 or t['h'] == t['th'] + 10 or t['ty'] == 1):
            continue
        x0, y0, x1, y1 = t['bx0'], t['by0'], t['bx0'] + t['w'] - 1, t['by0'] + t['h'] - 1
        frames[t['frame'], y0, x0] = np.nan
        frames[t['frame'], y1, x1] = np.inf
        frames[t['frame'], y0, x1] = -np.inf
        if n80 + n42 < 6:
            mask[y1, x0] = 1
        n80 += t['w'] == 80
        n42 += t['h'] == t['th'] + 10
    assert n80 >= 1 and n42 >= 1
    _need(tiles, 'rim', cls=rm.FAST)
    _check(ops, apref, frames, A, 'bad pixels on footprint rims')
    _check(ops, apref, frames, A, 'bad pixels on footprint rims, mask', mask=mask)
    _check(ops, apref, frames, rm.per_tile_copies(A, OUT), 'bad pixels on footprint rims, per tile, mask', mask=mask)


def _area_limits_present(tiles, what):
    areas = {t['w'] * t['h'] for t in tiles}
    assert areas & {4095, 4096} and any(a >= 4097 for a in areas), sorted(areas)
    assert any(t['cls'] != rm.GATHER and t['w'] * t['h'] in (4095, 4096) for t in tiles)
    assert all((t['cls'] == rm.GATHER) == (t['w'] * t['h'] > 4096) for t in tiles)
    _need(tiles, what, cls=(rm.STAGED_INTERIOR, rm.STAGED_BORDER))
    _need(tiles, what, cls=rm.GATHER)


def test_staged_gather_switch(ops, apref):
    """Minification across wl * hl = 4096 floats: footprints about 32 rows tall, x scales swept across 128 columns (4096 staged,
    4128 gather), picked by classify_tiles for 32-row workgroups, for the fused kernels' 16-row tiles and for the fine grids of
    oversampling 2, 3, 4."""
    in_shape = (160, 420)
    A = rm.area_limit_set(in_shape, OUT, 32)
    _area_limits_present(rm.classify_tiles(A, in_shape, OUT), 'staged/gather')
    frames = _frames(len(A), in_shape, seed=4)
    _check(ops, apref, frames, A, 'staged/gather switch')
    _check(ops, apref, frames, A, 'staged/gather switch, mask', mask=_sparse_mask(in_shape))
    _check(ops, apref, frames, A, 'staged/gather switch, dense mask', mask=_dense_mask(in_shape))
    _check(ops, apref, frames, A, 'staged/gather switch, conserve_flux', fscale=np.linspace(0.5, 2.0, len(A)).astype(np.float32), conserve_flux=True)
    in16 = (190, 420)
    A16 = rm.area_limit_set(in16, OUT, 16)
    _area_limits_present(rm.classify_tiles(A16, in16, OUT, th=16), 'staged/gather, 16-row tiles')
    f16 = _frames(len(A16), in16, seed=17)
    _check(ops, apref, f16, rm.per_tile_copies(A16, OUT), 'staged/gather switch, per tile')
    _check_fused(ops, apref, f16, A16, 'staged/gather switch', mask=_sparse_mask(in16))
    small_in = (160, 300)
    for n in (2, 3, 4):
        An = rm.area_limit_set(small_in, SMALL_OUT, 32, oversampling=n)
        _area_limits_present(rm.classify_tiles(rm.fine_affines(An, n), small_in, SMALL_OUT, oversampling=n), 'staged/gather, oversampling %d' % n)
        _check_oversampled(ops, apref, _frames(len(An), small_in, seed=30 + n), An, 'staged/gather switch', mask=_sparse_mask(small_in),
                           out_shape=SMALL_OUT, ns=(n,))


def test_one_side_alone_beyond_the_staged_limit(ops, apref):
    """Footprints where ONE side alone exceeds 4096: 66x in x (wide and flat), 280x in y (tall and thin: beyond 4096 rows for 16-row tiles too) - the plain, the
    oversampled (2, 3, 4) and both fused kernels."""
    for what, in_shape, out_shape, A, seed in (
            ('wide and flat', (40, 34000), (16, 512), [[66.0, 0, 3.3, 0, 1.0, 4.6], [65.9, 0.01, 2.2, 0.0001, 1.0, 5.5]], 5),
            ('tall and thin', (72000, 40), (256, 24), [[1.0, 0, 4.4, 0, 280.0, 3.1], [1.0, 0.001, 3.3, 0.01, 279.5, 2.7]], 6)):
        A = np.array(A)
        side = 'w' if what.startswith('wide') else 'h'
        other = 'h' if side == 'w' else 'w'
        sets = [rm.classify_tiles(A, in_shape, out_shape), rm.classify_tiles(A, in_shape, out_shape, th=16)]
        sets += [rm.classify_tiles(rm.fine_affines(A, n), in_shape, out_shape, oversampling=n) for n in (2, 3, 4)]
        for tiles in sets:
            _need(tiles, what, cls=rm.GATHER)
            assert all(t[side] > 4096 and t[other] <= 50 for t in tiles)
        frames = _frames(2, in_shape, seed=seed)
        _check(ops, apref, frames, A, what + ' footprints', out_shape=out_shape)
        _check_oversampled(ops, apref, frames, A, what + ' footprints', out_shape=out_shape)
        _check_fused(ops, apref, frames, A, what + ' footprints', out_shape=out_shape)


# ---- frame borders -------------------------------------------------------------------------------------------------------
def test_footprints_against_the_frame_border(ops, apref):
    """bx0 and by0 at -1, 0, +1 and bx0 + w, by0 + h at the frame's size - 1, + 0, + 1 for tiles that are fast when they fit.  The
    fractions (0.45, 0.6) keep those positions on the fine grids of oversampling 2, 3, 4 as well (their first sub-pixel centre lies
    up to 0.375 below, their last up to 0.375 above the pixel centres)."""
    def transforms(in_shape, out_shape):
        (H, W), (h, w) = in_shape, out_shape
        A = []
        for e in (-1, 0, 1):
            A.append([1, 0, 2 + e + 0.45, 0, 1, 2 + e + 0.6])                              # low edges: bx0 = by0 = e
            A.append([1, 0, W + e - 4 - (w - 1) + 0.45, 0, 1, 10.6])                        # bx0 + w = W + e
            A.append([1, 0, 20.45, 0, 1, H + e - 4 - (h - 1) + 0.6])                        # by0 + h = H + e
        return np.array(A, np.float64)

    def positions(tiles, th, in_shape=IN):
        H, W = in_shape
        txm, tym = max(t['tx'] for t in tiles), max(t['ty'] for t in tiles)
        first = {t['frame']: t for t in tiles if t['tx'] == 0 and t['ty'] == 0}
        last = {t['frame']: t for t in tiles if t['tx'] == txm and t['ty'] == tym}
        assert [(first[f]['bx0'], first[f]['by0']) for f in (0, 3, 6)] == [(-1, -1), (0, 0), (1, 1)]
        assert [last[f]['bx0'] + last[f]['w'] - W for f in (1, 4, 7)] == [-1, 0, 1]
        assert [last[f]['by0'] + last[f]['h'] - H for f in (2, 5, 8)] == [-1, 0, 1]
        assert [first[f]['cls'] for f in (0, 3, 6)] == [rm.STAGED_BORDER, rm.FAST, rm.FAST]
        assert [last[f]['cls'] for f in (1, 4, 7)] == [rm.FAST, rm.FAST, rm.STAGED_BORDER]
        assert [last[f]['cls'] for f in (2, 5, 8)] == [rm.FAST, rm.FAST, rm.STAGED_BORDER]
        _need(tiles, 'borders', cls=rm.FAST, th=th)
        _need(tiles, 'borders', cls=rm.STAGED_BORDER, th=th)

    A = transforms(IN, OUT)
    positions(rm.classify_tiles(A, IN, OUT), 32)
    positions(rm.classify_tiles(A, IN, OUT, th=16), 16)
    frames = _frames(len(A), IN, seed=7)
    _check(ops, apref, frames, A, 'frame borders')
    _check(ops, apref, frames, A, 'frame borders, mask', mask=_sparse_mask(IN))
    _check(ops, apref, frames, A, 'frame borders, dense mask', mask=_dense_mask(IN))
    _check(ops, apref, frames, rm.per_tile_copies(A, OUT), 'frame borders, per tile')
    sin, sout = (110, 264), (64, 192)                           # the oversampled kernel: the same positions on a smaller frame
    As = transforms(sin, sout)
    for n in (2, 3, 4):
        positions(rm.classify_tiles(rm.fine_affines(As, n), sin, sout, oversampling=n), 32, sin)
    fs = _frames(len(As), sin, seed=19)
    _check_oversampled(ops, apref, fs, As, 'frame borders', out_shape=sout)
    _check_oversampled(ops, apref, fs, As, 'frame borders, mask', mask=_sparse_mask(sin), out_shape=sout, ns=(3,))
    _check_fused(ops, apref, frames, A, 'frame borders', mask=_sparse_mask(IN))


def test_ragged_output_sizes(ops, apref):
    """Output heights 1 .. 47 (y0 + th beyond the output, the lower half of a 32-row workgroup present or not) and widths 1 .. 129."""
    shapes = [(hh, 129) for hh in (1, 15, 16, 17, 31, 32, 33, 47)] + [(47, ww) for ww in (1, 63, 64, 65)]
    frames = _frames(3, (70, 150), seed=8)
    th = np.deg2rad(0.4)
    A = np.array([[1, 0, 3.3, 0, 1, 2.6], [np.cos(th), -np.sin(th), 4.1, np.sin(th), np.cos(th), 3.2], [1.2, 0, 2.5, 0, 1.3, 2.5]])
    n_fast = n_border = 0
    for shp in shapes:
        tiles = rm.classify_tiles(A, (70, 150), shp)
        n_fast += rm.count_tiles(tiles, cls=rm.FAST)
        n_border += rm.count_tiles(tiles, cls=rm.STAGED_BORDER)
        _check(ops, apref, frames, A, 'output %d x %d' % shp, out_shape=shp, mask=_sparse_mask((70, 150)))
        _check(ops, apref, frames, A, 'output %d x %d, dense mask' % shp, out_shape=shp, mask=_dense_mask((70, 150)))
        if shp in ((17, 129), (33, 129), (47, 65)):
            _check_oversampled(ops, apref, frames, A, 'output %d x %d' % shp, out_shape=shp)
            _check_fused(ops, apref, frames, A, 'output %d x %d' % shp, out_shape=shp)
    assert n_fast >= MIN_TILES and n_border >= MIN_TILES, (n_fast, n_border)


def test_smallest_frame(ops, apref):
    """6 x 6 is the smallest frame with a defined pixel (one 6 x 6 window); 5 x 6 and 6 x 5 are refused loudly."""
    import torch
    from astrophotography_amd._lib import ApGpuError
    frames = _frames(2, (6, 6), seed=10)
    A = np.array([[1, 0, 0, 0, 1, 0], [1, 0, 0.5, 0, 1, 0.25]], np.float64)
    assert [t['cls'] for t in rm.classify_tiles(A, (6, 6), (6, 6))] == [rm.STAGED_BORDER] * 2       # (too few tiles for a minimum of 8)
    _check(ops, apref, frames, A, 'smallest frame', out_shape=(6, 6))
    got, w = ops.resample_affine(torch.from_numpy(frames).cuda(), A)
    assert w.sum().item() == 2 and w[0, 2, 2] == 1 and got[0, 2, 2].item() == frames[0, 2, 2]
    for shp in ((5, 6), (6, 5)):
        with pytest.raises(ApGpuError):
            ops.resample_affine(torch.zeros((1,) + shp, device='cuda'), [[1, 0, 0, 0, 1, 0]])


# ---- orientation and sign --------------------------------------------------------------------------------------------------
def test_flips_turns_and_negative_coordinates(ops, apref):
    """x flip, y flip, both; 90, 180, 270, 45, 135 and -45 degrees; and transforms whose products F0 x, F1 y are far below zero before the
    offset brings the sum back, with the defined region against the frame's low edge: there 'ix - 2 >= 0' is decided by an
    arithmetic shift of a negative or barely positive sum."""
    def transforms(i, o):
        d = ((i[1] - o[1]) / 2.0 + 4.3, (i[0] - o[0]) / 2.0 + 2.6)          # a shift that puts the output's corner beyond the frame's
        A = [rm.affine(i, o, flip_x=True), rm.affine(i, o, flip_y=True), rm.affine(i, o, flip_x=True, flip_y=True),
             rm.affine(i, o, deg=90), rm.affine(i, o, deg=180), rm.affine(i, o, deg=270), rm.affine(i, o, deg=45), rm.affine(i, o, deg=135), rm.affine(i, o, deg=-45),
             rm.affine(i, o, deg=180, shift=(-d[0], -d[1])), rm.affine(i, o, flip_x=True, shift=(-d[0] - 2.4, 0.2)),
             rm.affine(i, o, flip_y=True, shift=(0.1, -d[1] - 1.8)), [1, 0, -3.5, 0, 1, -2.25], [1, 0, 0.75, 0, 1, 1.5], [-1, 0, 60.25, 0, -1, 40.5]]
        return np.array(A, np.float64)

    def reached(tiles, gather=True):
        _need(tiles, 'orientation', cls=rm.FAST)
        _need(tiles, 'orientation', cls=(rm.STAGED_INTERIOR, rm.STAGED_BORDER))
        if gather:                                              # (the 61 x 61 footprint of a 16-row tile at 45 degrees is staged)
            _need(tiles, 'orientation', cls=rm.GATHER)
        assert sum(1 for t in tiles if t['bx0'] < -2 or t['by0'] < -2) >= MIN_TILES      # footprints that start below zero

    A = transforms(IN, OUT)
    reached(rm.classify_tiles(A, IN, OUT))
    reached(rm.classify_tiles(A, IN, OUT, th=16), gather=False)
    frames = _frames(len(A), IN, seed=11)
    _check(ops, apref, frames, A, 'orientation')
    _check(ops, apref, frames, A, 'orientation, mask', mask=_sparse_mask(IN))
    _check(ops, apref, frames, rm.per_tile_copies(A, OUT), 'orientation, per tile', mask=_sparse_mask(IN))
    _check_fused(ops, apref, frames, A, 'orientation')
    As = transforms(SMALL_IN, SMALL_OUT)                        # the oversampled kernel: the same orientations on a smaller frame
    for n in (2, 3, 4):
        reached(rm.classify_tiles(rm.fine_affines(As, n), SMALL_IN, SMALL_OUT, oversampling=n))
    _check_oversampled(ops, apref, _frames(len(As), SMALL_IN, seed=21), As, 'orientation', out_shape=SMALL_OUT)


def test_tie_coefficients(ops, apref):
    """Coefficients whose product with 2^32 is an exact tie (resample_model.tie_transforms): the kernel's own conversion must round
    them to even, as the oracle's and the model's do - with the offsets on a phase boundary, one unit of 2^-32 changes the phase."""
    A = rm.tie_transforms(1024)
    _need(rm.classify_tiles(A, IN, OUT), 'ties', cls=rm.FAST, th=32)
    _need(rm.classify_tiles(rm.per_tile_copies(A, OUT), IN, OUT), 'ties', cls=rm.FAST, th=16)
    frames = _frames(2, IN, seed=18)
    _check(ops, apref, frames, A, 'tie coefficients')
    _check(ops, apref, frames, rm.per_tile_copies(A, OUT), 'tie coefficients, per tile', mask=_sparse_mask(IN))
    _check_oversampled(ops, apref, frames, A, 'tie coefficients', ns=(2,))
    _check_fused(ops, apref, frames, A, 'tie coefficients')


# ---- phase wrap ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('log2n', range(1, 21))
def test_phase_wrap_at_every_table_size(ops, apref, log2n):
    """Fractions in [1 - 1/n, 1) across whole tiles: the carry into table row n, the half-width rows 0 and n, at every accepted
    table size.  16-row workgroups (per tile): fast tiles (translation), staged tiles (2x in y), gather tiles (2x in both).  32-row
    workgroups (per frame): fast and steady tiles, staged tiles on the frame's border (the translation two columns further left),
    gather tiles (2x in both)."""
    n = 1 << log2n
    in_shape = (240, 420)
    ty, tx = OUT[0] // 16, OUT[1] // 64
    fr = [(1 - 0.4 / n, 1 - 0.9 / n), (1 - 0.5 / n, 1 - 0.5 / n), (0.5 / n, 0.49 / n), (1 - 1.0 / n, 1 - 2.0 ** -32)]
    T = np.zeros((len(fr), ty, tx, 6))
    for k, (fx, fy) in enumerate(fr):
        for j in range(ty):
            kind = (j + k) % 3
            for i in range(tx):
                if kind == 0:
                    T[k, j, i] = [1, 0, 3 + fx, 0, 1, 2 + fy]
                elif kind == 1:
                    T[k, j, i] = [1, 0, 3 + fx, 0, 2, 4 + fy]
                else:
                    T[k, j, i] = [2, 0, 5 + fx, 0, 2, 4 + fy]
    tiles = rm.classify_tiles(T, in_shape, OUT, n_phases=n)
    _need(tiles, 'phase wrap', cls=rm.FAST)
    _need(tiles, 'phase wrap', cls=rm.STAGED_INTERIOR)
    _need(tiles, 'phase wrap', cls=rm.GATHER)
    frames = _frames(3 * len(fr), in_shape, seed=12)
    _check(ops, apref, frames[:len(fr)], T, 'phase wrap, %d phases, per tile' % n, n_phases=n)
    A = np.array([a for fx, fy in fr for a in ([1, 0, 3 + fx, 0, 1, 2 + fy], [1, 0, 1 + fx, 0, 1, 2 + fy], [2, 0, 5 + fx, 0, 2, 4 + fy])])
    tiles = rm.classify_tiles(A, in_shape, OUT, n_phases=n)
    _need(tiles, 'phase wrap', cls=rm.FAST, th=32, steady=True)
    _need(tiles, 'phase wrap', cls=rm.STAGED_BORDER, th=32)
    _need(tiles, 'phase wrap', cls=rm.GATHER, th=32)
    _check(ops, apref, frames, A, 'phase wrap, %d phases, per frame' % n, n_phases=n)


# ---- sanity guards -----------------------------------------------------------------------------------------------------------
def test_sanity_guards(ops, apref):
    """Coefficients just below and just above 2^30 (one output row: y = 0 keeps the coordinates small); corners just inside and
    outside +-1e9 pixels, with the upper half only and the lower half only of a 32-row workgroup defined and holding a defined pixel; NaN and inf coefficients in
    single tiles of the per-tile form, whose neighbours must not notice."""
    big = 2.0 ** 30
    A = []
    for v in (big - 1, np.nextafter(big, 0), big, big + 1, -(big - 1), -np.nextafter(big, 0), -big, -(big + 1)):
        A.append([1, v, 3.3, 0, 1, 2.6])
        A.append([1, 0, 3.3, 0, v, 2.6])
    A = np.array(A, np.float64)
    frames = _frames(len(A), (20, 90), seed=13)
    tiles = rm.classify_tiles(A, (20, 90), (1, 64))
    _need(tiles, 'coefficients', cls=rm.NOT_SANE)
    _need(tiles, 'coefficients', cls=rm.STAGED_BORDER)            # (one output row: y0 + th lies beyond the output)
    _check(ops, apref, frames, A, 'coefficients around 2^30', out_shape=(1, 64))
    # +-1e9 along y: one half of a 32-row workgroup is a defined tile, the other is not, and the defined half holds a defined pixel
    A = []
    for a4 in (3.3e7, 4.1e7, 6.2e7):
        A.append([1, 0, 2.3, 0, a4, 2.4])                      # rows 0 .. 15 reach 15 a4 < 1e9, rows 16 .. 31 reach 31 a4 > 1e9: row 0 is in the frame
    for a4 in (3.25e7, 3.3e7, 3.4e7):
        A.append([1, 0, 2.3, 0, -a4, 31 * a4 + 2.4])           # row 0 starts at 31 a4 > 1e9, rows 16 .. 31 at 15 a4 and below: row 31 is in the frame
    A.append([1, 0, 2.3, 0, (1e9 - 2.4 - 1e-3) / 15, 2.4])     # row 15 at 1e9 - 1e-3, just inside: upper half defined, row 0 in the frame
    A.append([1, 0, 2.3, 0, (1e9 - 2.4 + 1e-3) / 15, 2.4])     # row 15 at 1e9 + 1e-3, just outside: nothing defined
    # along x a corner beside 1e9 lies far outside any frame: these two cannot show a pixel either way and only run the guard
    A.append([1, 0, 1e9 - 63 - 1e-3, 0, 1, 2.4])
    A.append([1, 0, 1e9 - 63 + 1e-3, 0, 1, 2.4])
    A = np.array(A, np.float64)
    tiles = rm.classify_tiles(A, IN, OUT)
    top_only = [t for t in tiles if t['sane_top'] and not t['sane_bot'] and t['ty'] == 0]
    bot_only = [t for t in tiles if t['sane_bot'] and not t['sane_top'] and t['ty'] == 0]
    assert len(top_only) >= MIN_TILES and len(bot_only) >= MIN_TILES, (len(top_only), len(bot_only))
    assert {t['frame'] for t in top_only} == {0, 1, 2, 6} and {t['frame'] for t in bot_only} == {3, 4, 5}
    assert all(not t['sane_top'] and not t['sane_bot'] for t in tiles if t['frame'] == 7)
    _need(tiles, 'corners', cls=rm.NOT_SANE)
    frames = _frames(len(A), IN, seed=14)
    _, model = _check(ops, apref, frames, A, 'corners around 1e9', want_model=True)
    # the defined half really holds defined pixels: honouring one flag while the other is false is what gives them
    for f in (0, 1, 2, 6):
        assert model[0][f, 0].sum() > 150 and model[0][f].sum() == model[0][f, 0].sum(), f
    for f in (3, 4, 5):
        assert model[0][f, 31].sum() > 150 and model[0][f].sum() == model[0][f, 31].sum(), f
    assert model[0][7:].sum() == 0
    _check(ops, apref, frames, A, 'corners around 1e9, mask', mask=_sparse_mask(IN))
    _check(ops, apref, frames, A, 'corners around 1e9, dense mask', mask=_dense_mask(IN))
    # per tile: bad tiles among good ones
    rng = np.random.default_rng(15)
    T = rm.per_tile_copies([rm.affine(IN, OUT, deg=0.3), rm.affine(IN, OUT, deg=-1.0, sx=1.01)], OUT)
    bad = [[np.nan, 0, 0, 0, 1, 0], [1, 0, np.inf, 0, 1, 0], [1, 0, 0, -np.inf, 1, 0], [1, 0, 0, 0, 1, np.nan], [1, big, 0, 0, 1, 0], [1, 0, 1e9, 0, 1, 0]]
    for k in range(12):
        T[k % 2, rng.integers(0, 6), rng.integers(0, 3)] = bad[k % len(bad)]
    tiles = rm.classify_tiles(T, IN, OUT)
    _need(tiles, 'bad tiles', cls=rm.NOT_SANE)
    _need(tiles, 'bad tiles', cls=rm.FAST)
    frames = _frames(2, IN, seed=16)
    _check(ops, apref, frames, T, 'NaN / inf coefficients per tile')
    _check(ops, apref, frames, T, 'NaN / inf coefficients per tile, mask', mask=_sparse_mask(IN))
    _check_fused(ops, apref, frames, T, 'NaN / inf coefficients per tile')
