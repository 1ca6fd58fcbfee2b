"""F14 on the GPU (csrc/drizzle.hip) against the NumPy model tests/drizzle_model.py: the drizzle and the rejection flags
bit for bit, NaN positions included, over the tile edges, transforms, holes and Bayer arrangements; one cube past 2^31 elements; and
ApDrizzle / ap_drizzle end to end on the star scene of tests/test_drizzle_model_host.py."""
import itertools

import numpy as np
import pytest

from tests import drizzle_model as dm

pytestmark = pytest.mark.gpu

F = np.float32
TH, TW = 4, 64                                                        # APGPU_DRIZZLE_TILE_H, APGPU_DRIZZLE_TILE_W
OUT_SHAPES = ((1, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 5))
IN_SHAPES = ((7, 9), (33, 70), (64, 130))
KINDS = ('identity', 'half', 'rot3', 'rot-3', 'rot90', 'l2', 'off', 'halfoff')


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(got, want, what=''):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, 'NaN positions differ at', np.argwhere(gn != wn)[:5].tolist())
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~wn
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


def _affines(kind, N, H, W, s):
    """Reference pixel -> input pixel, one per frame."""
    if kind == 'identity':
        return [dm.shift_affine(0, 0)] * N
    if kind == 'half':                                                # drop edges land exactly on footprint edges: the a == 0 branch
        return [dm.shift_affine(0.5 * i, -0.5 * i + 0.25) for i in range(N)]
    if kind == 'rot3':
        return [dm.shift_affine(1.3 * i, -0.7, 3.0) for i in range(N)]
    if kind == 'rot-3':
        return [dm.shift_affine(0.37 * i, 2.2, -3.0) for i in range(N)]
    if kind == 'rot90':
        return [dm.shift_affine(W - 1 + 0.25 * i, 0.3, 90.0) for i in range(N)]
    if kind == 'l2':                                                  # lx = ly = 2 exactly
        return [dm.shift_affine(0.3 * i, -0.2 * i, 0.0, 2.0 * s) for i in range(N)]
    if kind == 'off':                                                 # the last frame wholly off the grid
        return [dm.shift_affine(0.25 * i, 0) for i in range(N - 1)] + [dm.shift_affine(5 * W, -3 * H)]
    return [dm.shift_affine(W / 2 + 0.37, -H / 2 + 0.1 * i) for i in range(N)]      # half off


def _frames(rng, N, H, W, holes):
    fr = rng.normal(300.0, 40.0, (N, H, W)).astype(F)
    mask = fmask = None
    if holes == 'isolated':
        bad = rng.random(fr.shape) < 0.07
        fr[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(bad.sum()))
    elif holes == 'lines':
        fr[:, H // 2, :] = np.nan
        fr[:, :, W // 3] = np.inf
    elif holes in ('mask', 'both'):
        mask = (rng.random((H, W)) < 0.15).astype(np.uint8) * 3
    if holes in ('fmask', 'both'):
        fmask = (rng.random((N, H, W)) < 0.15).astype(np.uint8)
    if holes == 'all':
        mask = np.ones((H, W), np.uint8)
    return fr, mask, fmask


def _check(fr, aff, s, p, what, mask=None, fmask=None, out_shape=None, **kw):
    from astrophotography_amd import ops
    want = dm.drizzle(fr, aff, s, p, mask=mask, frame_masks=fmask, out_shape=out_shape, **kw)
    got = ops.drizzle(_dev(fr), aff, s, p, mask=None if mask is None else _dev(mask), frame_masks=None if fmask is None else _dev(fmask),
                      out_shape=out_shape, **kw)
    _same_bits(got['image'].cpu().numpy(), want['image'], what + ' image')
    _same_bits(got['weight'].cpu().numpy(), want['weight'], what + ' weight')
    return want


@pytest.mark.parametrize('in_shape', IN_SHAPES)
def test_drizzle_shapes_and_transforms(in_shape):
    """Every output size about the tile, every transform kind, N, scale and pixfrac, cycled against each other."""
    H, W = in_shape
    rng = np.random.default_rng(H)
    cyc = itertools.cycle(itertools.product((1, 2, 5, 17) if H < 64 else (1, 2, 5), (1, 1.5, 2, 3), (0.3, 0.5, 1)))
    seen = 0
    for out_shape in OUT_SHAPES + (None,):
        for kind in KINDS:
            N, s, p = next(cyc)
            if out_shape is None and H >= 33:
                s = min(s, 2)
            fr, _, _ = _frames(rng, N, H, W, 'isolated' if seen % 2 else 'none')
            w = rng.uniform(0.3, 3.0, N)
            fs = rng.uniform(0.01, 1.0, N)
            r = _check(fr, _affines(kind, N, H, W, s), s, p, '%s %s -> %s N %d s %g p %g' % (kind, in_shape, out_shape, N, s, p),
                       out_shape=out_shape, fscale=fs, weights=w, conserve_flux=bool(seen % 3))
            seen += int((r['weight'] > 0).any())
    assert seen > 24                                                  # most cases put something on the grid


@pytest.mark.parametrize('holes', ['none', 'isolated', 'lines', 'mask', 'fmask', 'both', 'all'])
def test_drizzle_holes(holes):
    rng = np.random.default_rng(21)
    for (H, W), N, s, p, kind in (((33, 70), 5, 2, 0.5, 'rot3'), ((7, 9), 2, 3, 0.3, 'half'), ((64, 130), 2, 1.5, 1, 'identity')):
        fr, mask, fmask = _frames(rng, N, H, W, holes)
        r = _check(fr, _affines(kind, N, H, W, s), s, p, '%s %s' % (holes, kind), mask=mask, fmask=fmask, weights=rng.uniform(0.3, 3.0, N))
        if holes == 'all':
            assert np.isnan(r['image']).all() and (r['weight'] == 0).all()


@pytest.mark.parametrize('pattern', ['RGGB', 'BGGR', 'GRBG', 'GBRG'])
def test_drizzle_cfa(pattern):
    rng = np.random.default_rng(5)
    N, H, W = 5, 33, 70
    fr, _, fmask = _frames(rng, N, H, W, 'fmask')
    aff = [dm.shift_affine(0.25 * i + (i & 1), 0.5 * i + ((i >> 1) & 1), 1.0 * i) for i in range(N)]
    for c in range(3):
        r = _check(fr, aff, 2, 0.5, '%s channel %d' % (pattern, c), fmask=fmask, cfa=(dm.COLOURS[pattern], c))
        assert (r['weight'] > 0).any() and (r['weight'] == 0).any()


def _check_reject(fr, aff, ref, rs, what, **kw):
    from astrophotography_amd import ops
    want = dm.drizzle_reject(fr, aff, ref, rs, **kw)
    got = ops.drizzle_reject(_dev(fr), aff, _dev(ref), rs, **kw).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    return want


@pytest.mark.parametrize('rs', [1.0, 2.0])
def test_reject_against_the_model(rs):
    """The drizzle tests' frame sets against a reference at ref_scale 1 and 2: pixels that map outside the reference (rotations, shifts),
    NaN / inf among the four corners and in the frames, several k and grow."""
    rng = np.random.default_rng(31)
    flagged = 0
    for (H, W), N in (((7, 9), 1), ((33, 70), 5), ((64, 130), 17)):
        for kind in ('identity', 'half', 'rot3', 'rot-3', 'rot90', 'off', 'halfoff'):
            fr, _, _ = _frames(rng, N, H, W, 'isolated')
            hr, wr = int(H * rs), int(W * rs)
            ref = rng.normal(300.0, 40.0, (hr, wr)).astype(F)
            ref[rng.random(ref.shape) < 0.03] = rng.choice(np.array([np.nan, np.inf], F))
            want = _check_reject(fr, _affines(kind, N, H, W, 1), ref, rs, '%s %s N %d' % (kind, (H, W), N), fscale=rng.uniform(0.8, 1.2, N),
                                 sigmas=rng.uniform(5.0, 20.0, N), k=float(rng.choice([3.5, 2.0, 0.0])), grow=float(rng.choice([1.2, 0.5, 0.0])))
            flagged += int(want.sum())
            if kind in ('off',):
                assert want[-1].sum() == 0                            # the frame off the grid maps outside the reference: nothing flagged
    assert flagged > 1000
    one = np.ones((1, 1), F)                                          # a reference of one pixel has no four corners
    assert _check_reject(np.full((1, 5, 5), 1e6, F), [dm.shift_affine(0, 0)], one, 1.0, 'one-pixel reference').sum() == 0


def test_reject_threshold_tie():
    """|g v - b| == k sigma + grow d exactly is not an outlier (strict >); one ulp more is."""
    ref = np.full((6, 6), 100.0, F)
    ref[:, 3:] = 104.0                                                # d = 4 across the step, 0 elsewhere
    fr = np.full((1, 6, 6), 100.0, F)
    # g = 1, sigma = 2, k = 3.5, grow = 1.5: the threshold is 7 on the flat part; at the step (column 2 -> 3, fx = 0) b = 100, d = 4: 13
    fr[0, 1, 1], fr[0, 2, 1], fr[0, 3, 1] = 107.0, np.nextafter(F(107.0), F(200.0)), 93.0
    fr[0, 1, 2], fr[0, 2, 2], fr[0, 3, 2] = 113.0, np.nextafter(F(113.0), F(200.0)), np.nextafter(F(87.0), F(0.0))
    want = _check_reject(fr, [dm.shift_affine(0, 0)], ref, 1.0, 'tie', sigmas=[2.0], k=3.5, grow=1.5)
    assert want[0, :, 1].tolist() == [0, 0, 1, 0, 0, 0] and want[0, :, 2].tolist() == [0, 0, 1, 1, 0, 0]
    assert want[0, :, 5].sum() == 0 and want[0, 5].sum() == 0       # the last column and row have no four corners


def test_argument_errors():
    import torch
    from astrophotography_amd import _lib, ops
    fr = torch.ones((2, 8, 9), device='cuda')
    ident = [dm.shift_affine(0, 0)]
    with pytest.raises(ValueError, match='footprint'):
        ops.drizzle(fr, [dm.shift_affine(0, 0, 0, 2.2)], 1, 0.5)
    ops.drizzle(fr, [dm.shift_affine(0, 0, 0, 2.0)], 1, 0.5)
    for p in (0.0, -0.5, 1.01, float('nan')):
        with pytest.raises(ValueError, match='pixfrac'):
            ops.drizzle(fr, ident, 2, p)
    for w in ([1.0, 0.0], [1.0, -2.0], [1.0, float('inf')], [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match='weights'):
            ops.drizzle(fr, ident, 2, 0.5, weights=w)
    with pytest.raises(ValueError, match='mask'):
        ops.drizzle(fr, ident, 2, 0.5, mask=torch.zeros((9, 8), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError, match='frame_masks'):
        ops.drizzle(fr, ident, 2, 0.5, frame_masks=torch.zeros((8, 9), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError, match='Bayer'):
        ops.drizzle(fr, ident, 2, 0.5, cfa=((0, 1, 2, 3), 0))
    with pytest.raises(ValueError, match='channel'):
        ops.drizzle(fr, ident, 2, 0.5, cfa=((0, 1, 3, 2), 3))
    with pytest.raises(ValueError):
        ops.drizzle(fr.cpu(), ident, 2, 0.5)
    with pytest.raises(ValueError, match='singular'):
        ops.drizzle_reject(fr, [[1, 0, 0, 2, 0, 0]], torch.ones((8, 9), device='cuda'))
    import ctypes as C
    lib = _lib.load()
    prm = torch.zeros((2, 10), dtype=torch.float64, device='cuda')
    out = torch.empty((2, 16, 18), device='cuda')
    ptr = lambda t: C.c_void_p(t.data_ptr())                          # noqa: E731
    assert lib.apgpu_drizzle_f32(ptr(fr), 2, 8, 9, None, None, ptr(prm), 1.5, None, 0, ptr(out[0]), ptr(out[1]), 16, 18, None) == _lib.E_INVAL
    assert lib.apgpu_drizzle_f32(ptr(fr), 2, 8, 9, None, None, ptr(prm), 0.5, None, 0, ptr(out[0]), ptr(out[0]), 16, 18, None) == _lib.E_INVAL
    assert lib.apgpu_drizzle_f32(ptr(fr), 2, 8, 9, None, None, None, 0.5, None, 0, ptr(out[0]), ptr(out[1]), 16, 18, None) == _lib.E_INVAL
    bad = (C.c_int32 * 4)(0, 1, 1, 2)
    assert lib.apgpu_drizzle_f32(ptr(fr), 2, 8, 9, None, None, ptr(prm), 0.5, bad, 0, ptr(out[0]), ptr(out[1]), 16, 18, None) == _lib.E_INVAL


def test_offsets_past_2_31_elements():
    """33 x 8192 x 8192: frame and frame-mask offsets pass 2^31 elements (and 2^33 bytes) inside the last frame.  Only the last
    frame counts (the others are NaN, then masked), so the result must be, bit for bit, that of the last frame drizzled alone - a
    call whose offsets stay small; an offset wrapped at 32 bits would read frame 0 or 1 instead.  The rejection flags of the last
    frame likewise."""
    import torch
    from astrophotography_amd import ops
    N, H, W = 33, 8192, 8192
    assert (N - 1) * H * W == 2 ** 31 < N * H * W                     # every element of the last frame lies at or past 2^31
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip('needs 16 GB of free device memory')
    g = torch.Generator(device='cuda').manual_seed(3)
    frames = torch.full((N, H, W), float('nan'), device='cuda')
    frames[N - 1] = torch.randn((H, W), generator=g, device='cuda') * 40.0 + 300.0
    aff = [dm.shift_affine(0.25 * (i % 4), 0.25 * (i // 4 % 4)) for i in range(N)]
    alone = ops.drizzle(frames[N - 1], aff[N - 1:], 1, 0.5)
    assert bool((alone['weight'][8:-8, 8:-8] > 0).all())
    r = ops.drizzle(frames, aff, 1, 0.5)
    assert torch.equal(r['weight'], alone['weight']) and torch.equal(r['image'].view(torch.int32), alone['image'].view(torch.int32))
    # the same through the frame masks: every frame holds data, all but the last are masked
    frames[:N - 1] = 7.0
    fmask = torch.ones((N, H, W), dtype=torch.uint8, device='cuda')
    fmask[N - 1] = 0
    r = ops.drizzle(frames, aff, 1, 0.5, frame_masks=fmask)
    assert torch.equal(r['weight'], alone['weight']) and torch.equal(r['image'].view(torch.int32), alone['image'].view(torch.int32))
    del fmask, r
    ref = alone['image'].nan_to_num(300.0) + 100.0 * (torch.rand((H, W), generator=g, device='cuda') < 0.01)
    flags = ops.drizzle_reject(frames, aff, ref, 1.0, sigmas=1.0, grow=0.0)     # (the last frame's transform is the identity: b = ref)
    last = ops.drizzle_reject(frames[N - 1], aff[N - 1:], ref, 1.0, sigmas=1.0, grow=0.0)
    assert torch.equal(flags[N - 1], last[0]) and 0.005 < float(last.float().mean()) < 0.02
    del frames, flags, last, ref, alone
    torch.cuda.empty_cache()


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def star_files(tmp_path_factory):
    """The host test's rejection scene (stars, sky 100, noise 5, 40 hits) as FITS files with EXPOSURE 2 s and a transforms YAML."""
    from astrophotography_amd import fitsio
    from tests.test_drizzle_model_host import reject_scene
    sc = reject_scene()
    d = tmp_path_factory.mktemp('drizzle')
    names = []
    for k, fr in enumerate(sc['frames']):
        hdr = fitsio.Header()
        hdr['EXPOSURE'] = 2.0
        hdr['FILTER'] = 'L'
        names.append(str(d / ('frame-%02d.fits' % k)))
        fitsio.write(names[-1], fr, header=hdr)
    yml = str(d / 'transforms.yml')
    with open(yml, 'w') as fh:
        fh.write('transforms:\n')
        for n, a in zip(names, sc['affines']):
            fh.write('  %s: [%s]\n' % (n.rsplit('/', 1)[-1], ', '.join(repr(float(v)) for v in a)))
    return dict(sc, names=names, yml=yml, dir=d)


def test_files_and_script(star_files):
    from astrophotography_amd import fitsio
    from astrophotography_amd.scripts import ap_drizzle as script
    sc = star_files
    N = len(sc['names'])
    out, wout = str(sc['dir'] / 'out.fits'), str(sc['dir'] / 'weight.fits')
    assert script.main([out] + sc['names'] + ['--transforms', sc['yml'], '--scale', '2', '--pixfrac', '0.5', '--no_weighting',
                                              '--weight_image', wout, '-l', 'ERROR']) == 0
    data, h = fitsio.read(out)
    wdata, wh = fitsio.read(wout)
    assert (h['NCOMBINE'], h['COMBINET'], h['DRIZSCAL'], h['DRIZPIXF'], h['DRIZKERN'], h['DRIZNREJ'], h['TEXPTIME'], h['BUNIT']) == \
        (N, 'DRIZZLE', 2.0, 0.5, 'TURBO', 0, 2.0 * N, 'adu/s')
    assert h['IFILE000'] == 'frame-00.fits' and h['IFILE%03d' % (N - 1)] == 'frame-%02d.fits' % (N - 1) and h['FILTER'] == 'L'
    assert any('ApDrizzle' in line for line in h.history()) and wh['NCOMBINE'] == N
    want = dm.drizzle(sc['frames'], sc['affines'], 2, 0.5, fscale=np.full(N, 0.5))
    _same_bits(np.asarray(data, F), want['image'], 'script image')
    _same_bits(np.asarray(wdata, F), want['weight'], 'script weight')
    # the default weighting: frames of equal noise get weights equal to a few per cent (the clipped deviations of ~2500 pixels), so a
    # pixel moves by a few per cent of the spread of its values, which is below the brightest pixel
    out2 = str(sc['dir'] / 'out2.fits')
    assert script.main([out2] + sc['names'] + ['--transforms', sc['yml'], '--image_size', '80,70', '-l', 'ERROR']) == 0
    data2, h2 = fitsio.read(out2)
    assert data2.shape == (70, 80) and h2['DRIZNREJ'] == 0
    ok = np.isfinite(data2)
    assert ok.mean() > 0.9 and np.abs(data2[ok] - want['image'][:70, :80][ok]).max() < 0.05 * np.nanmax(want['image'])


def test_script_reject(star_files):
    """--reject: every injected hit is flagged (DRIZNREJ >= 40) and the sky, where the hits are, comes out closer to the drizzle of the
    hit-free frames than without the flags."""
    from astrophotography_amd import fitsio
    from astrophotography_amd.scripts import ap_drizzle as script
    sc = star_files
    N = len(sc['names'])
    out = str(sc['dir'] / 'rej.fits')
    assert script.main([out] + sc['names'] + ['--transforms', sc['yml'], '--reject', '--no_weighting', '-l', 'ERROR']) == 0
    data, h = fitsio.read(out)
    assert h['DRIZNREJ'] >= len(sc['hits'])
    truth = dm.drizzle(sc['clean_frames'], sc['affines'], 2, 0.5, fscale=np.full(N, 0.5))['image']
    plain = dm.drizzle(sc['frames'], sc['affines'], 2, 0.5, fscale=np.full(N, 0.5))['image']
    vv, uu = np.mgrid[0:truth.shape[0], 0:truth.shape[1]]
    sky = np.isfinite(truth) & np.isfinite(data)
    for x, y, _ in sc['stars']:
        sky &= np.hypot((uu + 0.5) / 2 - 0.5 - x, (vv + 0.5) / 2 - 0.5 - y) > 5
    rms0 = np.sqrt(np.mean((plain[sky].astype(np.float64) - truth[sky]) ** 2))
    rms1 = np.sqrt(np.mean((np.asarray(data, F)[sky].astype(np.float64) - truth[sky]) ** 2))
    print('DRIZNREJ %d (hits %d); sky rms against the hit-free drizzle %.4f without, %.4f with the flags' % (h['DRIZNREJ'], len(sc['hits']), rms0, rms1))
    assert rms1 < rms0


def test_class_cfa_files(star_files):
    """cfa: three planes from the frames read as RGGB mosaics, each the model's plane bit for bit; rejection is refused."""
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio
    from astrophotography_amd.scripts import ap_drizzle as script
    sc = star_files
    N = len(sc['names'])
    out = str(sc['dir'] / 'colour.fits')
    assert script.main([out] + sc['names'] + ['--transforms', sc['yml'], '--cfa', '--pattern', 'RGGB', '--no_weighting', '-l', 'ERROR']) == 0
    for c, n in enumerate('rgb'):
        data, h = fitsio.read(str(sc['dir'] / ('colour_%s.fits' % n)))
        assert h['COMBINET'] == 'DRIZZLE' and h['DRIZCHAN'] == 'RGB'[c]
        want = dm.drizzle(sc['frames'], sc['affines'], 2, 0.5, fscale=np.full(N, 0.5), cfa=(dm.COLOURS['RGGB'], c))
        _same_bits(np.asarray(data, F), want['image'], 'cfa plane ' + n)
    with pytest.raises(ValueError, match='CFA'):
        ap.ApDrizzle('ERROR', reject=True).drizzle_files(sc['names'], sc['affines'], out, cfa=True, pattern='RGGB')
    with pytest.raises(RuntimeError, match='Bayer'):
        ap.ApDrizzle('ERROR').drizzle_files(sc['names'], sc['affines'], out, cfa=True)
