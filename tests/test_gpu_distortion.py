"""F19 on the GPU (DESIGN 4.3e'): the polynomial neighbour search (csrc/register.hip), the tile affines (csrc/distortion.hip) and the
per-tile drizzle and rejection (csrc/drizzle.hip) against the NumPy model tests/distortion_model.py, bit for bit; ops.register_lists
with a polynomial model on the planted scene; one image-level round trip; the argument checks; and the four new entry points under
the guard of tests/guard.py, through the catalogue's own runner (tests/test_gpu_guard.py counts them as covered from there).

PARITY UNPINNED (nothing in the reference does this): the model is the rule of DESIGN 4.3e', the truth a planted map.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distortion_model as dm  # noqa: E402
import drizzle_model as drm  # noqa: E402
import register_model as rm  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SIGMA = 0.05
WORST_POLY3 = 0.0553                                                  # the model's figure (tests/test_distortion_model_host.py, DESIGN 4.3e')


def _ops():
    from astrophotography_amd import ops
    return ops


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _maps(coef, x0, y0, L):
    from astrophotography_amd.distortion import PolyMap
    return [PolyMap(c[0], c[1], (x0, y0), L) for c in coef]


def _random_coef(d, rng, n, size=2048.0, px=3.0):
    """n maps of degree d: a small rotation, scale and shift each, plus random terms of every degree 2 .. d, about px in all at the
    corner."""
    x0, y0 = 0.5 * size - 3.0, 0.5 * size + 5.0
    L = float(np.hypot(x0, y0))
    coef = []
    for f in range(n):
        c = dm.from_affine(rm.make_affine(1.5 * f, 1.0 + 1e-3 * f, shift=(3.0 * f, -2.0 * f), centre=(x0, y0)), d, x0, y0, L)
        for k, (i, j) in enumerate(dm.exponents(d)):
            if i + j >= 2:
                c[:, k] = rng.uniform(-1.0, 1.0, 2) * px / max(d - 1, 1) / (i + j + 1)
        coef.append(c)
    return np.stack(coef), x0, y0, L


# -- nearest neighbours -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nearest_case(d):
    """F = 3: the reference and frame 2 hold 1100 stars - more than one LDS chunk of 1024 in both directions -, frame 1 holds 300."""
    rng = np.random.default_rng(100 + d)
    coef, x0, y0, L = _random_coef(d, rng, 3)
    sky = rng.uniform(0.0, 2047.0, size=(1100, 2))
    lists = [sky]
    for f, n in ((1, 300), (2, 1100)):
        pick = rng.permutation(1100)[:n]
        X, Y = dm.evaluate(coef[f], x0, y0, L, sky[pick, 0], sky[pick, 1])
        lists.append(np.stack([X, Y], axis=1) + rng.normal(0.0, 0.3, size=(n, 2)))
    xy, count = rm.pad_lists(lists, M=1100)
    want = {radius: dm.nearest_match(xy, count, coef, x0, y0, L, radius) for radius in (0.5, 3.0)}
    return xy, count, coef, x0, y0, L, want


@pytest.mark.parametrize('d', [1, 2, 3, 4, 5])
def test_nearest_match_poly_equals_the_model(d):
    ops = _ops()
    xy, count, coef, x0, y0, L, want = _nearest_case(d)
    assert count.tolist() == [1100, 300, 1100]
    for radius, (fi, fd, bi, bd, margin) in want.items():
        print('degree %d, radius %g: margin %.2e; %d of 1100 reference stars matched in frame 2' % (d, radius, margin, (fi[2] >= 0).sum()))
        assert margin >= 1e-9                                            # no decision of the model within rounding of its threshold
        assert 100 < (fi[2] >= 0).sum() < 1100 or radius == 3.0
        r = ops.nearest_match(xy, count, None, radius, maps=_maps(coef, x0, y0, L))
        for name, w in (('fwd_idx', fi), ('bwd_idx', bi)):
            got = r[name].cpu().numpy()
            assert got.dtype == w.dtype and np.array_equal(got, w), (name, radius)
        for name, w in (('fwd_d2', fd), ('bwd_d2', bd)):
            assert np.array_equal(_bits(r[name].cpu().numpy()), _bits(w)), (name, radius)
    # the tuple form of maps= is the same call
    r2 = ops.nearest_match(xy, count, None, 3.0, maps=(coef, (x0, y0), L))
    assert np.array_equal(r2['fwd_idx'].cpu().numpy(), want[3.0][0])


def test_nearest_match_degree_1_equals_the_affine_entry_point():
    """The same neighbours as apgpu_nearest_match; d2 within the rounding of the two forms ((c0 + c1 u) + c2 v against (a0 x + a1 y)
    + a2), and bit-equal where both are exact (integer coordinates, a rotation by 90 degrees)."""
    ops = _ops()
    xy, count, _, _, _, _, _ = _nearest_case(1)
    from astrophotography_amd.distortion import PolyMap
    T = np.stack([rm.IDENTITY, rm.make_affine(1.5, 1.001, shift=(3.0, -2.0), centre=(1021.0, 1029.0)),
                  rm.make_affine(3.0, 1.002, shift=(6.0, -4.0), centre=(1021.0, 1029.0))])
    maps = [PolyMap.from_affine(t, 1) for t in T]
    for radius in (0.5, 3.0):
        margin = rm.nearest_match(xy, count, T, radius)[4]
        assert margin >= 1e-9
        a, p = ops.nearest_match(xy, count, T, radius), ops.nearest_match(xy, count, None, radius, maps=maps)
        for name in ('fwd_idx', 'bwd_idx'):
            assert np.array_equal(a[name].cpu().numpy(), p[name].cpu().numpy()), (name, radius)
        for name in ('fwd_d2', 'bwd_d2'):
            np.testing.assert_allclose(p[name].cpu().numpy(), a[name].cpu().numpy(), rtol=0, atol=1e-9)
    ref = np.array([[10.0, 10.0], [50.0, 50.0], [200.0, 200.0], [300.0, 300.0]])
    xy2, count2 = rm.pad_lists([ref, np.array([[-10.0, 10.0], [-50.0, 53.0]])])
    T2 = np.array([rm.IDENTITY, [0.0, -1.0, 0.0, 1.0, 0.0, 0.0]])
    a, p = ops.nearest_match(xy2, count2, T2, 3.0), ops.nearest_match(xy2, count2, None, 3.0, maps=[PolyMap.from_affine(t, 1) for t in T2])
    for name in ('fwd_idx', 'fwd_d2', 'bwd_idx', 'bwd_d2'):
        assert np.array_equal(a[name].cpu().numpy(), p[name].cpu().numpy()), name
    assert p['fwd_idx'][1, :4].tolist() == [0, 1, -1, -1] and p['fwd_d2'][1, :2].tolist() == [0.0, 9.0]


# -- tile affines -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 2, 3, 4, 5])
def test_poly_tile_affines_equal_the_model(d):
    """33 x 130 (ragged: 3 x 3 tiles; 2 x 2 at tile_scale 2), the co-add's grid, the OVERSAMPLING grid and the drizzle's (s = 2 and
    1.5, in both forms), N = 1 and 3."""
    ops = _ops()
    rng = np.random.default_rng(200 + d)
    coef, x0, y0, L = _random_coef(d, rng, 3, size=160.0, px=0.05)
    for N in (1, 3):
        for ts, s, composed in ((1, 1.0, True), (2, 2.0, True), (1, 2.0, True), (1, 1.5, True), (1, 2.0, False), (1, 1.5, False), (2, 1.0, True)):
            want = dm.tile_affines(coef[:N], x0, y0, L, (33, 130), ts, s, composed)
            got, est = ops.poly_tile_affines(_maps(coef[:N], x0, y0, L), (33, 130), tile_scale=ts, scale=s, composed=composed)
            assert got.is_cuda and tuple(got.shape) == want.shape == (N, 3 if ts == 1 else 2, 3 if ts == 1 else 2, 6)
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (N, ts, s, composed)
            assert est == max(m.tile_error((33, 130), ts, s) for m in _maps(coef[:N], x0, y0, L)) and (est > 0.0) == (d > 1)


# -- drizzle ------------------------------------------------------------------------------------------------------------------
def _whole_pixel_tiles(N, ty, tx, s, rng, identical=False):
    """Reference pixel -> input pixel per frame and tile: a frame's sub-pixel dither and small rotation, and per tile a whole-pixel
    offset and a magnification of its own - a wrong tile index shows as a shifted, rescaled tile."""
    t = np.empty((N, ty, tx, 6))
    for n in range(N):
        for j in range(ty):
            for i in range(tx):
                k = 0 if identical else 1
                t[n, j, i] = drm.shift_affine(0.25 * n + k * (2 * i - j), -0.5 * n + k * (j - i), 1.0 * n, 1.0 + k * 0.01 * (j * tx + i))
    return t


@pytest.mark.parametrize('N', [1, 3])
def test_drizzle_tiles_equal_the_model(N):
    """Input 40 x 70, s = 2, output 80 x 140: 5 x 3 tiles, the last column and nothing else ragged."""
    ops = _ops()
    rng = np.random.default_rng(300 + N)
    H, W, s = 40, 70, 2.0
    fr = rng.normal(300.0, 40.0, (N, H, W)).astype(F)
    fr[0, 5, 7], fr[-1, 30, 60] = np.nan, np.inf
    mask = (rng.random((H, W)) < 0.1).astype(np.uint8) * 3
    fmask = (rng.random((N, H, W)) < 0.1).astype(np.uint8)
    w, fs = rng.uniform(0.3, 3.0, N), rng.uniform(0.01, 1.0, N)
    tiles = _whole_pixel_tiles(N, 5, 3, s, rng)
    cases = [dict(pixfrac=0.5), dict(pixfrac=0.5, mask=mask), dict(pixfrac=1.0, frame_masks=fmask, weights=w),
             dict(pixfrac=0.5, mask=mask, frame_masks=fmask, fscale=fs, weights=w, conserve_flux=True),
             dict(pixfrac=0.3, cfa=(drm.COLOURS['GRBG'], 1), fscale=fs), dict(pixfrac=0.5, cfa=(drm.COLOURS['RGGB'], 0), frame_masks=fmask)]
    for kw in cases:
        want = dm.drizzle_tiles(fr, tiles, s, **kw)
        dkw = {k: (_dev(v) if k in ('mask', 'frame_masks') else v) for k, v in kw.items()}
        got = ops.drizzle(_dev(fr), tiles, s, **dkw)
        for name in ('image', 'weight'):
            g, wv = got[name].cpu().numpy(), want[name]
            assert g.shape == wv.shape == (80, 140) and g.dtype == np.float32
            assert np.array_equal(np.isnan(g), np.isnan(wv)), (name, sorted(kw))
            bad = (g.view(np.uint32) != wv.view(np.uint32)) & ~np.isnan(wv)
            assert not bad.any(), (name, sorted(kw), int(bad.sum()), np.argwhere(bad)[:5].tolist())
        assert (want['weight'] > 0).mean() > 0.1
        # the per-frame model with any ONE tile's transforms differs from the tiled result outside that tile: the index matters
        one = drm.drizzle(fr, tiles[:, 0, 0], s, **kw)
        assert not np.array_equal(np.nan_to_num(one['image'][16:, 64:]), np.nan_to_num(want['image'][16:, 64:]))
    # a device tensor of tiles (what poly_tile_affines returns) is taken as well as an array
    got2 = ops.drizzle(_dev(fr), _dev(tiles), s, pixfrac=0.5)
    assert np.array_equal(got2['image'].cpu().numpy().view(np.uint32), ops.drizzle(_dev(fr), tiles, s, pixfrac=0.5)['image'].cpu().numpy().view(np.uint32))


def test_identical_tiles_equal_the_per_frame_entry_points():
    ops = _ops()
    rng = np.random.default_rng(33)
    N, H, W, s = 3, 40, 70, 2.0
    fr = rng.normal(300.0, 40.0, (N, H, W)).astype(F)
    fmask = (rng.random((N, H, W)) < 0.1).astype(np.uint8)
    w, fs = rng.uniform(0.3, 3.0, N), rng.uniform(0.01, 1.0, N)
    tiles = _whole_pixel_tiles(N, 5, 3, s, rng, identical=True)
    a = ops.drizzle(_dev(fr), tiles, s, 0.5, frame_masks=_dev(fmask), weights=w, fscale=fs, conserve_flux=True)
    b = ops.drizzle(_dev(fr), tiles[:, 0, 0], s, 0.5, frame_masks=_dev(fmask), weights=w, fscale=fs, conserve_flux=True)
    for name in ('image', 'weight'):
        assert np.array_equal(a[name].cpu().numpy().view(np.uint32), b[name].cpu().numpy().view(np.uint32)), name
    ref = rng.normal(300.0, 40.0, (H, W)).astype(F)
    in_tiles = _whole_pixel_tiles(N, 3, 2, s, rng, identical=True)
    ra = ops.drizzle_reject(_dev(fr), in_tiles, _dev(ref), 1.0, fscale=fs + 0.8, sigmas=[8.0] * N, k=2.0, grow=0.5)
    rb = ops.drizzle_reject(_dev(fr), in_tiles[:, 0, 0], _dev(ref), 1.0, fscale=fs + 0.8, sigmas=[8.0] * N, k=2.0, grow=0.5)
    assert np.array_equal(ra.cpu().numpy(), rb.cpu().numpy()) and 0 < int(ra.sum()) < ra.numel()


@pytest.mark.parametrize('N', [1, 3])
def test_drizzle_reject_tiles_equal_the_model(N):
    """Input 40 x 70: 3 x 2 INPUT tiles, both edges ragged; the reference at ref_scale 1 and 2, with holes."""
    ops = _ops()
    rng = np.random.default_rng(400 + N)
    H, W = 40, 70
    fr = rng.normal(300.0, 40.0, (N, H, W)).astype(F)
    fr[0, 3, 4] = np.nan
    tiles = _whole_pixel_tiles(N, 3, 2, 2.0, rng)
    fs, sig = rng.uniform(0.8, 1.2, N), rng.uniform(5.0, 20.0, N)
    for rs in (1.0, 2.0):
        ref = rng.normal(300.0, 40.0, (int(H * rs), int(W * rs))).astype(F)
        ref[rng.random(ref.shape) < 0.03] = np.nan
        want = dm.drizzle_reject_tiles(fr, tiles, ref, ref_scale=rs, fscale=fs, sigmas=sig, k=2.0, grow=0.5)
        got = ops.drizzle_reject(_dev(fr), tiles, _dev(ref), rs, fscale=fs, sigmas=sig, k=2.0, grow=0.5).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want), (rs, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
        assert 0 < int(want.sum()) < want.size
        one = drm.drizzle_reject(fr, tiles[:, 0, 0], ref, rs, fscale=fs, sigmas=sig, k=2.0, grow=0.5)
        assert not np.array_equal(one, want)


def test_input_tile_affines_equal_the_model_and_invert_the_map():
    ops = _ops()
    rng = np.random.default_rng(9)
    coef, x0, y0, L = _random_coef(3, rng, 2, size=160.0, px=0.5)
    got = ops.poly_input_tile_affines(_maps(coef, x0, y0, L), (40, 150))
    want = dm.input_tile_affines(coef, x0, y0, L, (40, 150))
    assert got.shape == (2, 3, 3, 6) and np.array_equal(_bits(got), _bits(want))
    xc, yc = dm.tile_centres((40, 150))
    for f in range(2):                                                   # the tile's transform takes the reference point p back to the centre
        px, py = dm.inverse(coef[f], x0, y0, L, xc, yc)
        assert np.abs(got[f][..., 0] * px + got[f][..., 1] * py + got[f][..., 2] - xc).max() < 1e-10


# -- registration -------------------------------------------------------------------------------------------------------------
def _worst_on_grid(evaluate, planted, size=4096):
    g = np.linspace(0.0, size - 1.0, 65)
    gx, gy = np.meshgrid(g, g)
    X, Y = evaluate(gx, gy)
    TX, TY = planted(gx, gy)
    return float(np.hypot(X - TX, Y - TY).max())


def test_register_lists_poly3_on_the_planted_scene():
    """F = 3: the reference, the planted frame and the first 20 stars of the planted frame.  The host test's three assertions: the affine
    leaves more than 0.3 px rms, the polynomial's rms is the noise to 10 %, its worst error against the planted map on a 65 x 65
    grid is at most twice the model's figure.  The pairs are the model's; the short frame keeps its affine (order 1)."""
    ops = _ops()
    ref, frm, planted = dm.planted_scene()
    xy, count = rm.pad_lists([ref, frm, frm[:20]])
    got = ops.register_lists(xy, count, model='poly3')
    affine = ops.register_lists(xy, count, model='affine')
    assert got['ok'].tolist() == [True, True, True] and got['order'].tolist() == [1, 3, 1]
    assert np.array_equal(_bits(got['coeffs']), _bits(affine['coeffs']))                 # coeffs stays the affine of step 5
    assert np.array_equal(_bits(got['rms_affine']), _bits(affine['rms'])) and got['rms'][2] == affine['rms'][2]
    m = got['maps'][1]
    worst = _worst_on_grid(m.eval, planted)
    noise = SIGMA * np.sqrt(2.0)
    print('affine rms %.4f px; degree 3: %d pairs, rms %.4f px (noise %.4f), worst %.4f px' % (got['rms_affine'][1], got['n_matched'][1], got['rms'][1], noise, worst))
    assert got['rms_affine'][1] > 0.3
    assert abs(got['rms'][1] - noise) <= 0.1 * noise
    assert worst <= 2.0 * WORST_POLY3
    want = dm.refine(ref, frm, affine['coeffs'][1], affine['rms'][1], 3, frame=(got['origin'][0], got['origin'][1], got['scale']))
    assert want['margin'] >= 1e-9 and want['order'] == 3
    assert (got['origin'][0], got['origin'][1], got['scale']) == dm.bbox_frame(ref)
    assert np.array_equal(got['pairs'][1], want['pairs']) and np.array_equal(_bits(np.stack([m.cx, m.cy])), _bits(want['coef']))
    assert got['maps'][2].degree == 3 and np.abs(got['maps'][2].affine_part() - got['coeffs'][2]).max() < 1e-9
    assert got['maps'][0].degree == 3 and np.abs(got['maps'][0].affine_part() - rm.IDENTITY).max() < 1e-12
    with pytest.raises(ValueError):
        ops.register_lists(xy, count, model='poly6')
    with pytest.raises(ValueError):
        ops.register_lists(xy, count, model='poly1')


def _round_trip(model, img0, img1, c0, centroids):
    import astrophotography_amd as ap
    import torch
    ops = _ops()
    reg = ap.ApRegister('ERROR', model=model)
    r = reg.register_images([img0, img1])
    assert r['ok'].tolist() == [True, True]
    if model == 'affine':
        assert reg.maps() is None
        res, _ = ops.resample_affine(img1[None], reg.affines()[1:])
    else:
        # 2 px over 256 px is a hundred times the curvature of the 4096 x 4096 probe: its tiles cost 0.03 px, a quarter of the bound
        tiles, est = ops.poly_tile_affines(reg.maps()[1:], tuple(img0.shape), max_tile_error=0.05)
        assert 0.01 < est < 0.05
        res, _ = ops.resample_affine(img1[None], tiles)
    from tests.test_gpu_register import _centroid_pairs
    d = _centroid_pairs(centroids(torch.nan_to_num(res[0], nan=400.0)), c0)
    return r, float(np.sqrt(np.mean(d ** 2))), len(d)


def test_image_round_trip_512_needs_the_polynomial():
    """find stars -> ApRegister.register_images(model) -> poly_tile_affines -> resample_affine -> find stars, on 80 rendered stars
    under the planted map scaled to 2 px at the corner (1.4 px cubic, 0.6 px quadratic).  With 'poly3' the per-axis rms of the
    paired centroid differences meets the bound of test_gpu_register.py::test_image_round_trip_512, 3 sigma_c sqrt 2; with 'affine'
    the same chain exceeds it: the scene needs the feature.  Measured on an MI355X: sigma_c 0.0270 px, bound 0.1147 px, 'poly3' 0.0288 px,
    'affine' 0.1431 px (DESIGN 4.3e')."""
    import astrophotography_amd as ap
    import torch
    from tests.test_gpu_register import _centroid_pairs, _render
    size = 512
    rng = np.random.default_rng(2027)
    pos = []
    while len(pos) < 80:
        c = rng.uniform(20.0, size - 21.0, size=2)
        if all((c[0] - q[0]) ** 2 + (c[1] - q[1]) ** 2 >= 14.0 ** 2 for q in pos):
            pos.append(c)
    pos = np.array(pos)
    ampl = 10.0 ** rng.uniform(np.log10(600.0), np.log10(30000.0), size=len(pos))
    planted = dm.planted_map(size, rot_deg=1.2, cubic_px=1.4, quad_px=0.6, shift=(5.4, -3.8))
    pos1 = np.stack(planted(pos[:, 0], pos[:, 1]), axis=1)
    img0 = torch.from_numpy(_render(pos, ampl, size, rng)).cuda()
    img1 = torch.from_numpy(_render(pos1, ampl, size, rng)).cuda()

    def centroids(img):
        t = ap.ApFindStars.from_device(img, loglevel='ERROR')._phot_table
        return np.stack([t['xcenter'], t['ycenter']], axis=1)

    c0, c1 = centroids(img0), centroids(img1)
    e = np.concatenate([_centroid_pairs(c0, pos), _centroid_pairs(c1, pos1)])
    assert len(e) >= 120
    sigma_c = float(np.sqrt(np.mean(e ** 2)))
    bound = 3.0 * sigma_c * np.sqrt(2.0)
    r3, rms3, n3 = _round_trip('poly3', img0, img1, c0, centroids)
    ra, rmsa, na = _round_trip('affine', img0, img1, c0, centroids)
    print('sigma_c %.4f px, bound %.4f px; poly3: order %d, %d matched, %d pairs after resampling, rms %.4f px; affine: %d pairs, rms %.4f px'
          % (sigma_c, bound, r3['order'][1], r3['n_matched'][1], n3, rms3, na, rmsa))
    assert r3['order'][1] == 3 and n3 >= 50 and na >= 50
    assert rms3 <= bound
    assert rmsa > bound


# -- argument checks --------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked():
    from astrophotography_amd import _lib
    from astrophotography_amd.distortion import PolyMap
    ops = _ops()
    xy, count = rm.pad_lists([np.array([[1.0, 2.0], [30.0, 40.0]])] * 2)
    ident = lambda d: dm.from_affine(rm.IDENTITY, d, 0.0, 0.0, 1.0)
    bad_sets = [(np.zeros((2, 2, 1)), 'degree 0'), (np.zeros((2, 2, 28)), 'degree 6'), (np.zeros((2, 2, 7)), 'no degree holds 7 coefficients'),
                (np.stack([ident(2), np.where(np.arange(6) == 4, np.nan, ident(2))]), 'a NaN coefficient'),
                (np.stack([ident(2), np.where(np.arange(6) == 1, np.inf, ident(2))]), 'an infinite coefficient'),
                (np.zeros((2, 3, 6)), 'three axes'), (np.stack([ident(2)]), 'one map for two frames')]
    for coef, what in bad_sets:
        with pytest.raises(ValueError):
            ops.nearest_match(xy, count, None, 3.0, maps=(coef, (0.0, 0.0), 1.0))
        if coef.shape[0] == 2:
            with pytest.raises(ValueError):
                ops.poly_tile_affines((coef, (0.0, 0.0), 1.0), (33, 130))
    good = [PolyMap.from_affine(rm.IDENTITY, 2)] * 2
    with pytest.raises(ValueError):
        ops.nearest_match(xy, count, None, 3.0, maps=[good[0], PolyMap.from_affine(rm.IDENTITY, 3)])     # two degrees in one call
    for kw in (dict(tile_scale=0), dict(tile_scale=17), dict(scale=0.0), dict(scale=float('nan'))):
        with pytest.raises(ValueError):
            ops.poly_tile_affines(good, (33, 130), **kw)
    with pytest.raises(ValueError):
        ops.poly_tile_affines(good, (0, 130))
    # a map too curved for its tiles is refused, and taken when the caller allows the error
    curved = [PolyMap([0.0, 100.0, 0.0, 40.0, 0.0, 0.0], [0.0, 0.0, 100.0, 0.0, 0.0, 0.0], (50.0, 50.0), 100.0)]
    with pytest.raises(ValueError, match='max_tile_error'):
        ops.poly_tile_affines(curved, (100, 100))
    assert ops.poly_tile_affines(curved, (100, 100), max_tile_error=10.0)[1] > 0.01
    # the library refuses what the wrapper would: degree, L, scale, tile_scale
    lib = _lib.load()
    d = _dev(np.zeros(64))
    p = lambda t: C.c_void_p(t.data_ptr())
    i32 = _dev(np.zeros(8, np.int32))
    for degree, L in ((0, 1.0), (6, 1.0), (2, 0.0), (2, float('nan'))):
        assert lib.apgpu_poly_tile_affines(p(d), 1, degree, 0.0, 0.0, L, 16, 64, 1, 1.0, 1, p(d), None) == _lib.E_INVAL
        assert lib.apgpu_nearest_match_poly(p(d), p(i32), p(d), degree, 0.0, 0.0, L, 1, 2, 3.0, p(i32), p(d), p(i32), p(d), None) == _lib.E_INVAL
    assert lib.apgpu_poly_tile_affines(p(d), 1, 2, 0.0, 0.0, 1.0, 16, 64, 17, 1.0, 1, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_poly_tile_affines(p(d), 1, 2, 0.0, 0.0, 1.0, 16, 64, 1, 0.0, 1, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_poly_tile_affines(None, 1, 2, 0.0, 0.0, 1.0, 16, 64, 1, 1.0, 1, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_drizzle_tiles_f32(None, 1, 4, 4, None, None, p(d), 0.5, None, 0, p(d), p(d), 4, 4, None) == _lib.E_INVAL
    assert lib.apgpu_drizzle_reject_tiles_u8(p(d), 1, 4, 4, None, p(d), 4, 4, 1.0, 1.0, p(d), None) == _lib.E_INVAL
    # drizzle: a tile array of the wrong shape, a footprint out of (0, 2] in ONE tile, a tile that is not finite
    rng = np.random.default_rng(1)
    fr = _dev(rng.normal(300.0, 40.0, (2, 40, 70)).astype(F))
    tiles = _whole_pixel_tiles(2, 5, 3, 2.0, rng)
    for wrong in (tiles[:, :4], tiles[:, :, :2], tiles[:1], tiles[..., :5], np.concatenate([tiles, tiles], axis=1)):
        with pytest.raises(ValueError):
            ops.drizzle(fr, wrong, 2.0)
    with pytest.raises(ValueError):
        ops.drizzle_reject(fr, tiles, _dev(np.zeros((40, 70), F)))        # output tiles where input tiles (3 x 2) are due
    wide = tiles.copy()
    wide[1, 3, 2, [0, 4]] *= 5.0                                          # 2.5 input pixels per output pixel in that tile alone
    with pytest.raises(ValueError, match='footprint'):
        ops.drizzle(fr, wide, 2.0)
    flat = tiles.copy()
    flat[0, 0, 1, [0, 3]] = 0.0                                           # a footprint of zero width
    with pytest.raises(ValueError, match='footprint'):
        ops.drizzle(fr, flat, 2.0)
    nan = tiles.copy()
    nan[1, 4, 0, 2] = np.nan
    with pytest.raises(ValueError):
        ops.drizzle(fr, nan, 2.0)
    sing = _whole_pixel_tiles(2, 3, 2, 2.0, rng)
    sing[1, 2, 1, [0, 1, 3, 4]] = 0.0
    with pytest.raises(ValueError, match='singular'):
        ops.drizzle_reject(fr, sing, _dev(np.zeros((40, 70), F)))


# -- the guard ----------------------------------------------------------------------------------------------------------------------
def _guard_case(io, shift):
    """The four new entry points with their inputs inside poisoned slabs, against the model."""
    ops = _ops()

    def make():
        rng = np.random.default_rng(77)
        coef, x0, y0, L = _random_coef(3, rng, 3, size=160.0, px=0.3)
        sky = rng.uniform(0.0, 150.0, size=(60, 2))
        lists = [sky] + [np.stack(dm.evaluate(coef[f], x0, y0, L, sky[:n, 0], sky[:n, 1]), axis=1) + rng.normal(0.0, 0.3, (n, 2)) for f, n in ((1, 40), (2, 0))]
        xy, count = rm.pad_lists(lists)
        d = dict(coef=coef, frame=(x0, y0, L), xy=xy, count=count, nn=dm.nearest_match(xy, count, coef, x0, y0, L, 1.0))
        assert d['nn'][4] >= 1e-9
        d['tiles_model'] = dm.tile_affines(coef, x0, y0, L, (33, 130), 1, 2.0, False)
        N, H, W = 2, 20, 70
        d['fr'] = rng.normal(300.0, 40.0, (N, H, W)).astype(F)
        d['mask'] = (rng.random((H, W)) < 0.1).astype(np.uint8)
        d['fmask'] = (rng.random((N, H, W)) < 0.1).astype(np.uint8)
        d['tiles'] = _whole_pixel_tiles(N, 3, 3, 2.0, rng)
        d['w'], d['fs'] = rng.uniform(0.3, 3.0, N), rng.uniform(0.5, 1.0, N)
        d['driz'] = dm.drizzle_tiles(d['fr'], d['tiles'], 2.0, pixfrac=0.5, mask=d['mask'], frame_masks=d['fmask'], weights=d['w'], fscale=d['fs'],
                                     conserve_flux=True)
        d['ref'] = rng.normal(300.0, 40.0, (H, W)).astype(F)
        d['in_tiles'] = _whole_pixel_tiles(N, 2, 2, 2.0, rng)
        d['rej'] = dm.drizzle_reject_tiles(d['fr'], d['in_tiles'], d['ref'], ref_scale=1.0, fscale=d['fs'], sigmas=[8.0] * N, k=2.0, grow=0.5)
        return d
    d = io.once('data', make)
    x0, y0, L = d['frame']
    xy, count = io.dev(np.asarray(d['xy'], np.float64), shift), io.dev(np.asarray(d['count'], np.int32), shift)
    r = ops.nearest_match(xy, count, None, 1.0, maps=_maps(d['coef'], x0, y0, L))
    for name, want in zip(('fwd_idx', 'fwd_d2', 'bwd_idx', 'bwd_d2'), d['nn']):
        io.out('nearest_poly_' + name, r[name], want)
    io.out('tile_affines', ops.poly_tile_affines(_maps(d['coef'], x0, y0, L), (33, 130), scale=2.0, composed=False)[0], d['tiles_model'])
    fr, mask, fmask, ref = io.dev(d['fr'], shift), io.dev(d['mask'], shift), io.dev(d['fmask'], shift), io.dev(d['ref'], shift)
    got = ops.drizzle(fr, d['tiles'], 2.0, 0.5, mask=mask, frame_masks=fmask, weights=d['w'], fscale=d['fs'], conserve_flux=True)
    io.out('drizzle_tiles_image', got['image'], d['driz']['image'])
    io.out('drizzle_tiles_weight', got['weight'], d['driz']['weight'])
    io.out('reject_tiles', ops.drizzle_reject(fr, d['in_tiles'], ref, 1.0, fscale=d['fs'], sigmas=[8.0] * 2, k=2.0, grow=0.5), d['rej'])


@pytest.mark.parametrize('shift', [0, 1])
def test_new_entry_points_under_the_guard(shift, monkeypatch):
    """The protocol of tests/test_gpu_guard.py::test_guarded (runs A, B and C: poison 0xFF, poison 0x00, a side stream) for the entry
    points this feature adds, through that module's runner - which also records them as covered for its own final count."""
    import torch
    import test_gpu_guard as catalogue                                   # the module object pytest collected: its SEEN is the one counted
    fn = lambda io: _guard_case(io, shift)
    memo = {}
    default = torch.cuda.default_stream().cuda_stream
    assert torch.cuda.current_stream().cuda_stream == default
    A, sa = catalogue.run(fn, 0, 0xFF, memo, monkeypatch)
    assert {n for n, _ in sa} == {'apgpu_nearest_match_poly', 'apgpu_poly_tile_affines', 'apgpu_drizzle_tiles_f32', 'apgpu_drizzle_reject_tiles_u8'}
    assert all(s == default for _, s in sa)
    for label, got, ref, tol in A:
        catalogue.compare(got, ref, tol, '%s against the model' % label)
    B, _ = catalogue.run(fn, 0, 0x00, memo, monkeypatch)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Cr, sc = catalogue.run(fn, 0, 0xFF, memo, monkeypatch)
    assert [n for n, _ in sc] == [n for n, _ in sa] and all(s == side.cuda_stream for _, s in sc)
    for tag, other in (('B (poison 0x00)', B), ('C (side stream)', Cr)):
        assert [r[0] for r in other] == [r[0] for r in A]
        for (label, got, _, _), (_, first, _, _) in zip(other, A):
            catalogue.compare(got, first, 'bit', '%s, run %s against run A' % (label, tag))
    assert {'apgpu_nearest_match_poly', 'apgpu_poly_tile_affines', 'apgpu_drizzle_tiles_f32', 'apgpu_drizzle_reject_tiles_u8'} <= catalogue.SEEN
