"""F8 on the GPU: the registration kernels (csrc/register.hip) and ops.register_lists against the NumPy model
(tests/register_model.py), and one image-level round trip find stars -> register -> resample -> find stars.

PARITY UNPINNED (nothing in the reference does this step): the model is the rule of DESIGN 4.3e, the truth a known transform.
Triangle lists are compared as sets with bit-equal invariants, votes and neighbour indices exactly.  The vote inputs are
chosen so that the model's margin (the smallest relative distance of any comparison to its threshold) is >= 1e-9, seven
orders above a last-bit difference: then exact equality is the right demand.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import register_model as rm  # noqa: E402

pytestmark = pytest.mark.gpu


def _ops():
    from astrophotography_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _field(seed=21, rot=178.3, scale=1.004):
    A = rm.make_affine(rot, scale, shift=(11.0, -21.0))
    p0, p1, truth, sigma = rm.make_field(seed, A)
    return p0, p1, truth, sigma, A


def _ulps(a, b):
    return int(np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64)).max()) if len(a) else 0


def _check_triangles(xy, count, K, min_side=5.0):
    ops = _ops()
    tri = ops.triangle_build(xy, count, K=K, min_side=min_side)
    dev = ops.triangle_unpack(tri)
    model, _ = rm.triangle_build(xy, count, K=K, min_side=min_side)
    assert tri['count'].cpu().numpy().tolist() == [len(m['x']) for m in model]
    for d, m in zip(dev, model):
        ds, ms = rm.triangle_set(d), rm.triangle_set(m)
        assert ds.keys() == ms.keys()
        keys = sorted(ms)
        ulp = _ulps([ds[k] for k in keys], [ms[k] for k in keys]) if keys else 0
        print('K = %d: %d triangles, invariants differ by at most %d ulp' % (K, len(keys), ulp))
        assert ulp == 0
    return tri, model


# -- triangles -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [3, 4, 17, 40, 64])
def test_triangles_match_model(K):
    p0, p1 = _field()[:2]
    xy, count = rm.pad_lists([p0, p1])
    _, model = _check_triangles(xy, count, K)
    if K >= 17:
        assert all(len(m['x']) > 0 for m in model)


def test_triangles_short_and_empty_lists():
    p0, p1 = _field()[:2]
    xy, count = rm.pad_lists([p0[:10], p1[:40]])
    _check_triangles(xy, count, 40)                                      # a list shorter than K
    xy, count = rm.pad_lists([p0[:40], p0[:0], p0[:2], p0[:3]], M=40)
    assert count.tolist() == [40, 0, 2, 3]
    tri, model = _check_triangles(xy, count, 40)
    assert [len(m['x']) for m in model][1:3] == [0, 0]


def test_triangles_degenerate_triples():
    """Collinear stars (orientation 0, kept), two stars at one position (a zero side), an exactly isosceles triple both ways
    round (a2 == b2 and b2 == c2: the stable tie rule decides the vertices; x <= 0.98 and y <= 0.98 x then drop them) and an
    equilateral one as nearly as float64 coordinates allow, among ordinary stars."""
    s3 = np.sqrt(3.0)
    pts = np.array([[0.0, 0.0], [20.0, 0.0], [8.0, 0.0],                 # collinear
                    [100.0, 100.0], [100.0, 100.0],                      # coincident
                    [200.0, 0.0], [260.0, 0.0], [230.0, 40.0],           # isosceles: 50, 50, 60
                    [300.0, 300.0], [400.0, 300.0], [350.0, 300.0 + 10.0],   # isosceles with the equal sides longest
                    [500.0, 0.0], [564.0, 0.0], [532.0, 32.0 * s3],      # equilateral
                    [37.5, 411.25], [811.0, 77.5], [640.25, 903.0]])
    xy, count = rm.pad_lists([pts, pts[::-1].copy()])
    _, model = _check_triangles(xy, count, len(pts))
    sets = rm.triangle_set(model[0])
    assert (1, 0, 2, 0) in sets and sets[(1, 0, 2, 0)] == (0.6, 0.4)
    assert not any({3, 4} <= set(k[:3]) for k in sets)
    assert (5, 6, 7) not in {tuple(sorted(k[:3])) for k in sets} and (8, 9, 10) not in {tuple(sorted(k[:3])) for k in sets}
    _check_triangles(xy, count, len(pts), min_side=0.0)                  # the zero side now reaches the 0 / 0 and y >= 0.1 rules


def test_triangle_arguments_are_checked():
    ops = _ops()
    xy, count = rm.pad_lists([_field()[0]])
    for K in (2, 65):
        with pytest.raises(ValueError):
            ops.triangle_build(xy, count, K=K)


# -- votes -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vote_case(K, F):
    p0, p1, _, _, A = _field()
    frames = [p0, p1]
    if F == 5:
        other = rm.make_field(77, rm.make_affine())[0]
        p4 = rm.make_field(21, rm.make_affine(-3.0, 0.999, shift=(40.0, 9.0)))[1]   # the same sky (seed) under another transform
        frames = [p0, p1, other, p0[:2], p4]
    xy, count = rm.pad_lists(frames)
    tris, m1 = rm.triangle_build(xy, count, K=K)
    model = {}
    for mirror in (False, True):
        model[mirror] = rm.triangle_vote(tris, K=K, allow_mirror=mirror)
    return xy, count, tris, m1, model


@pytest.mark.parametrize('mirror', [False, True])
@pytest.mark.parametrize('K,F', [(8, 2), (8, 5), (33, 2), (33, 5), (64, 2)])
def test_votes_match_model(K, F, mirror):
    ops = _ops()
    xy, count, tris, m1, model = _vote_case(K, F)
    votes_model, m2 = model[mirror]
    print('K = %d, F = %d: triangles %s, margin %.2e (build), %.2e (vote)' % (K, F, [len(t['x']) for t in tris], m1, m2))
    assert min(m1, m2) >= 1e-9
    if K >= 33:
        assert any(len(t['x']) % 64 and len(t['x']) % 256 for t in tris)
        assert votes_model[1].max() >= 10
    tri = ops.triangle_build(xy, count, K=K)
    votes = ops.triangle_vote(tri, allow_mirror=mirror).cpu().numpy()
    again = ops.triangle_vote(tri, allow_mirror=mirror).cpu().numpy()
    assert votes.dtype == np.int32 and votes.shape == (F, K, K)
    assert np.array_equal(votes, votes_model)
    assert np.array_equal(votes, again)
    assert not votes[0].any()
    if F == 5:
        assert len(tris[3]['x']) == 0 and not votes[3].any()
    if mirror:
        assert (votes >= model[False][0]).all()


# -- nearest neighbours ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_ref', [0, 1, 65, 1000, 4096])
def test_nearest_match_model(n_ref):
    ops = _ops()
    rng = np.random.default_rng(n_ref + 5)
    M = 4096
    sky = rng.uniform(0.0, 2047.0, size=(M, 2))
    counts = [n_ref, 0, 1, 65, 1000] + ([4096] if n_ref in (0, 1, 4096) else [])
    T = [rm.IDENTITY] + [rm.make_affine(7.0 * f, 1.0 + 0.001 * f, shift=(3.0 * f, -2.0 * f)) for f in range(1, len(counts))]
    lists = [sky[:n_ref]]
    for f in range(1, len(counts)):
        pick = rng.permutation(M)[:counts[f]]
        lists.append(rm.apply_affine(T[f], sky[pick]) + rng.normal(0.0, 0.7, size=(counts[f], 2)))
    xy, count = rm.pad_lists(lists, M=M)
    assert count.tolist() == counts
    fi, fd, bi, bd, _ = rm.nearest_match(xy, count, np.array(T), 2.0)
    r = ops.nearest_match(xy, count, np.array(T), 2.0)
    for name, want in (('fwd_idx', fi), ('fwd_d2', fd), ('bwd_idx', bi), ('bwd_d2', bd)):
        got = r[name].cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(got, want), name
    if n_ref >= 1000:
        assert (fi[4] >= 0).sum() > 100 and (fi[4] < 0).sum() > 100


def test_nearest_match_ties_and_radius():
    ops = _ops()
    ref = np.array([[10.0, 10.0], [50.0, 50.0], [200.0, 200.0], [300.0, 300.0]])
    frm = np.array([[13.0, 10.0], [7.0, 10.0], [10.0, 13.0], [53.0, 54.0], [90.0, 90.0], [200.0, 205.0], [200.0, 195.0]])
    xy, count = rm.pad_lists([ref, frm])
    T = np.tile(rm.IDENTITY, (2, 1))
    for radius in (3.0, 5.0, np.nextafter(5.0, 0.0)):
        want = rm.nearest_match(xy, count, T, radius)
        r = ops.nearest_match(xy, count, T, radius)
        for name, w in zip(('fwd_idx', 'fwd_d2', 'bwd_idx', 'bwd_d2'), want):
            assert np.array_equal(r[name].cpu().numpy(), w), (name, radius)
    fwd = ops.nearest_match(xy, count, T, 5.0)
    assert fwd['fwd_idx'][1, :4].tolist() == [0, 3, 5, -1]               # three- and two-way ties: the lowest index; d2 == 25 is inside
    assert fwd['fwd_d2'][1, :2].tolist() == [9.0, 25.0]
    assert ops.nearest_match(xy, count, T, float(np.nextafter(5.0, 0.0)))['fwd_idx'][1, 1].item() == -1
    # a rotation by 90 degrees about the origin, exact in float64: (x, y) -> (-y, x)
    T[1] = [0.0, -1.0, 0.0, 1.0, 0.0, 0.0]
    xy2, count2 = rm.pad_lists([ref, np.array([[-10.0, 10.0], [-50.0, 53.0]])])
    r = ops.nearest_match(xy2, count2, T, 3.0)
    assert r['fwd_idx'][1, :4].tolist() == [0, 1, -1, -1] and r['fwd_d2'][1, :2].tolist() == [0.0, 9.0]
    assert r['bwd_idx'][1, :2].tolist() == [0, 1]


# -- ops.register_lists ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch():
    p0, p1, truth1, sigma, A1 = _field()
    A3 = rm.make_affine(3.0, 1.0, shift=(20.0, 30.0), shear=0.01)
    _, p3, truth3, _ = rm.make_field(21, A3)
    other = rm.make_field(77, rm.make_affine())[0]
    return [p0, p1, other, p3], {1: (A1, truth1), 3: (A3, truth3)}, sigma


def test_register_lists_matches_model_and_truth():
    ops = _ops()
    lists, truth, sigma = _batch()
    xy, count = rm.pad_lists(lists)
    want, margin = rm.register_lists(xy, count)
    got = ops.register_lists(xy, count)
    assert margin >= 1e-9
    assert got['ok'].tolist() == want['ok'].tolist() == [True, True, False, True]
    assert np.array_equal(got['votes'].cpu().numpy(), want['votes'])
    assert got['n_seed'].tolist() == want['n_seed'].tolist() and got['n_matched'].tolist() == want['n_matched'].tolist()
    assert np.isnan(got['coeffs'][2]).all()
    alone = ops.register_lists(*rm.pad_lists([lists[0], lists[1], lists[3]]))
    for f, (A, pairs) in truth.items():
        assert np.array_equal(got['pairs'][f], want['pairs'][f])
        assert rm.corner_error(got['coeffs'][f], want['coeffs'][f]) <= 1e-9
        n = int(got['n_matched'][f])
        err, bound = rm.corner_error(got['coeffs'][f], A), 5.0 * sigma * np.sqrt(7.0 / n)
        print('frame %d: %d seeds, %d matched, rms %.3f, corner error %.4f (bound %.4f)' % (f, got['n_seed'][f], n, got['rms'][f], err, bound))
        assert err <= bound
        truth_set = set(map(tuple, pairs))
        found = set(map(tuple, got['pairs'][f]))
        assert found <= truth_set and all(tuple(t) in found for t in pairs if t[0] < 40 and t[1] < 40)
        assert np.array_equal(alone['coeffs'][{1: 1, 3: 2}[f]], got['coeffs'][f])    # the unrelated frame changes nothing
    assert np.array_equal(got['coeffs'][0], rm.IDENTITY)


def test_register_lists_refuses():
    ops = _ops()
    p0, p1, _, _, A = _field()
    mirrored = rm.apply_affine(rm.make_affine(mirror=True), p1)
    for n in (0, 1, 2):
        got = ops.register_lists(*rm.pad_lists([p0, p1[:n], p1]))
        assert got['ok'].tolist() == [True, False, True]
    xy, count = rm.pad_lists([p0, mirrored])
    assert not ops.register_lists(xy, count)['ok'][1]
    got = ops.register_lists(xy, count, allow_mirror=True)
    want, _ = rm.register_lists(xy, count, allow_mirror=True)
    assert got['ok'][1] and np.array_equal(got['pairs'][1], want['pairs'][1])
    assert rm.corner_error(got['coeffs'][1], want['coeffs'][1]) <= 1e-9
    assert got['coeffs'][1][0] * got['coeffs'][1][4] - got['coeffs'][1][1] * got['coeffs'][1][3] < 0


# -- images ----------------------------------------------------------------------------------------------------------------
def _render(pos, ampl, size, rng, fwhm=3.0, sky=400.0):
    """Gaussian stars sampled at the pixel centres (integer coordinate = pixel centre), sky, Gaussian noise of the Poisson size."""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    s2 = (fwhm / 2.35482) ** 2
    img = np.full((size, size), sky)
    for (x, y), a in zip(pos, ampl):
        if -10 < x < size + 10 and -10 < y < size + 10:
            y0, y1, x0, x1 = max(0, int(y) - 12), min(size, int(y) + 13), max(0, int(x) - 12), min(size, int(x) + 13)
            img[y0:y1, x0:x1] += a * np.exp(-((xx[y0:y1, x0:x1] - x) ** 2 + (yy[y0:y1, x0:x1] - y) ** 2) / (2.0 * s2))
    return (img + rng.normal(0.0, 1.0, size=img.shape) * np.sqrt(img)).astype(np.float32)


def _centroid_pairs(found, truth, radius=1.5):
    """For every found position the nearest truth position within `radius`: (found - truth) [n, 2]."""
    d = found[:, None, :] - truth[None, :, :]
    d2 = (d ** 2).sum(axis=2)
    j = d2.argmin(axis=1)
    ok = d2[np.arange(len(found)), j] <= radius * radius
    return d[np.arange(len(found)), j][ok]


def test_image_round_trip_512():
    """find stars -> ApRegister.register_images -> resample_affine -> find stars: the centroids of the resampled frame fall on
    the reference frame's.  Bounds from sigma_c, the per-axis rms centroid error of the star finder (code that was there
    before F8) against the rendered truth on these two frames: corner error of the map <= 5 sigma_c sqrt(7 / n_matched),
    per-axis rms of the paired centroid differences after resampling <= 3 sigma_c sqrt(2).
    Measured on an MI355X: see DESIGN 4.3e."""
    import torch
    import astrophotography_amd as ap
    ops = _ops()
    size = 512
    rng = np.random.default_rng(2026)
    pos = []
    while len(pos) < 80:                                                 # at least 14 px apart, 20 px inside the frame
        c = rng.uniform(20.0, size - 21.0, size=2)
        if all((c[0] - q[0]) ** 2 + (c[1] - q[1]) ** 2 >= 14.0 ** 2 for q in pos):
            pos.append(c)
    pos = np.array(pos)
    ampl = 10.0 ** rng.uniform(np.log10(600.0), np.log10(30000.0), size=len(pos))
    A = rm.make_affine(1.2, 1.0, shift=(13.4, -7.8), centre=(255.5, 255.5))
    pos1 = rm.apply_affine(A, pos)
    img0 = torch.from_numpy(_render(pos, ampl, size, rng)).cuda()
    img1 = torch.from_numpy(_render(pos1, ampl, size, rng)).cuda()

    def centroids(img):
        t = ap.ApFindStars.from_device(img, loglevel='ERROR')._phot_table
        return np.stack([t['xcenter'], t['ycenter']], axis=1)

    c0, c1 = centroids(img0), centroids(img1)
    e = np.concatenate([_centroid_pairs(c0, pos), _centroid_pairs(c1, pos1)])
    assert len(e) >= 120
    sigma_c = float(np.sqrt(np.mean(e ** 2)))
    reg = ap.ApRegister('ERROR')
    r = reg.register_images([img0, img1])
    assert r['ok'].tolist() == [True, True]
    n = int(r['n_matched'][1])
    corner = rm.corner_error(r['coeffs'][1], A, size=size)
    res, _ = ops.resample_affine(img1[None], reg.affines()[1:])
    back = torch.nan_to_num(res[0], nan=400.0)
    d = _centroid_pairs(centroids(back), c0)
    rms = float(np.sqrt(np.mean(d ** 2)))
    print('sigma_c %.4f px; %d matched, corner error %.4f px (bound %.4f); %d pairs after resampling, rms %.4f px (bound %.4f)'
          % (sigma_c, n, corner, 5.0 * sigma_c * np.sqrt(7.0 / n), len(d), rms, 3.0 * sigma_c * np.sqrt(2.0)))
    assert n >= 50 and len(d) >= 50
    assert corner <= 5.0 * sigma_c * np.sqrt(7.0 / n)
    assert rms <= 3.0 * sigma_c * np.sqrt(2.0)
