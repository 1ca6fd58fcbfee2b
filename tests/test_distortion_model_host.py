"""F19 on the host (DESIGN 4.3e'): the NumPy model tests/distortion_model.py and the host half of the feature
(astrophotography_amd/distortion.py, wcs.SipWcs, the transforms file) against what they must do.  No GPU: the kernels are held to
the model bit for bit in tests/test_gpu_distortion.py.

The planted scene is the issue's probe: 4096 x 4096, 600 stars, a pair's centroid difference 0.05 px per axis, a rotation of 1.2
degrees after a cubic radial term of 3 px and a quadratic term of 1.5 px at the corner; seed 20261 (distortion_model.planted_scene).
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distortion_model as dm  # noqa: E402
import register_model as rm  # noqa: E402

from astrophotography_amd import distortion, wcs  # noqa: E402
from astrophotography_amd.distortion import PolyMap  # noqa: E402
from tests.util import load_golden  # noqa: E402

SIGMA = 0.05
# the worst distance between the fitted and the planted map on a 65 x 65 grid over the frame, measured on the model with seed 20261
# (DESIGN 4.3e'); a fit may be twice as far off
WORST_POLY3, WORST_AFFINE = 0.0553, 2.98


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# -- SIP ---------------------------------------------------------------------------------------------------------------------
def test_sip_wcs_matches_astropy_golden():
    """G20: SipWcs against astropy.wcs (all_pix2world, all_world2pix) for SIP orders 2, 3 (with AP / BP) and 4, at G10's tolerances:
    1e-11 degrees on the sky, 1e-8 px on the way back (astropy's own round trip in the capture is 0.8 .. 1.7e-10 px)."""
    g = load_golden('g20_sip_wcs.npz')
    assert int(g['ncases']) == 3
    orders = []
    for i in range(3):
        hdr = json.loads(str(g[f'hdr{i}']))
        w = wcs.from_header(hdr)
        assert isinstance(w, wcs.SipWcs)
        orders.append((hdr['A_ORDER'], w.ap is not None))
        assert float(g[f'roundtrip{i}']) < 1e-9 and 1.5 < float(g[f'distortion_px{i}']) < 6.0
        pix, sky = g[f'pix{i}'], g[f'sky{i}']
        ra, dec = w.pix2sky(pix[:, 0], pix[:, 1])
        dra = (ra - sky[:, 0] + 180.0) % 360.0 - 180.0
        assert np.abs(dra * np.cos(np.deg2rad(dec))).max() < 1e-11 and np.abs(dec - sky[:, 1]).max() < 1e-11
        x, y = w.sky2pix(sky[:, 0], sky[:, 1])
        assert np.abs(x - pix[:, 0]).max() < 1e-8 and np.abs(y - pix[:, 1]).max() < 1e-8
        if w.ap is not None:                                             # AP / BP are a starting point only: the answer without them
            bare = wcs.SipWcs(w.crpix, w.crval, w.cd, w.a, w.b)
            xb, yb = bare.sky2pix(sky[:, 0], sky[:, 1])
            assert np.abs(xb - x).max() < 1e-9 and np.abs(yb - y).max() < 1e-9
    assert orders == [(2, False), (3, True), (4, False)]


def test_from_header_picks_the_class_and_refuses_the_rest():
    g10, g20 = load_golden('g10_wcs.npz'), load_golden('g20_sip_wcs.npz')
    tan, sip = json.loads(str(g10['hdr0'])), json.loads(str(g20['hdr0']))
    assert type(wcs.from_header(tan)) is wcs.TanWcs and type(wcs.from_header(sip)) is wcs.SipWcs
    with pytest.raises(ValueError):
        wcs.TanWcs.from_header(sip)                                      # TanWcs itself keeps refusing a distorted header
    with pytest.raises(ValueError):
        wcs.from_header(dict(sip, PV1_1=0.01))                           # TPV stays refused
    with pytest.raises(ValueError):
        wcs.from_header(dict(tan, PV1_1=0.01))
    with pytest.raises(ValueError):
        wcs.from_header(dict(sip, A_ORDER=6))
    with pytest.raises(ValueError):
        wcs.from_header({k: v for k, v in sip.items() if k != 'B_ORDER'})
    # the output grid is pure TAN: the SIP cards are recognised (to be dropped), the TAN part is a TanWcs with the same linear terms
    w = wcs.from_header(sip)
    assert type(w.tan()) is wcs.TanWcs and w.tan().header_cards()['CTYPE1'] == 'RA---TAN'
    assert all(wcs.is_sip_card(k) for k in sip if k[:2] in ('A_', 'B_')) and not any(wcs.is_sip_card(k) for k in tan)


def test_wcs_tile_affines_follow_a_sip_input():
    """wcs.tile_affines with a SIP input: within 1e-3 px of the exact map over a 1024 x 1024 corner of the frame, where the
    distortion is largest; the same header without its SIP terms is off by pixels there."""
    sip = json.loads(str(load_golden('g20_sip_wcs.npz')['hdr0']))
    inp = wcs.from_header(sip)
    out = inp.tan()
    A = wcs.tile_affines(out, inp, (1024, 1024))
    rng = np.random.default_rng(5)
    x, y = rng.uniform(0, 1023, 4000), rng.uniform(0, 1023, 4000)
    t = A[(y.astype(int) // 16), (x.astype(int) // 64)]
    xin, yin = t[:, 0] * x + t[:, 1] * y + t[:, 2], t[:, 3] * x + t[:, 4] * y + t[:, 5]
    xe, ye = inp.sky2pix(*out.pix2sky(x, y))
    assert np.abs(xin - xe).max() < 1e-3 and np.abs(yin - ye).max() < 1e-3
    assert np.hypot(xe - x, ye - y).max() > 1.0


# -- the map -------------------------------------------------------------------------------------------------------------------
def _random_map(d, rng, size=4096, px=3.0):
    """A rotation and shift plus random terms of every degree 2 .. d, each about px / (d - 1) at the corner."""
    x0 = y0 = (size - 1) / 2.0
    L = float(np.hypot(x0, y0))
    c = dm.from_affine(rm.make_affine(2.0, 1.003, shift=(5.5, -3.25), centre=(x0, y0)), d, x0, y0, L)
    for k, (i, j) in enumerate(dm.exponents(d)):
        if i + j >= 2:
            c[:, k] = rng.uniform(-1.0, 1.0, 2) * px / max(d - 1, 1) / (i + j + 1)
    return c, x0, y0, L


@pytest.mark.parametrize('d', [1, 2, 3, 4, 5])
def test_host_map_equals_the_model_and_its_derivatives_are_derivatives(d):
    rng = np.random.default_rng(d)
    c, x0, y0, L = _random_map(d, rng)
    m = PolyMap(c[0], c[1], (x0, y0), L)
    assert m.degree == d and len(dm.exponents(d)) == distortion.ncoef(d) == c.shape[1] and distortion.exponents(d) == dm.exponents(d)
    x, y = rng.uniform(0, 4095, 500), rng.uniform(0, 4095, 500)
    for got, want in zip(m.eval(x, y) + m.jacobian(x, y), dm.evaluate(c, x0, y0, L, x, y) + dm.jacobian(c, x0, y0, L, x, y)):
        assert np.array_equal(_bits(got), _bits(want))
    h = 1e-3
    num = [(np.array(m.eval(x + h, y)) - np.array(m.eval(x - h, y))) / (2 * h), (np.array(m.eval(x, y + h)) - np.array(m.eval(x, y - h))) / (2 * h)]
    J = m.jacobian(x, y)
    assert max(np.abs(num[0][0] - J[0]).max(), np.abs(num[1][0] - J[1]).max(), np.abs(num[0][1] - J[2]).max(), np.abs(num[1][1] - J[3]).max()) < 1e-8
    H = m.hessian(x, y)
    Jp, Jm = m.jacobian(x + h, y), m.jacobian(x - h, y)
    assert np.abs((Jp[0] - Jm[0]) / (2 * h) - H[0]).max() < 1e-9 and np.abs((Jp[1] - Jm[1]) / (2 * h) - H[1]).max() < 1e-9
    # exact against a sum of exactly representable monomials: coefficients and coordinates that are small dyadic numbers
    e = PolyMap(np.arange(1, c.shape[1] + 1.0), -np.arange(1, c.shape[1] + 1.0), (8.0, 16.0), 4.0)
    xs, ys = np.array([8.0, 12.0, 6.0, 10.0]), np.array([16.0, 12.0, 20.0, 18.0])
    u, v = (xs - 8.0) / 4.0, (ys - 16.0) / 4.0
    want = sum((k + 1.0) * u ** i * v ** j for k, (i, j) in enumerate(dm.exponents(d)))
    X, Y = e.eval(xs, ys)
    assert np.array_equal(X, want) and np.array_equal(Y, -want)


def test_from_affine_compose_and_inverse():
    rng = np.random.default_rng(11)
    A = rm.make_affine(33.0, 0.98, shift=(40.0, -12.0), shear=0.02, centre=(2047.5, 2047.5))
    x, y = rng.uniform(0, 4095, 300), rng.uniform(0, 4095, 300)
    want = rm.apply_affine(A, np.stack([x, y], axis=1))
    for d in (1, 3, 5):
        m = PolyMap.from_affine(A, d, (2000.0, 2100.0), 2900.0)
        X, Y = m.eval(x, y)
        assert np.abs(X - want[:, 0]).max() < 1e-11 and np.abs(Y - want[:, 1]).max() < 1e-11
        assert np.array_equal(_bits(np.stack([m.cx, m.cy])), _bits(dm.from_affine(A, d, 2000.0, 2100.0, 2900.0)))
        assert np.abs(m.affine_part() - A).max() < 1e-12
    with pytest.raises(ValueError):
        PolyMap.from_affine(A, 0)
    with pytest.raises(ValueError):
        PolyMap.from_affine(A, 6)
    for d in (2, 3, 4, 5):
        c, x0, y0, L = _random_map(d, rng)
        m = PolyMap(c[0], c[1], (x0, y0), L)
        X, Y = m.eval(x, y)
        xi, yi = m.inverse(X, Y)
        err = float(np.hypot(xi - x, yi - y).max())
        assert err <= 1e-10, err                                        # inverse(eval(p)) = p
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((xi, yi), dm.inverse(c, x0, y0, L, X, Y)))
        B = np.array([0.5, 0.0, -0.25, 0.0, 0.5, -0.25])                # 2 x 2 binning of the input frame
        Xb, Yb = m.compose_affine(B).eval(x, y)
        wb = rm.apply_affine(B, np.stack([X, Y], axis=1))
        assert np.abs(Xb - wb[:, 0]).max() < 1e-11 and np.abs(Yb - wb[:, 1]).max() < 1e-11
    # a fold: no reference point maps there, Newton must say so
    fold = PolyMap([0.0, 1.0, 0.0, 50.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0, 0.0, 0.0], (0.0, 0.0), 1.0)     # X = u + 50 u^2 >= -1 / 200
    xi, _ = fold.inverse(np.array([-1.0, 0.02]), np.array([0.0, 0.0]))
    assert np.isnan(xi[0]) and abs(fold.eval(xi[1], 0.0)[0] - 0.02) < 1e-12


def test_argument_checks_of_the_map():
    with pytest.raises(ValueError):
        PolyMap([1.0], [1.0])                                            # degree 0
    with pytest.raises(ValueError):
        PolyMap(np.zeros(28), np.zeros(28))                              # degree 6
    with pytest.raises(ValueError):
        PolyMap(np.zeros(6), np.zeros(10))
    with pytest.raises(ValueError):
        PolyMap([0.0, np.nan, 0.0], [0.0, 0.0, 1.0])
    with pytest.raises(ValueError):
        PolyMap([0.0, 1.0, 0.0], [0.0, 0.0, 1.0], scale=0.0)
    a, b = PolyMap.from_affine(rm.IDENTITY, 2), PolyMap.from_affine(rm.IDENTITY, 3)
    with pytest.raises(ValueError):
        distortion.stack_coefficients([a, b])
    with pytest.raises(ValueError):
        distortion.stack_coefficients([a, PolyMap.from_affine(rm.IDENTITY, 2, scale=2.0)])


# -- tile affines ---------------------------------------------------------------------------------------------------------------
def _third_derivative_bound(c, L, umax):
    """An upper bound of every third partial derivative (per pixel^3) of both axes over |u|, |v| <= umax, from the coefficients."""
    d = dm.degree_of(c)
    worst = 0.0
    for a, b in ((3, 0), (2, 1), (1, 2), (0, 3)):
        for axis in (0, 1):
            s = 0.0
            for k, (i, j) in enumerate(dm.exponents(d)):
                if i >= a and j >= b:
                    fall = np.prod([i - q for q in range(a)]) * np.prod([j - q for q in range(b)])
                    s += abs(c[axis, k]) * fall * umax ** (i - a + j - b)
            worst = max(worst, s / L ** 3)
    return worst


def _tile_error_everywhere(c, x0, y0, L, shape, tile_scale=1, scale=1.0):
    """The largest per-axis distance between the model's tile affines and the exact map, over every pixel of every tile."""
    T = dm.tile_affines(c[None], x0, y0, L, shape, tile_scale, scale)[0]
    th, tw = 16 * tile_scale, 64 * tile_scale
    xs = np.arange(shape[1], dtype=np.float64)
    worst = 0.0
    for r0 in range(0, shape[0], 256):
        ys = np.arange(r0, min(r0 + 256, shape[0]), dtype=np.float64)
        X, Y = dm.evaluate(c, x0, y0, L, (xs[None, :] + 0.5) / scale - 0.5, (ys[:, None] + 0.5) / scale - 0.5)
        t = T[(ys.astype(int) // th)[:, None], (xs.astype(int) // tw)[None, :]]
        ax = t[..., 0] * xs[None, :] + t[..., 1] * ys[:, None] + t[..., 2]
        ay = t[..., 3] * xs[None, :] + t[..., 4] * ys[:, None] + t[..., 5]
        worst = max(worst, float(np.abs(ax - X).max()), float(np.abs(ay - Y).max()))
    return worst


@functools.lru_cache(maxsize=None)
def _planted_poly3(size=4096):
    """The planted map as an exact degree-3 polynomial (it is one: a least-squares fit on a noiseless grid leaves 1e-12 px)."""
    f = dm.planted_map(size)
    g = np.linspace(0.0, size - 1.0, 80)
    gx, gy = [a.ravel() for a in np.meshgrid(g, g)]
    x0 = y0 = (size - 1) / 2.0
    L = float(np.hypot(x0, y0))
    c, rank, rms = dm.fit(np.stack([gx, gy], 1), np.stack(f(gx, gy), 1), 3, x0, y0, L)
    assert rank == 10 and rms < 1e-10
    return c, x0, y0, L


@pytest.mark.parametrize('case', ['poly3_4096', 'poly5', 'poly3_oversampled'])
def test_tile_affines_against_the_exact_map_on_every_pixel(case):
    """true error <= tile_error's estimate + the third-order remainder over a tile + what the estimate can miss between the tiles it
    samples, both from a bound T3 on the third derivatives taken from the coefficients: with h = hx + hy the remainder is at most
    T3 h^3 / 6, and between sampled tile centres at most (gx, gy) apart a second derivative moves by at most T3 (gx + gy) / 2."""
    if case == 'poly5':
        c, x0, y0, L = _random_map(5, np.random.default_rng(55), size=1500, px=2.0)
        shape, ts, s = (1000, 1500), 1, 1.0
    else:
        c, x0, y0, L = _planted_poly3()
        shape, ts, s = ((4096, 4096), 1, 1.0) if case == 'poly3_4096' else ((2 * 1100, 2 * 900), 2, 2.0)
    m = PolyMap(c[0], c[1], (x0, y0), L)
    est = m.tile_error(shape, ts, s)
    ref_h, ref_w = shape[0] / s, shape[1] / s
    umax = max(abs(-0.5 - x0), abs(ref_w - 0.5 - x0), abs(-0.5 - y0), abs(ref_h - 0.5 - y0)) / L
    T3 = _third_derivative_bound(c, L, umax)
    hx, hy = 32.0 * ts / s, 8.0 * ts / s
    ty, tx = -(-shape[0] // (16 * ts)), -(-shape[1] // (64 * ts))
    gap_y = 0.0 if ty <= 64 else np.ceil((ty - 1) / 63.0) * 16.0 * ts / s
    gap_x = 0.0 if tx <= 64 else np.ceil((tx - 1) / 63.0) * 64.0 * ts / s
    bound = est + T3 * (hx + hy) ** 3 / 6.0 + 0.5 * (hx + hy) ** 2 * T3 * (gap_x + gap_y) / 2.0
    true = _tile_error_everywhere(c, x0, y0, L, shape, ts, s)
    print('%s: true %.3e px, estimate %.3e, bound %.3e (T3 %.2e)' % (case, true, est, bound, T3))
    assert true <= bound
    assert true >= 0.5 * est                                             # the estimate is no wild overestimate either
    if case == 'poly3_4096':
        assert true < 1e-3 and est < 1e-3


def test_tile_affines_forms():
    """composed=False is the same affine expressed in reference pixels; a map that is an affine gives that affine in every tile."""
    c, x0, y0, L = _planted_poly3()
    for s, ts in ((1.0, 1), (2.0, 1), (1.5, 1), (2.0, 2)):
        shape = (33 * ts, 130 * ts)
        a = dm.tile_affines(c[None], x0, y0, L, shape, ts, s, composed=True)[0]
        r = dm.tile_affines(c[None], x0, y0, L, shape, ts, s, composed=False)[0]
        xc, yc = dm.tile_centres(shape, ts)
        assert a.shape == r.shape == (3, 3, 6)
        xr, yr = (xc + 0.5) / s - 0.5, (yc + 0.5) / s - 0.5
        assert np.abs((a[..., 0] * xc + a[..., 1] * yc + a[..., 2]) - (r[..., 0] * xr + r[..., 1] * yr + r[..., 2])).max() < 1e-9
        assert np.abs(a[..., [0, 1, 3, 4]] * s - r[..., [0, 1, 3, 4]]).max() < 1e-15
    A = rm.make_affine(5.0, 1.01, shift=(3.0, 4.0))
    t = dm.tile_affines(dm.from_affine(A, 3, 100.0, 200.0, 500.0)[None], 100.0, 200.0, 500.0, (100, 300))[0]
    assert np.abs(t - A).max() < 1e-11


# -- the fit --------------------------------------------------------------------------------------------------------------------
def _worst_on_grid(evaluate, planted, size=4096):
    g = np.linspace(0.0, size - 1.0, 65)
    gx, gy = np.meshgrid(g, g)
    X, Y = evaluate(gx, gy)
    TX, TY = planted(gx, gy)
    return float(np.hypot(X - TX, Y - TY).max())


def test_fit_on_the_planted_scene():
    ref, frm, planted = dm.planted_scene()
    noise = SIGMA * np.sqrt(2.0)
    A, rms_affine = rm.fit_transform(ref, frm, 'affine')
    x0, y0, L = dm.bbox_frame(ref)
    m, rank, rms = PolyMap.fit(ref, frm, 3, (x0, y0), L)
    worst = _worst_on_grid(m.eval, planted)
    worst_affine = _worst_on_grid(lambda x, y: tuple(np.moveaxis(rm.apply_affine(A, np.stack([x, y], -1)), -1, 0)), planted)
    print('affine rms %.4f px (worst %.3f); degree 3: rank %d, rms %.4f px (noise %.4f), worst %.4f px' % (rms_affine, worst_affine, rank, rms, noise, worst))
    assert rms_affine > 0.3
    assert rank == 10 and abs(rms - noise) <= 0.1 * noise
    assert worst <= 2.0 * WORST_POLY3 and worst >= 0.5 * WORST_POLY3     # (and the recorded figure is the model's)
    assert abs(worst_affine - WORST_AFFINE) < 0.05 * WORST_AFFINE and worst_affine > 20.0 * worst
    cm, rk, rm_ = dm.fit(ref, frm, 3, x0, y0, L)
    assert rk == rank and rm_ == rms and np.array_equal(_bits(cm), _bits(np.stack([m.cx, m.cy])))
    # rank deficiency is reported, not fitted through: stars on one line, and fewer stars than coefficients
    line = np.stack([np.linspace(0, 4000, 50), np.linspace(0, 4000, 50)], axis=1)
    assert PolyMap.fit(line, line, 2, (x0, y0), L)[0] is None and PolyMap.fit(line, line, 2, (x0, y0), L)[1] < 6
    assert PolyMap.fit(ref[:5], frm[:5], 2, (x0, y0), L)[0] is None


def test_refinement_on_the_planted_scene():
    """Step 7 on the model: from the affine (0.5 px rms, so 3 rms clips at 1.5 px) to degree 3; every star is paired with itself; a
    frame with 20 stars keeps its affine."""
    ref, frm, planted = dm.planted_scene()
    A, rms_affine = rm.fit_transform(ref, frm, 'affine')
    r = dm.refine(ref, frm, A, rms_affine, 3)
    assert r['order'] == 3 and r['margin'] >= 1e-9
    assert np.array_equal(r['pairs'][:, 0], r['pairs'][:, 1]) and len(r['pairs']) >= 590
    assert abs(r['rms'] - SIGMA * np.sqrt(2.0)) <= 0.1 * SIGMA * np.sqrt(2.0)
    assert _worst_on_grid(lambda x, y: dm.evaluate(r['coef'], r['x0'], r['y0'], r['L'], x, y), planted) <= 2.0 * WORST_POLY3
    few = dm.refine(ref, frm[:20], A, rms_affine, 3)
    assert few['order'] == 1 and few['pairs'] is None
    assert np.array_equal(_bits(few['coef']), _bits(dm.from_affine(A, 3, few['x0'], few['y0'], few['L'])))


# -- the transforms file ----------------------------------------------------------------------------------------------------------
def test_yaml_round_trip_through_ap_coadds_lookup(tmp_path):
    yaml = pytest.importorskip('yaml')
    from astrophotography_amd.scripts import ap_coadd
    ref, frm, _ = dm.planted_scene()
    x0, y0, L = dm.bbox_frame(ref)
    m3 = PolyMap.fit(ref, frm, 3, (x0, y0), L)[0]
    A = rm.fit_transform(ref, frm, 'affine')[0]
    maps = [PolyMap.from_affine(rm.IDENTITY, 3, (x0, y0), L), m3, None, PolyMap.from_affine(A, 3, (x0, y0), L)]
    names = ['a.fits', 'b.fits', 'failed.fits', 'c.fits']
    doc = {'transforms': {n: list(map(float, rm.IDENTITY)) for n in names},
           'distortion': distortion.to_document(maps, [1, 3, 1, 1], names)}
    path = tmp_path / 't.yml'
    path.write_text(yaml.safe_dump(doc, sort_keys=False))
    back = yaml.safe_load(path.read_text())
    assert set(back['distortion']['frames']) == {'a.fits', 'b.fits', 'c.fits'}
    assert [len(back['distortion']['frames'][n]['x']) for n in ('a.fits', 'b.fits', 'c.fits')] == [3, 10, 3]
    got = ap_coadd.distortion_maps(back, ['/some/dir/b.fits', 'c.fits', 'a.fits'])
    assert [m.degree for m in got] == [3, 3, 3] and got[0].origin == (x0, y0) and got[0].L == L
    for g, w in zip(got, (maps[1], maps[3], maps[0])):                  # float -> text -> float is exact
        assert np.array_equal(_bits(g.cx), _bits(w.cx)) and np.array_equal(_bits(g.cy), _bits(w.cy))
    assert ap_coadd.distortion_maps(back, ['a.fits'], ignore=True) is None
    assert ap_coadd.distortion_maps({'transforms': {}}, ['a.fits']) is None
    with pytest.raises(RuntimeError):
        ap_coadd.distortion_maps(back, ['failed.fits'])
    back['distortion']['frames']['a.fits']['x'].append(0.0)
    with pytest.raises(RuntimeError):
        ap_coadd.distortion_maps(back, ['a.fits'])
    opts = ap_coadd.command_line_opts(['o.fits', 'a.fits', '--transforms', 't.yml', '--ignore_distortion'])
    assert opts.ignore_distortion and opts.max_tile_error == 0.01
    from astrophotography_amd.scripts import ap_drizzle, ap_register
    assert ap_drizzle.command_line_opts(['o.fits', 'a.fits', '--transforms', 't.yml']).ignore_distortion is False
    assert ap_register.command_line_opts(['-o', 't.yml', 'a.fits', '--model', 'poly3']).model == 'poly3'


def test_an_identity_distortion_gives_the_tiles_of_the_plain_affine():
    """A file whose distortion entry holds order-1 maps describes the affines themselves: every tile's transform is the frame's
    affine, to the rounding of the two forms (1e-11 px over 4096 px)."""
    A = [rm.make_affine(0.7 * f, 1.0 + 1e-3 * f, shift=(2.5 * f, -1.5 * f), centre=(2047.5, 2047.5)) for f in range(3)]
    names = ['f%d.fits' % f for f in range(3)]
    maps = [PolyMap.from_affine(a, 1, (2047.5, 2047.5), 2896.0) for a in A]
    got = distortion.from_document(distortion.to_document(maps, [1, 1, 1], names), names)
    coef, d, x0, y0, L = distortion.stack_coefficients(got)
    assert d == 1
    tiles = dm.tile_affines(coef, x0, y0, L, (4096, 4096))
    xc, yc = dm.tile_centres((4096, 4096))
    for f in range(3):
        assert np.abs(tiles[f][..., [0, 1, 3, 4]] - A[f][[0, 1, 3, 4]]).max() < 1e-15
        assert np.abs(tiles[f][..., [2, 5]] - A[f][[2, 5]]).max() < 1e-11
        assert got[f].tile_error((4096, 4096)) == 0.0
