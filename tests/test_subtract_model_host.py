"""tests/subtract_model.py (F23) against planted truth, on the CPU.

The scene (subtract_model.make_scene): 256 x 256, 64 stars on a jittered grid, the template's PSF a round Gaussian of sigma 1.1; the
image is the noise-free template through a planted, spatially varying kernel, times 0.8, plus a sloped sky, plus noise.

  (a) in span, no noise, float64: the planted kernel is a combination of the basis with coefficients that vary over the field to degree
      2.  The fit takes the spatial terms at a stamp's centre, so the image is planted that way inside the stamps (and pixel by pixel
      elsewhere): the coefficients and a_0 must come back and D must vanish outside the stamps, where the fit has not seen it.
      The bound: the normal equations are sums of N = (2 r + 1)^2 + S n^2 rounded terms, a relative perturbation of at most N 2^-52
      of the scaled system, which the solve multiplies by at most the condition number the model reports:
      |d (theta - truth)| <= cond N 2^-52 |d truth| in the diagonal scaling d of the fit.  A pixel of D is sum_j (truth_j - theta_j)
      D_j with |D_j| <= d_j (d_j^2 is the sum of D_j^2 over the stamps' pixels, sky level included), so |D| <= sqrt(unknowns) times the
      coefficient error: D is held to the error that was reached (itself held to the bound above) plus the roundings of the evaluation.
  (b) noise, out-of-span kernel: chi^2(D) / chi^2(D_true) - 1 over the interior, D_true = I - 0.8 T (x) K_true - B_true with the planted
      kernel on the same noisy pixels.  Measured with this model over the seeds 0 .. 4: see MARGINS; asserted at twice the largest.
  (c) on the same data the kernel degree 2 beats degree 0 in the largest residual at a star.
  (d) a stamp on a variable star (flux ratio 1.5 instead of 0.8) is dropped in the first round, and a_0 moves back.
  (e) convolve='image': D is on the image's flux scale.
  (f) argument errors.
"""
import functools

import numpy as np
import pytest

from tests import subtract_model as sm

SIGMAS, DEGREES, RADIUS, HALF = (0.7, 1.5, 3.0), (4, 3, 2), 8, 12          # 31 functions, stamps of 25 x 25
KDEG, BDEG = 2, 1
SEED = 0
# chi^2(D) / chi^2(D_true) - 1 of the seeds 0 .. 4 (float64 model, measured on the CPU); the assertion is at twice the largest
MARGINS = (0.00156, 0.00250, 0.00245, 0.00205, 0.00257)
CHI2_BOUND = 2.0 * max(MARGINS)
EDGE = 20                                                                   # the interior: RADIUS + the planted kernel's radius, rounded up


@functools.lru_cache(maxsize=None)
def basis():
    return sm.basis(SIGMAS, DEGREES, RADIUS)


@functools.lru_cache(maxsize=None)
def scene(seed=SEED, variable=None):
    return sm.make_scene(seed, variable=variable)


def centers_of(sc, **kw):
    return sm.select_stamps(sc['x'], sc['y'], sc['flux'], sc['image'].shape, HALF, RADIUS, **kw)


@functools.lru_cache(maxsize=None)
def fitted(seed=SEED, kdeg=KDEG, variable=None, convolve='template'):
    sc = scene(seed, variable)
    return sm.optimal_subtract(sc['image'], sc['template'], centers_of(sc), HALF, basis(), kdeg, BDEG, convolve=convolve)


@functools.lru_cache(maxsize=None)
def d_true(seed=SEED):
    sc = scene(seed)
    return sc['image'].astype(np.float64) - sc['scale'] * sm.convolve_field(sc['template'], sc['K']) - sc['bg']


def chi2_margin(seed):
    inner = (slice(EDGE, -EDGE), slice(EDGE, -EDGE))
    D = fitted(seed)['diff'].astype(np.float64)[inner]
    return float((D * D).sum() / (d_true(seed)[inner] ** 2).sum() - 1.0)


def star_residual(sc, D):
    """The largest |D| within 4 pixels of a star of the interior."""
    worst = 0.0
    for x, y in zip(sc['x'], sc['y']):
        cx, cy = int(round(x)), int(round(y))
        if EDGE + 4 <= cx < D.shape[1] - EDGE - 4 and EDGE + 4 <= cy < D.shape[0] - EDGE - 4:
            worst = max(worst, float(np.abs(D[cy - 4:cy + 5, cx - 4:cx + 5]).max()))
    return worst


def test_a_in_span_coefficients_come_back():
    bs = basis()
    sc = scene()
    T = sm.make_scene(SEED, noise_image=0.0, noise_template=0.0)['template'].astype(np.float64)
    H, W = T.shape
    rng = np.random.default_rng(5)
    ntk = (KDEG + 1) * (KDEG + 2) // 2
    akt = np.zeros((bs['nb'], ntk))
    akt[0, 0] = 0.8
    akt[1:] = rng.standard_normal((bs['nb'] - 1, ntk)) * 0.02 / (1.0 + np.arange(1, bs['nb']))[:, None]
    bg = np.array([40.0, 8.0, 15.0])
    _, I = sm.apply(T, np.zeros_like(T), sm.composites(akt, bs, np.float64), KDEG, bg, BDEG, dtype=np.float64)
    cen = centers_of(sc)
    stamp = np.zeros((H, W), bool)
    for cx, cy in cen:                                               # inside a stamp the spatial terms are those of its centre
        X, Y = float(sm.norm_coord(cx, W)), float(sm.norm_coord(cy, H))
        coef = akt @ sm.poly_terms(KDEG, X, Y)
        V = sm.stamp_vectors(T, cx, cy, HALF, bs)
        sl = (slice(cy - HALF, cy + HALF + 1), slice(cx - HALF, cx + HALF + 1))
        I[sl] = np.tensordot(coef, V, 1) + bg @ sm.poly_terms(BDEG, X, Y)
        stamp[sl] = True
    r = sm.optimal_subtract(I, T, cen, HALF, bs, KDEG, BDEG, rounds=0, dtype=np.float64)    # (no rejection: every chi^2 is rounding noise)
    assert r['kept'].all() and r['rounds'] == 1
    truth = np.concatenate([[0.8], akt[1:].ravel(), bg])
    d = r['scale_diag']
    N = (2 * RADIUS + 1) ** 2 + len(cen) * (2 * HALF + 1) ** 2
    rel = r['cond'] * N * 2.0 ** -52
    err = np.linalg.norm(d * (r['theta'] - truth))
    print('cond = %.3g, N = %d, bound = %.3g, |d (theta - truth)| / |d truth| = %.3g, a0 - 0.8 = %.3g' % (
        r['cond'], N, rel, err / np.linalg.norm(d * truth), r['a0'] - 0.8))
    assert rel < 1e-3, 'the bound says something'
    assert err <= rel * np.linalg.norm(d * truth)
    assert abs(r['a0'] - 0.8) <= rel * np.linalg.norm(d * truth) / d[0]
    D = r['diff']
    seen = np.isfinite(D) & ~stamp
    assert seen.sum() > 10000
    # D against the coefficient error that was reached (err, held to its own bound above), not against that bound: with the Cauchy
    # inequality |D| <= |d (theta - truth)| |D_j / d_j| <= err sqrt(unknowns), plus the roundings of the float64 evaluation itself,
    # (taps + terms + 3) 2^-52 times the sum of the magnitudes of the terms, at most max|I| (sum|K| <= 2 here) each
    taps = (2 * RADIUS + 1) ** 2
    d_bound = np.sqrt(len(truth)) * err + (taps + ntk + 3) * 2.0 ** -52 * 2.0 * np.nanmax(np.abs(I)) * ntk
    print('max |D| outside the stamps = %.3g, bound %.3g' % (np.abs(D[seen]).max(), d_bound))
    assert np.abs(D[seen]).max() <= d_bound


@pytest.mark.parametrize('seed', range(5))
def test_b_chi2_against_the_planted_kernel(seed):
    m = chi2_margin(seed)
    print('seed %d: chi2(D) / chi2(D_true) - 1 = %.5f (recorded %.5f), a0 = %.5f' % (seed, m, MARGINS[seed], fitted(seed)['a0']))
    assert max(MARGINS) <= 0.05, 'the scene shows something'
    assert m <= CHI2_BOUND


def test_c_spatial_terms_earn_their_place():
    sc = scene()
    r2, r0 = star_residual(sc, fitted(SEED, 2)['diff']), star_residual(sc, fitted(SEED, 0)['diff'])
    print('largest star residual: degree 2 %.1f, degree 0 %.1f ADU' % (r2, r0))
    assert r2 < r0


def test_d_variable_star_is_rejected():
    sc = scene()
    cen = centers_of(sc)
    v = int(np.argmax(sc['peak']))                                   # the brightest star varies
    at = [k for k, (cx, cy) in enumerate(cen) if abs(cx - sc['x'][v]) <= 1 and abs(cy - sc['y'][v]) <= 1]
    assert len(at) == 1
    scv = scene(SEED, v)
    bs = basis()
    gram, status, count = sm.stamps(scv['template'], scv['image'], cen, HALF, bs)
    all_in = sm.fit(gram, status, count, cen, scv['image'].shape, KDEG, BDEG, rounds=0)
    one = sm.fit(gram, status, count, cen, scv['image'].shape, KDEG, BDEG, rounds=1)
    clean = fitted(SEED)
    print('a0: no rejection %.5f, one round %.5f, without the variable %.5f' % (all_in['a0'], one['a0'], clean['a0']))
    assert all_in['kept'][at[0]] and not one['kept'][at[0]], 'dropped in the first round'
    assert abs(one['a0'] - 0.8) < abs(all_in['a0'] - 0.8)
    D = sm.optimal_subtract(scv['image'], scv['template'], cen, HALF, bs, KDEG, BDEG)['diff']
    cx, cy = cen[at[0]]
    assert D[cy, cx] > 0.5 * (1.5 - 0.8) * sc['peak'][v] * 0.3, 'the variable is in the difference image'


def test_e_convolving_the_image_keeps_its_flux_scale():
    """The image's PSF is the broader one, so this direction deconvolves and the residuals are larger; what is held is the scale: a
    source that brightened by f in the image shows with about f in D, not f a_0."""
    sc = scene()
    r = fitted(SEED, KDEG, None, 'image')
    assert r['a0'] > 1.0, 'the kernel sum is about 1 / 0.8 (the deconvolving kernel is noisy: no tight bound)'
    v = int(np.argmax(sc['peak']))
    scv = scene(SEED, v)
    rv = sm.optimal_subtract(scv['image'], scv['template'], centers_of(sc), HALF, basis(), KDEG, BDEG, convolve='image')
    rt = sm.optimal_subtract(scv['image'], scv['template'], centers_of(sc), HALF, basis(), KDEG, BDEG, convolve='template')
    cx, cy = int(round(sc['x'][v])), int(round(sc['y'][v]))
    fi, ft = rv['diff'][cy - 6:cy + 7, cx - 6:cx + 7].sum(dtype=np.float64), rt['diff'][cy - 6:cy + 7, cx - 6:cx + 7].sum(dtype=np.float64)
    print('flux of the variable in D: image convolved %.1f, template convolved %.1f' % (fi, ft))
    assert ft > 0 and abs(fi / ft - 1.0) < 0.1


def test_f_argument_errors():
    with pytest.raises(ValueError):
        sm.basis((0.7, 1.5), (6,), 10)
    with pytest.raises(ValueError):
        sm.basis((0.7,), (2,), 16)
    with pytest.raises(ValueError):
        sm.basis((0.7,), (2,), 0)
    with pytest.raises(ValueError):
        sm.basis((-1.0,), (2,), 5)
    with pytest.raises(ValueError):
        sm.basis((0.7, 1.5, 3.0), (6, 5, 5), 10)                     # 70 functions
    sc = scene()
    bs = basis()
    cen = centers_of(sc)
    gram, status, count = sm.stamps(sc['template'], sc['image'], cen[:4], HALF, bs)
    with pytest.raises(ValueError):
        sm.fit(gram, status, count, cen[:4], sc['image'].shape, 4, 1)
    with pytest.raises(ArithmeticError):                             # four stamps for the six terms of degree 2
        sm.fit(gram, status, count, cen[:4], sc['image'].shape, 2, 1)
    assert sm.fit(gram, status, count, cen[:4], sc['image'].shape, 1, 1)['kept'].all()
    edge = sm.stamps(sc['template'], sc['image'], [[5, 5]], HALF, bs)
    assert edge[1][0] == sm.ST_OUTSIDE and edge[2][0] == 0 and not edge[0].any()
