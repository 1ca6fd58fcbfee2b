"""The empirical PSF (F22) on the GPU against tests/epsf_model.py: the five kernels of csrc/epsf.hip, ops.epsf_build,
ApEmpiricalPsf and ap_epsf end to end on the planted field of tests/test_epsf_model_host.py, and the new entry points under the
memory guard.

What is held to what (the model's margins - node assignment, clip bounds, min_count - are asserted >= 1e-9 first, for every seed):
  accumulate  counts equal the model's exactly, so the kept sets are the model's; means within N 2^-52 sum|r| / count (float64 sums
              in another order); two calls give the same bytes
  update      (add + smooth) and shift: within 2 float32 ulp of the model's float64 result (float64 arithmetic, one rounding)
  fit         fit_ok, pixels used and refusals equal the model's; x, y within 1e-6 px and f within 1e-8 relative (ten times the stop
              tolerance: near the minimum the last step bounds the remaining distance and the runs differ in summation order only);
              the second-pass form the same
  render      within 4 2^-24 (|image| + sum|f E|) per pixel; NaN kept; two calls give the same bytes
  end to end  the device's grid within 1e-5 max(E) of the model's: per round the update and the shift differ by at most 2 float32
              ulp each (1.2e-7 relative) and the fitted centres by at most 1e-6 px, which moves a residual by at most
              1e-6 max|dE/dx| <= 5e-7 max(E); eight rounds of (2.4e-7 + 5e-7) max(E) stay below 1e-5 max(E) as long as no clip decision
              flips, which the model's margin of this seed (4e-6 relative, against a perturbation of the residuals below 1e-6
              relative to the bounds) rules out.  Against the truth: the host test's bound.
DESIGN 4.3n records what was measured on an MI355X.
"""
import functools
import os

import numpy as np
import pytest

from astrophotography_amd import fitsio
from tests import epsf_model as em
from tests.test_epsf_model_host import BOUND, NSTARS, O, R, R_FIT, grid_error, planted

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

MARGIN = 1e-9


def _ops():
    from astrophotography_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _grid(o, R, fwhm=2.6, seed=0):
    """A plausible current ePSF: an elongated Gaussian on the grid plus a little structure, float32, sum / o^2 = 1."""
    rng = np.random.default_rng(1000 + seed)
    G = em.grid_size(o, R)
    off = (np.arange(G) - o * R) / float(o)
    s = fwhm / 2.3548
    g = np.exp(-0.5 * ((off[None, :] / s) ** 2 + (off[:, None] / (0.85 * s)) ** 2 + 0.3 * off[None, :] * off[:, None] / (s * s)))
    g = g * (1.0 + 0.02 * rng.normal(size=g.shape))
    return (g / (g.sum() / (o * o))).astype(np.float32)


# the cases: (shape, stars, oversampling, radius, seed).  The seeds were searched on the CPU with the model for margins >= 1e-9.
CASES = [((64, 96), 1, 4, 2, 0), ((64, 96), 3, 4, 8, 0), ((96, 64), 63, 1, 8, 0), ((128, 128), 64, 2, 8, 0), ((100, 130), 65, 3, 2, 0),
         ((256, 256), 200, 2, 8, 0)]
IDS = ['%dx%d-n%d-o%d-R%d' % (c[0][0], c[0][1], c[1], c[2], c[3]) for c in CASES]


@functools.lru_cache(maxsize=None)
def scene(shape, n, o, R, seed):
    """An image of n stars under a planted grid (not the one the kernels are given, so that residuals are not zero) with noise, NaN
    and inf pixels, and its star list.  From 63 stars on: stamps that hang over every edge and corner, one star outside the image,
    one with flux 0, one with a NaN centre, one with a NaN flux.  -> dict(image, stars [n, 4], E: the grid handed to the kernels)."""
    rng = np.random.default_rng(seed * 7919 + n * 31 + o * 7 + R)
    H, W = shape
    truth = _grid(o, R, 2.9, seed + 1).astype(np.float64)
    x, y = rng.uniform(-0.4 * R, W - 1 + 0.4 * R, n), rng.uniform(-0.4 * R, H - 1 + 0.4 * R, n)
    if n <= 3:
        x, y = rng.uniform(R + 1, W - R - 2, n), rng.uniform(R + 1, H - R - 2, n)
    f = 10.0 ** rng.uniform(3.0, 4.5, n)
    sky = rng.uniform(90.0, 110.0, n)
    if n >= 63:
        edge = [(1.3, 2.2), (W - 2.1, 1.7), (1.9, H - 2.4), (W - 1.6, H - 1.2), (W / 2 + 0.3, 0.4), (W / 2 - 0.2, H - 1.3), (0.7, H / 2 + 0.1),
                (W - 0.6, H / 2 - 0.3), (-R - 3.2, 10.0), (W / 3, -0.45 * R)]
        for k, (a, b) in enumerate(edge):
            x[k], y[k] = a + 0.01 * rng.uniform(), b + 0.01 * rng.uniform()
        f[20], x[21], f[22], sky[23] = 0.0, np.nan, np.nan, np.inf
    img = 100.0 + rng.normal(0.0, 4.0, (H, W))
    stars3 = np.stack([f, x, y], axis=1)
    img = img + em.render(None, stars3, truth, o, shape=(H, W))[0]
    img = img.astype(np.float32)
    bad = rng.random((H, W)) < 0.004
    img[bad] = np.nan
    img[rng.integers(H), rng.integers(W)] = np.inf
    # a star list as a finder gives it
    ok = np.isfinite(x) & np.isfinite(y)
    xs, ys = x + np.where(ok, rng.uniform(-0.2, 0.2, n), 0.0), y + np.where(ok, rng.uniform(-0.2, 0.2, n), 0.0)
    stars = np.stack([f * rng.uniform(0.9, 1.1, n), xs, ys, sky], axis=1)
    return dict(image=img, stars=stars, E=_grid(o, R, 2.6, seed), truth=truth.astype(np.float32))


@functools.lru_cache(maxsize=None)
def accumulated(shape, n, o, R, seed, sigma=2.5, maxiters=5):
    sc = scene(shape, n, o, R, seed)
    m = em.Margin()
    return em.accumulate(sc['image'], sc['stars'], sc['E'], o, sigma, maxiters, margin=m) + (m.value,)


# ---- accumulate -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape, n, o, R, seed', CASES, ids=IDS)
def test_accumulate_equals_the_model(shape, n, o, R, seed):
    ops = _ops()
    sc = scene(shape, n, o, R, seed)
    mean, count, kept, (node, r, who), sabs, margin = accumulated(shape, n, o, R, seed)
    assert margin >= MARGIN, margin
    image, E = _dev(sc['image']), _dev(sc['E'])
    got_mean, got_count = ops.epsf_accumulate(image, sc['stars'], E, o)
    gm, gc = got_mean.cpu().numpy(), got_count.cpu().numpy()
    assert gc.dtype == np.int32 and gm.dtype == np.float64 and gm.shape == gc.shape == (em.grid_size(o, R),) * 2
    assert np.array_equal(gc, count)
    tol = n * 2.0 ** -52 * sabs / np.maximum(count, 1)
    assert np.all(np.abs(gm - mean) <= tol), float((np.abs(gm - mean) - tol).max())
    assert np.all(gm[count == 0] == 0.0)
    print('accumulate: margin %.3e, %d of %d nodes without a sample, largest count %d, %d of %d samples clipped, largest |mean - model| %.3e' % (
        margin, int((count == 0).sum()), count.size, int(count.max()), int((~kept).sum()), kept.size, float(np.abs(gm - mean).max())))
    if (n, o) == (3, 4):
        assert (count == 0).sum() > count.size // 2                            # most nodes get no sample: 3 stars fill 3 / 16 of them
    if n >= 63:
        assert (~kept).any() and count.max() > 3                               # the clip removed something
    again = ops.epsf_accumulate(image, sc['stars'], E, o)
    assert torch.equal(again[0].view(torch.int64), got_mean.view(torch.int64)) and torch.equal(again[1], got_count)
    # no clipping at all, and a tight clip
    for sigma, maxiters in ((2.5, 0), (1.5, 2)):
        ref = accumulated(shape, n, o, R, seed, sigma, maxiters)
        assert ref[5] >= MARGIN, ref[5]
        g = ops.epsf_accumulate(image, sc['stars'], E, o, sigma, maxiters)
        assert np.array_equal(g[1].cpu().numpy(), ref[1])
        assert np.all(np.abs(g[0].cpu().numpy() - ref[0]) <= n * 2.0 ** -52 * ref[4] / np.maximum(ref[1], 1))


def test_accumulate_no_stars_and_refusals():
    ops = _ops()
    image, E = torch.zeros((64, 64), dtype=torch.float32, device='cuda'), _dev(_grid(2, 4))
    mean, count = ops.epsf_accumulate(image, np.zeros((0, 4)), E, 2)
    assert not mean.any() and not count.any()
    with pytest.raises(ValueError):
        ops.epsf_accumulate(image, np.zeros((2, 3)), E, 2)                        # [n, 4] wanted
    with pytest.raises(ValueError):
        ops.epsf_accumulate(image, np.zeros((2, 4)), E, 3)                        # 17 nodes are not 2 * 3 * R + 1
    with pytest.raises(ValueError):
        ops.epsf_accumulate(image, np.zeros((2, 4)), E.double(), 2)
    with pytest.raises(ValueError):
        ops.epsf_accumulate(image, np.zeros((2, 4)), E[:, :16], 2)
    with pytest.raises(ValueError):
        ops.epsf_accumulate(image, np.zeros((2, 4)), E, 2, sigma=0.0)
    with pytest.raises(ValueError):
        ops.epsf_accumulate(image, np.zeros((2, 4)), E.cpu(), 2)
    with pytest.raises(TypeError):
        ops.epsf_accumulate(image.double(), np.zeros((2, 4)), E, 2)
    with pytest.raises(ValueError):
        ops.epsf_shift(E, 2, np.nan, 0.0)
    with pytest.raises(ValueError):
        ops.epsf_fit(image, np.zeros((2, 4)), E, 2, 0.5)
    with pytest.raises(ValueError):
        ops.epsf_fit(image, np.zeros((2, 4)), E, 2, 3.0, prev=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        ops.epsf_render(image, np.zeros((2, 3)), E, 2, lists=(torch.zeros(3, dtype=torch.int32, device='cuda'),) * 2)
    with pytest.raises(ValueError):
        ops.epsf_render(None, np.zeros((2, 3)), E, 2)


# ---- update, shift ----------------------------------------------------------------------------------------------------------------------
def _within_ulp(got, ref64, ulps, what):
    tol = ulps * np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    d = np.abs(got.astype(np.float64) - ref64)
    assert np.all(d <= tol), '%s: %g ulp at worst' % (what, float((d / (tol / ulps)).max()))


@pytest.mark.parametrize('o, R', [(1, 2), (2, 8), (3, 5), (4, 8), (4, 32)])
def test_update_and_shift_within_two_ulp(o, R):
    ops = _ops()
    rng = np.random.default_rng(o * 100 + R)
    G = em.grid_size(o, R)
    E = _grid(o, R, 3.0)
    mean = rng.normal(0.0, 1e-3, (G, G))
    count = rng.integers(0, 4, (G, G)).astype(np.int32)
    Ed, md, cd = _dev(E), _dev(mean), _dev(count)
    for kind in ('quartic', 'quadratic', 'none'):
        for min_count in (1, 2):
            taps = ops.epsf_smoothing_taps(kind)
            got, delta = ops.epsf_update(Ed, md, cd, o, taps, min_count, recentre=False, normalise=False)
            assert delta == (0.0, 0.0) and got.dtype == torch.float32
            _within_ulp(got.cpu().numpy(), em.add_smooth(E, mean, count, taps, min_count), 2, 'update %s %d' % (kind, min_count))
    for dx, dy, scale in ((0.0, 0.0, 1.0), (0.013, -0.027, 1.0), (-0.4999, 0.25, 1.7), (1.5, -2.25, 0.3), (R + 1.0, 0.0, 1.0)):
        got = ops.epsf_shift(Ed, o, dx, dy, scale).cpu().numpy()
        _within_ulp(got, em.shift(E, o, dx, dy, scale), 2, 'shift %g %g' % (dx, dy))
    assert np.array_equal(ops.epsf_shift(Ed, o, 0.0, 0.0).cpu().numpy(), E)
    assert not ops.epsf_shift(Ed, o, 2 * R + 1.0, 0.0).any()
    # the whole update: recentred (the centre of mass within r_fit ends at the origin) and normalised
    got, delta = ops.epsf_update(Ed, md, cd, o, 'quartic', 1, r_fit=min(3.0, R))
    ref, rdelta = em.update(E, mean, count, o, em.smoothing_taps('quartic'), 1, min(3.0, R))
    g = got.cpu().numpy()
    assert abs(delta[0] - rdelta[0]) <= 1e-7 and abs(delta[1] - rdelta[1]) <= 1e-7      # (a node off by an ulp moves the centre of mass by 1e-9 px)
    assert abs(float(g.astype(np.float64).sum()) / o ** 2 - 1.0) <= 1e-6
    # three roundings to float32, and a centre of mass 1e-7 px off moves a value by 1e-7 max|dE/dx| < 2^-24 max(E)
    assert np.abs(g.astype(np.float64) - ref.astype(np.float64)).max() <= 8 * 2.0 ** -24 * float(np.abs(ref).max())


# ---- fit --------------------------------------------------------------------------------------------------------------------------------
def _check_fit(got, ref, what):
    assert got.shape == ref.shape == (len(ref), 8)
    assert np.array_equal(got[:, 7], ref[:, 7]), what                              # fit_ok, and so the refusals
    assert np.array_equal(got[:, 5], ref[:, 5]), what                              # pixels used
    ok = ref[:, 7] == 1.0
    bad = ~ok
    assert np.array_equal(got[bad, :4], ref[bad, :4], equal_nan=True) and np.all(np.isnan(got[bad, 4])), what       # the input values
    conv = ok & (ref[:, 6] < 50)                                                  # the stars the model converges: chosen by the model alone
    assert np.all(got[conv, 6] < 50), '%s: %d stars ran into the iteration limit on the device only' % (what, int((got[conv, 6] >= 50).sum()))
    assert np.all(np.abs(got[conv, 1] - ref[conv, 1]) <= 1e-6) and np.all(np.abs(got[conv, 2] - ref[conv, 2]) <= 1e-6), what
    assert np.all(np.abs(got[conv, 0] - ref[conv, 0]) <= 1e-8 * np.abs(ref[conv, 0])), what
    assert np.all(np.abs(got[conv, 3] - ref[conv, 3]) <= 1e-8 * np.maximum(np.abs(ref[conv, 3]), 1.0)), what
    return int(conv.sum()), int(ok.sum())


@pytest.mark.parametrize('shape, n, o, R, seed', CASES, ids=IDS)
def test_fit_equals_the_model(shape, n, o, R, seed):
    ops = _ops()
    sc = scene(shape, n, o, R, seed)
    E = sc['truth']                                                             # the fits have a minimum to find
    image, Ed = _dev(sc['image']), _dev(E)
    r_fit = 2.0 if R == 2 else 3.5
    for fit_sky, gain, rn in ((False, 0.0, 0.0), (True, 0.0, 0.0), (False, 2.0, 3.0)):
        ref = em.fit(sc['image'], sc['stars'], E, o, r_fit, fit_sky, gain, rn)
        got = ops.epsf_fit(image, sc['stars'], Ed, o, r_fit, fit_sky, gain, rn).cpu().numpy()
        conv, ok = _check_fit(got, ref, 'fit_sky %s gain %g' % (fit_sky, gain))
        print('fit, fit_sky %s gain %g: %d of %d stars ok, %d of them converged by the model and compared' % (fit_sky, gain, ok, n, conv))
        if n >= 63:
            assert ok >= n // 2 and conv >= 0.8 * ok and (ref[:, 7] == 0).sum() >= 4     # flux 0, NaN centre, NaN flux, inf sky, outside
        else:
            assert conv == ok == n                                                 # the one or three stars: each is fitted, converged and compared
    if n >= 63:
        first = em.fit(sc['image'], sc['stars'], E, o, r_fit)
        okf = first[:, 7] == 1.0
        prev = np.where(okf[:, None], first[:, :3], 0.0)
        resid = em.render(sc['image'], prev, E, o)[2].astype(np.float32)
        start = np.where(okf[:, None], first[:, :4], sc['stars'])
        ref = em.fit(resid, start, E, o, r_fit, prev=prev)
        got = ops.epsf_fit(_dev(resid), start, Ed, o, r_fit, prev=prev).cpu().numpy()
        conv, ok = _check_fit(got, ref, 'second pass')
        assert conv >= 0.8 * ok and ok >= n // 2
        # with the other stars gone a star's own fit moves little
        both = okf & (ref[:, 7] == 1.0)
        assert np.median(np.hypot(ref[both, 1] - first[both, 1], ref[both, 2] - first[both, 2])) < 0.05


# ---- render -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape, n, o, R, seed', CASES, ids=IDS)
def test_render_equals_the_model(shape, n, o, R, seed):
    ops = _ops()
    sc = scene(shape, n, o, R, seed)
    stars3 = sc['stars'][:, :3].copy()
    if n >= 63:
        H, W = shape
        stars3[30:40, 1] = 40.0 + np.arange(10) * 0.37                         # a crowd: ten stamps over one tile
        stars3[30:40, 2] = 41.0 - np.arange(10) * 0.21
        off, idx = em.tile_lists(stars3[:, 1], stars3[:, 2], R, shape)
        assert np.diff(off).max() >= 8
    E = sc['E']
    model, mabs, resid = em.render(sc['image'], stars3, E, o)
    image, Ed = _dev(sc['image']), _dev(E)
    gm, gr = ops.epsf_render(image, stars3, Ed, o)
    gm, gr = gm.cpu().numpy(), gr.cpu().numpy()
    assert gm.dtype == gr.dtype == np.float32 and np.isfinite(gm).all()
    assert np.all(np.abs(gm.astype(np.float64) - model) <= 4 * 2.0 ** -24 * mabs)
    nan = np.isnan(sc['image'])
    assert nan.any() and np.array_equal(np.isnan(gr), nan)
    fin = np.isfinite(sc['image'])
    tol = 4 * 2.0 ** -24 * (np.abs(sc['image'].astype(np.float64)) + mabs)
    assert np.all(np.abs(gr[fin].astype(np.float64) - resid[fin]) <= tol[fin])
    assert np.array_equal(gr[~fin & ~nan], sc['image'][~fin & ~nan])               # inf stays inf
    lists = ops.epsf_tile_lists(stars3[:, 1], stars3[:, 2], R, shape)
    again = ops.epsf_render(image, _dev(stars3), Ed, o, lists=lists)
    assert np.array_equal(again[0].cpu().numpy(), gm) and np.array_equal(again[1].cpu().numpy().view(np.uint32), gr.view(np.uint32))
    only_m = ops.epsf_render(None, stars3, Ed, o, shape=shape, residual=False)
    assert only_m[1] is None and np.array_equal(only_m[0].cpu().numpy(), gm)
    only_r = ops.epsf_render(image, stars3, Ed, o, model=False)
    assert only_r[0] is None and np.array_equal(only_r[1].cpu().numpy().view(np.uint32), gr.view(np.uint32))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _star_list(fld):
    return dict(xcenter=fld['x0'], ycenter=fld['y0'], aperture_sum=fld['flux0'], bgmed_per_pix=np.full(len(fld['x0']), fld['sky']),
                psbl_sat=np.zeros(len(fld['x0']), bool))


def _robust_scatter(v):
    v = v[np.isfinite(v)]
    return 1.4826 * float(np.median(np.abs(v - np.median(v))))


def test_build_and_photometry_on_the_planted_field():
    from astrophotography_amd.core.ApEmpiricalPsf import ApEmpiricalPsf
    fld, ref = planted(5.0)
    assert ref['margin'] >= MARGIN
    ep = ApEmpiricalPsf(loglevel='ERROR', oversampling=O, radius=R, fit_radius=R_FIT)
    image = _dev(fld['image'])
    built = ep.build(image, _star_list(fld))
    E = built['epsf'].cpu().numpy()
    peak = float(ref['epsf'].max())
    diff = float(np.abs(E.astype(np.float64) - ref['epsf'].astype(np.float64)).max())
    err = grid_error(E, fld['truth'])
    print('device against model: %.3e of the peak; against the truth: %.4e of the peak (model %.4e)' % (diff / peak, err, grid_error(ref['epsf'], fld['truth'])))
    assert built['niter'] == ref['niter'] and np.array_equal(built['index'], ref['index']) and np.array_equal(built['count'], ref['count'])
    assert diff <= 1e-5 * peak
    assert err <= BOUND[5.0][0]
    rec, idx = built['stars'], built['index']
    assert np.all(rec[:, 7] == 1.0) and np.hypot(rec[:, 1] - fld['x'][idx], rec[:, 2] - fld['y'][idx]).max() <= BOUND[5.0][1]
    assert np.abs(rec[:, 1] - ref['stars'][:, 1]).max() <= 1e-5 and np.abs(rec[:, 2] - ref['stars'][:, 2]).max() <= 1e-5
    assert built['stamp'].shape == (2 * R + 1,) * 2 and abs(float(built['stamp'].astype(np.float64).sum()) - 1.0) < 1e-6

    p1 = ep.photometry(image, _star_list(fld), passes=1)
    p2 = ep.photometry(image, _star_list(fld), passes=2, epsf=built['epsf'])
    for p in (p1, p2):
        c = p['columns']
        assert c['fit_ok'].all() and len(c['fit_ok']) == NSTARS
        assert np.hypot(c['x_fit'] - fld['x'], c['y_fit'] - fld['y']).max() <= BOUND[5.0][1]
        assert np.abs(c['flux_fit'] / fld['flux'] - 1.0).max() < 0.03
    # isolated stars: the second pass finds what the first found, where its disc of pixels (about the rounded start) is the same one
    c1, c2 = p1['columns'], p2['columns']
    moved = np.hypot(c2['x_fit'] - c1['x_fit'], c2['y_fit'] - c1['y_fit'])
    same = (np.rint(fld['x0']) == np.rint(c1['x_fit'])) & (np.rint(fld['y0']) == np.rint(c1['y_fit']))
    assert same.sum() > NSTARS // 2 and moved[same].max() < 1e-4 and moved.max() <= BOUND[5.0][1]
    resid, model = ep.subtract(image, p2['records'], model=True)
    resid, model = resid.cpu().numpy(), model.cpu().numpy()
    inside = model > 1e-3 * model.max()
    assert 0.02 < inside.mean() < 0.9
    assert _robust_scatter(resid[inside]) < _robust_scatter(fld['image'][inside])
    assert _robust_scatter(resid[inside]) < 1.5 * 5.0                              # about the noise that was put in
    with pytest.raises(ValueError):
        ep.photometry(image, _star_list(fld), passes=3)
    with pytest.raises(ValueError):
        ApEmpiricalPsf(loglevel='ERROR').photometry(image, _star_list(fld))         # no ePSF yet


def test_ap_epsf_writes_files_that_deconvolve_reads(tmp_path):
    from astrophotography_amd.core.ApDeconvolve import ApDeconvolve
    from astrophotography_amd.core.ApEmpiricalPsf import ApEmpiricalPsf
    from astrophotography_amd.scripts import ap_epsf
    fld, ref = planted(5.0)
    img, src, psf, phot, res, mod = (str(tmp_path / n) for n in ('image.fits', 'stars.fits', 'psf.fits', 'phot.fits', 'res.fits', 'model.fits'))
    hdr = fitsio.Header()
    hdr['EGAIN'] = 1.5
    fitsio.write(img, fld['image'], hdr)
    fitsio.write_table(src, [('AP_L1MAG', _star_list(fld), {'xcenter': 'pix', 'ycenter': 'pix'}, None)], header={'AP_FWHM': (R_FIT, '[pix]')})
    flags = ['--oversampling', str(O), '--radius', str(R), '-l', 'ERROR']
    assert ap_epsf.main([img, src, psf, '--photometry', phot, '--residual', res, '--model', mod, '--passes', '2'] + flags) == 0
    stamp, h = fitsio.read(psf)
    assert stamp.shape == (2 * R + 1,) * 2 and h['OVERSAMP'] == O and h['RADIUS'] == R and h['NSTARS'] == NSTARS and h['NITER'] == ref['niter']
    taken = ApDeconvolve(loglevel='ERROR', psf=psf).make_psf(None)
    assert np.array_equal(taken, ApDeconvolve.normalise_stamp(stamp)) and taken.shape == stamp.shape
    grid, o, r = ApEmpiricalPsf.read_psf(psf)
    assert (o, r) == (O, R) and grid_error(grid, fld['truth']) <= BOUND[5.0][0]       # the fit radius came from the list's AP_FWHM
    cols, _, prim = fitsio.read_table(phot, 'AP_L1MAG')
    for name in ('xcenter', 'ycenter', 'aperture_sum', 'bgmed_per_pix', 'psbl_sat', 'flux_fit', 'x_fit', 'y_fit', 'sky_fit', 'chi2', 'fit_ok'):
        assert name in cols and len(cols[name]) == NSTARS
    assert cols['fit_ok'].all() and np.array_equal(cols['xcenter'], fld['x0']) and prim['AP_FWHM'] == R_FIT
    assert np.hypot(cols['x_fit'] - fld['x'], cols['y_fit'] - fld['y']).max() <= BOUND[5.0][1]
    resid, model = fitsio.read(res)[0], fitsio.read(mod)[0]
    np.testing.assert_allclose(resid + model, fld['image'], rtol=0, atol=8 * 2.0 ** -24 * float(fld['image'].max()))
    inside = model > 1e-3 * model.max()
    assert _robust_scatter(resid[inside]) < _robust_scatter(fld['image'][inside])
    # the single steps from the PSF file that exists now: the same table and planes
    ep = ApEmpiricalPsf(loglevel='ERROR')
    phot2, res2, mod2 = (str(tmp_path / n) for n in ('phot2.fits', 'res2.fits', 'model2.fits'))
    ep.photometry_files(img, src, psf, phot2, passes=2)
    assert (ep.oversampling, ep.radius) == (O, R)
    cols2 = fitsio.read_table(phot2, 'AP_L1MAG')[0]
    assert all(np.array_equal(cols2[k], cols[k], equal_nan=True) for k in cols)
    ep.subtract_files(img, src, psf, residual_file=res2, model_file=mod2, passes=2)
    assert np.array_equal(fitsio.read(res2)[0], resid) and np.array_equal(fitsio.read(mod2)[0], model)
    # gain-weighted fits run as well; bad input and too few stars have their own exit status
    assert ap_epsf.main([img, src, psf, '--gain_keyword', 'EGAIN', '--readnoise', '5', '--fit_sky'] + flags) == 0
    assert ap_epsf.main([img, str(tmp_path / 'missing.fits'), psf] + flags) == 1
    assert ap_epsf.main([img, img, psf] + flags) == 1                                # no AP_L1MAG table in it
    assert ap_epsf.main([img, src, psf, '--oversampling', '7', '-l', 'ERROR']) == 1
    few = {k: v[:2] for k, v in _star_list(fld).items()}
    fitsio.write_table(src, [('AP_L1MAG', few, None, None)])
    os.remove(psf)
    assert ap_epsf.main([img, src, psf] + flags) == 2 and not os.path.exists(psf)


# ---- the guard --------------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {'apgpu_epsf_accumulate_f32', 'apgpu_epsf_update_f32', 'apgpu_epsf_shift_f32', 'apgpu_epsf_fit_f32', 'apgpu_epsf_render_f32'}


def _guard_case(io, shift):
    """The five new entry points with their inputs inside poisoned slabs, against the model."""
    ops = _ops()
    shape, n, o, R, seed = CASES[3]
    r_fit = 3.5

    def make():
        sc = scene(shape, n, o, R, seed)
        acc = accumulated(shape, n, o, R, seed)
        assert acc[5] >= MARGIN
        taps = em.smoothing_taps('quartic')
        first = em.fit(sc['image'], sc['stars'], sc['truth'], o, r_fit)
        prev = np.where(first[:, 7:8] == 1.0, first[:, :3], 0.0)
        model, mabs, resid = em.render(sc['image'], prev, sc['truth'], o)
        return dict(sc=sc, mean=acc[0], count=acc[1], sabs=acc[4], smooth=em.add_smooth(sc['E'], acc[0], acc[1], taps), taps=taps,
                    shifted=em.shift(sc['E'], o, 0.21, -0.13, 1.1), first=first, prev=prev, model=model, mabs=mabs, resid=resid,
                    second=em.fit(resid.astype(np.float32), first[:, :4], sc['truth'], o, r_fit, prev=prev),
                    lists=em.tile_lists(prev[:, 1], prev[:, 2], R, shape))
    d = io.once('data', make)
    sc = d['sc']
    image, E, T = io.dev(sc['image'], shift), io.dev(sc['E'], shift), io.dev(sc['truth'], shift)
    mean, count = ops.epsf_accumulate(image, io.dev(sc['stars'], shift), E, o)

    def near_mean(got, ref, what):
        assert np.all(np.abs(got - ref) <= n * 2.0 ** -52 * d['sabs'] / np.maximum(d['count'], 1)), what
    io.out('mean', mean, d['mean'], near_mean)
    io.out('count', count, d['count'])
    upd, _ = ops.epsf_update(E, io.dev(d['mean'], shift), io.dev(d['count'], shift), o, d['taps'], recentre=False, normalise=False)
    io.out('update', upd, d['smooth'], lambda got, ref, what: _within_ulp(got, ref, 2, what))
    io.out('shift', ops.epsf_shift(E, o, 0.21, -0.13, 1.1), d['shifted'], lambda got, ref, what: _within_ulp(got, ref, 2, what))
    io.out('fit', ops.epsf_fit(image, io.dev(sc['stars'], shift), T, o, r_fit), d['first'], lambda got, ref, what: _check_fit(got, ref, what))
    stars3 = io.dev(d['prev'], shift)
    lists = (io.dev(d['lists'][0], shift), io.dev(d['lists'][1], shift))
    model, resid = ops.epsf_render(image, stars3, T, o, lists=lists)
    io.out('model', model, d['model'], lambda got, ref, what: np.testing.assert_array_less(np.abs(got - ref), 4 * 2.0 ** -24 * d['mabs'] + 1e-30, what))
    io.out('residual', resid)
    rec2 = ops.epsf_fit(io.dev(d['resid'].astype(np.float32), shift), io.dev(d['first'][:, :4], shift), T, o, r_fit, prev=stars3)
    io.out('second', rec2, d['second'], lambda got, ref, what: _check_fit(got, ref, what))


@pytest.mark.parametrize('shift', [0, 1])
def test_new_entry_points_under_the_guard(shift, monkeypatch):
    """The protocol of tests/test_gpu_guard.py::test_guarded (runs A, B and C: poison 0xFF, poison 0x00, a side stream) for the five
    entry points this feature adds, through that module's runner - which also records them as covered for its own final count.  All
    five kernels are deterministic, so every result is compared between the runs bit for bit."""
    import test_gpu_guard as catalogue                                   # the module object pytest collected: its SEEN is the one counted
    fn = lambda io: _guard_case(io, shift)
    memo = {}
    default = torch.cuda.default_stream().cuda_stream
    assert torch.cuda.current_stream().cuda_stream == default
    A, sa = catalogue.run(fn, 0, 0xFF, memo, monkeypatch)
    assert {n for n, _ in sa} == NEW_ENTRY_POINTS
    assert all(s == default for _, s in sa)
    for label, got, ref, tol in A:
        if ref is not None:
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
    assert NEW_ENTRY_POINTS <= catalogue.SEEN
