"""The empirical PSF (F22) on the host: tests/epsf_model.py against a planted truth, and the host side of ops.epsf_*.

The planted PSF is an elliptical Moffat (beta 2.5, axis ratio 0.8, rotated 30 degrees) plus a faint offset Gaussian lobe, used as the
effective PSF: a star is the function at pixel centres minus the star's position.  60 isolated stars on 256 x 256, o = 2, R = 8,
r_fit = 3, the star list off by up to 0.15 px and 8 % in flux.

Measured with the model on the build host (8 rounds, default clip and smoothing):
    noise-free            max|E - truth| / max truth = 6.155e-3   largest position error 1.166e-2 px
    Gaussian noise 5 ADU  max|E - truth| / max truth = 4.458e-3   largest position error 2.427e-2 px
(the noise-free error is the quartic smoothing's and the cubic interpolant's bias at o = 2; the stamp's outermost nodes carry half
of it: their samples straddle |dx| = R, where the ePSF is defined as 0).  The assertions are twice these values: the margin covers
libm and BLAS differences between hosts; nothing else in the test is non-deterministic.  The best least-squares circular Gaussian
to the same truth is off by 0.120 of the peak.
"""
import functools
import os

import numpy as np
import pytest

from tests import epsf_model as em

O, R, R_FIT, SHAPE, NSTARS = 2, 8, 3.0, (256, 256), 60
MEASURED = {0.0: (6.155e-3, 1.166e-2), 5.0: (4.458e-3, 2.427e-2)}           # noise -> (grid error / peak, position error px)
BOUND = {k: (2.0 * a, 2.0 * b) for k, (a, b) in MEASURED.items()}


@functools.lru_cache(maxsize=None)
def planted(noise):
    """(the field, the model's build of it): computed once, shared by the tests here and in tests/test_gpu_epsf.py; never changed."""
    fld = em.planted_field(SHAPE, NSTARS, O, R, R_FIT, seed=1, noise=noise)
    built = em.build(fld['image'], fld['x0'], fld['y0'], fld['flux0'], fld['sky'], o=O, R=R, r_fit=R_FIT)
    return fld, built


def grid_error(E, truth):
    return float(np.abs(np.asarray(E, np.float64) - truth).max() / truth.max())


def _ops():
    from astrophotography_amd import ops
    return ops


# ---- the taps ---------------------------------------------------------------------------------------------------------------------------
def test_quartic_taps_sum_to_one_and_return_the_centre_of_quartics():
    ops = _ops()
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[-2:3, -2:3].astype(np.float64)
    for kind, deg in (('quartic', 4), ('quadratic', 2)):
        taps = ops.epsf_smoothing_taps(kind)
        assert taps.shape == (5, 5) and abs(taps.sum() - 1.0) <= 1e-13
        assert np.abs(taps - em.smoothing_taps(kind)).max() <= 1e-13               # pinv here, lstsq of unit neighbourhoods there
        worst = 0.0
        for _ in range(20):
            c = {(a, b): rng.uniform(-1, 1) for a in range(deg + 1) for b in range(deg + 1 - a)}
            z = sum(v * xx ** a * yy ** b for (a, b), v in c.items())
            worst = max(worst, abs((taps * z).sum() - c[(0, 0)]))
        print('%s taps: centre of 20 random polynomials off by %.3e at worst' % (kind, worst))
        assert worst <= 1e-13
    none = ops.epsf_smoothing_taps('none')
    assert none[2, 2] == 1.0 and none.sum() == 1.0
    assert np.abs(ops.epsf_smoothing_taps('quartic') - ops.epsf_smoothing_taps('quadratic')).max() > 1e-3
    with pytest.raises(ValueError):
        ops.epsf_smoothing_taps('cubic')


# ---- the interpolant --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('o, R', [(1, 2), (2, 8), (3, 5), (4, 3)])
def test_interpolant_reproduces_nodes_and_its_gradient_matches_differences(o, R):
    rng = np.random.default_rng(o * 10 + R)
    G = em.grid_size(o, R)
    E = rng.normal(size=(G, G)).astype(np.float32)
    off = (np.arange(G) - o * R) / float(o)
    assert np.array_equal(em.evaluate(E, o, off[None, :], off[:, None]), E.astype(np.float64))
    assert np.array_equal(em.shift(E, o, 0.0, 0.0), E.astype(np.float64))
    dx, dy = rng.uniform(-R + 0.01, R - 0.01, 400), rng.uniform(-R + 0.01, R - 0.01, 400)
    _, gx, gy = em.evaluate(E, o, dx, dy, grad=True)
    h = 1e-6 / o                                                         # (a cubic's central difference is off by h^2 f''' / 6)
    nx = (em.evaluate(E, o, dx + h, dy) - em.evaluate(E, o, dx - h, dy)) / (2 * h)
    ny = (em.evaluate(E, o, dx, dy + h) - em.evaluate(E, o, dx, dy - h)) / (2 * h)
    # leave out the points whose difference stencil straddles a node (the second derivative jumps there)
    u, v = dx * o + o * R, dy * o + o * R
    smooth = (np.abs(u - np.rint(u)) > 1e-5) & (np.abs(v - np.rint(v)) > 1e-5)
    assert smooth.sum() > 390
    assert np.abs(gx - nx)[smooth].max() <= 1e-6 * o * 10 and np.abs(gy - ny)[smooth].max() <= 1e-6 * o * 10
    # outside the stamp, and for NaN
    val, gx, gy = em.evaluate(E, o, np.array([R + 1e-9, 0.0, np.nan, -R - 1.0]), np.array([0.0, -R - 1e-9, 0.0, 0.0]), grad=True)
    assert not val.any() and not gx.any() and not gy.any()
    assert em.evaluate(E, o, float(R), float(-R)) == float(E[0, G - 1])              # the corners belong to it


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------
NEW = ('apgpu_epsf_accumulate_f32', 'apgpu_epsf_update_f32', 'apgpu_epsf_shift_f32', 'apgpu_epsf_fit_f32', 'apgpu_epsf_render_f32')


def test_header_and_signatures_agree_for_the_new_names():
    import ctypes as C
    import astrophotography_amd as ap
    from astrophotography_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'apgpu.h')).read()
    for name in NEW:
        res, args = _lib.SIGNATURES[name]
        decl = header[header.index('int ' + name + '('):]
        decl = decl[decl.index('(') + 1:decl.index(';')].rstrip(')')
        params = [p.strip() for p in decl.split(',')]
        assert len(params) == len(args), name
        assert res is C.c_int and params[-1] == 'void *stream' and args[-1] is C.c_void_p
        for p, a in zip(params, args):
            want = {'int64_t': C.c_int64, 'int32_t': C.c_int32, 'double': C.c_double}.get(p.split()[0]) if '*' not in p else None
            if want is None:
                assert '*' in p and a in (C.c_void_p, C.POINTER(C.c_double)), (name, p)
            else:
                assert a is want, (name, p)
    for key, value in (('MAX_OVERSAMPLING', 4), ('MAX_RADIUS', 32), ('REC', 8), ('TILE', 32)):
        assert getattr(_lib, 'EPSF_' + key) == value and '#define APGPU_EPSF_%s %d' % (key, value) in header
    assert em.REC == _lib.EPSF_REC and em.TILE == _lib.EPSF_TILE
    assert 'ApEmpiricalPsf' in ap.__all__ and ap.ApEmpiricalPsf.__name__ == 'ApEmpiricalPsf'
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW)
    # argument checks come before any device work
    assert lib.apgpu_epsf_shift_f32(None, 2, 8, 0.0, 0.0, 1.0, None, None) == _lib.E_INVAL
    assert lib.apgpu_epsf_accumulate_f32(None, 4, 4, None, 0, None, 5, 8, 2.5, 5, None, None, None) == _lib.E_INVAL


def test_host_side_of_ops_refuses_and_agrees_with_the_model():
    ops = _ops()
    for o, R in ((0, 8), (5, 8), (2, 1), (2, 33), (2.5, 8), (True, 8)):
        with pytest.raises(ValueError):
            ops.epsf_grid_size(o, R)
    assert ops.epsf_grid_size(4, 32) == 257 == em.grid_size(4, 32)
    rng = np.random.default_rng(8)
    H, W, Rr = 70, 100, 8
    x, y = rng.uniform(-12, W + 12, 80), rng.uniform(-12, H + 12, 80)
    x[3], y[4] = np.nan, np.inf
    x[5], y[5] = -8.0, 10.0                                              # the stamp touches column 0 exactly
    x[6], y[6] = W - 1 + 8.0, H - 1 + 8.0
    x[7] = -8.000001
    off, idx = ops.epsf_tile_lists(x, y, Rr, (H, W), device='cpu')
    moff, midx = em.tile_lists(x, y, Rr, (H, W))
    assert np.array_equal(off.numpy(), moff) and np.array_equal(idx.numpy(), midx) and off.dtype == idx.dtype
    assert 5 in midx and 6 in midx and 7 not in midx and 3 not in midx and 4 not in midx
    flux = rng.uniform(1, 100, 80)
    flux[10], flux[11] = 0.0, np.nan
    sat = np.zeros(80, bool)
    sat[12] = True
    for max_stars in (3, 500):
        got = ops.epsf_select_stars(x, y, flux, (H, W), 4, 2.0, sat, max_stars)
        assert np.array_equal(got, em.select_stars(x, y, flux, (H, W), 4, 2.0, sat, max_stars))
    assert 3 < len(got) < 80 and np.all(np.diff(flux[got]) <= 0)
    E = rng.uniform(-0.1, 1.0, (17, 17)).astype(np.float32)
    assert ops.epsf_centroid(E, 2, 3.0) == em.centroid(E, 2, 3.0)
    st = ops.epsf_stamp(E, 2)
    assert st.shape == (9, 9) and st.dtype == np.float32 and st.min() >= 0 and np.array_equal(st, em.stamp(E, 2))
    for bad_o in (3, 0):
        with pytest.raises(ValueError):
            ops.epsf_stamp(E, bad_o)


# ---- the planted truth ------------------------------------------------------------------------------------------------------------------
def best_gaussian_error(truth, o):
    """max|g - truth| / max truth of the least-squares circular Gaussian (amplitude and width free, centred) on the grid."""
    G = truth.shape[0]
    off = (np.arange(G) - (G - 1) // 2) / float(o)
    r2 = off[None, :] ** 2 + off[:, None] ** 2
    best = (np.inf, None)
    for s in np.linspace(0.8, 3.0, 2201):
        g = np.exp(-0.5 * r2 / (s * s))
        a = (g * truth).sum() / (g * g).sum()
        sse = ((a * g - truth) ** 2).sum()
        if sse < best[0]:
            best = (sse, a * g)
    return grid_error(best[1], truth)


@pytest.mark.parametrize('noise', [0.0, 5.0])
def test_build_recovers_the_planted_psf(noise):
    """Measured: see the module's docstring (6.155e-3 and 1.166e-2 px noise-free, 4.458e-3 and 2.427e-2 px with noise); asserted at
    twice that.  Independently of any number the ePSF is closer to the truth than the best circular Gaussian."""
    fld, b = planted(noise)
    truth = fld['truth']
    err = grid_error(b['epsf'], truth)
    rec, idx = b['stars'], b['index']
    pos = float(np.hypot(rec[:, 1] - fld['x'][idx], rec[:, 2] - fld['y'][idx]).max())
    flux = float(np.abs(rec[:, 0] / fld['flux'][idx] - 1.0).max())
    print('noise %g: grid error %.4e of the peak, position error %.4e px, flux error %.3e, margin %.3e, rounds %d' % (
        noise, err, pos, flux, b['margin'], b['niter']))
    assert len(idx) == NSTARS and np.all(rec[:, 7] == 1.0)
    assert abs(float(b['epsf'].astype(np.float64).sum()) / O ** 2 - 1.0) <= 1e-6
    assert err <= BOUND[noise][0]
    assert pos <= BOUND[noise][1]
    gauss = best_gaussian_error(truth, O)
    assert err < gauss and gauss > 0.05
    # the start was further off than the result: 0.15 px and 8 %
    assert pos < 0.1 and flux < 0.02


def test_psf_file_stamp_is_what_deconvolve_takes(tmp_path):
    from astrophotography_amd import fitsio
    from astrophotography_amd.core.ApDeconvolve import ApDeconvolve
    from astrophotography_amd.core.ApEmpiricalPsf import ApEmpiricalPsf
    _, b = planted(5.0)
    built = dict(b, stamp=_ops().epsf_stamp(b['epsf'], O))
    path = str(tmp_path / 'psf.fits')
    ApEmpiricalPsf(loglevel='ERROR', oversampling=O, radius=R).write_psf(path, built)
    stamp, hdr = fitsio.read(path)
    assert stamp.shape == (2 * R + 1, 2 * R + 1) and hdr['OVERSAMP'] == O and hdr['RADIUS'] == R and hdr['NSTARS'] == NSTARS
    norm = ApDeconvolve.normalise_stamp(stamp)
    assert norm.dtype == np.float32 and abs(float(norm.astype(np.float64).sum()) - 1.0) < 1e-6
    assert np.array_equal(ApDeconvolve(loglevel='ERROR', psf=path).make_psf(None), norm)
    grid, o, r = ApEmpiricalPsf.read_psf(path)
    assert (o, r) == (O, R) and np.array_equal(grid, b['epsf'])
    assert np.unravel_index(np.argmax(stamp), stamp.shape) == (R, R)


def test_class_refuses_bad_arguments_and_star_lists():
    from astrophotography_amd.core.ApEmpiricalPsf import ApEmpiricalPsf
    for kw in (dict(oversampling=5), dict(radius=1), dict(smoothing='cubic'), dict(fit_radius=0.5), dict(niter=0), dict(readnoise=-1.0)):
        with pytest.raises(ValueError):
            ApEmpiricalPsf(loglevel='ERROR', **kw)
    with pytest.raises(ValueError):
        ApEmpiricalPsf.star_columns({'xcenter': [1.0], 'ycenter': [2.0]})
    x, y, f, sky, sat = ApEmpiricalPsf.star_columns({'xcenter': [1.0, 2.0], 'ycenter': [2.0, 3.0], 'aperture_sum': [5.0, 6.0]})
    assert not sky.any() and not sat.any() and f.tolist() == [5.0, 6.0]


def test_margins_see_a_sample_on_a_node_boundary_and_on_a_clip_bound():
    img = np.zeros((24, 24), np.float32)
    E = np.zeros((em.grid_size(2, 4),) * 2, np.float32)
    m = em.Margin()
    em.samples(img, [[1.0, 10.25, 10.0, 0.0]], E, 2, m)                      # (p - 10.25) 2 + 0.5 is an integer for every p
    assert m.value == 0.0
    m = em.Margin()
    em.samples(img, [[1.0, 10.1, 10.3, 0.0]], E, 2, m)
    assert abs(m.value - 0.1) < 1e-9                                       # (p - 10.3) 2 + 0.5 = integer - 0.1
    m = em.Margin()
    rng = np.random.default_rng(0)
    img = rng.normal(0, 1, (24, 24)).astype(np.float32)
    stars = [[1.0 + 0.1 * k * k, 10.0 + 0.01 * k, 12.0 - 0.013 * k, 0.0] for k in range(9)]      # one pixel per node, nine fluxes
    mean, count, kept, (node, r, who), _ = em.accumulate(img, stars, E, 2, sigma=1.5, margin=m)
    assert 0 < m.value < 1.0 and (~kept).any() and 0 < count.max() < 9
    assert np.array_equal(count.ravel(), np.bincount(node[kept], minlength=count.size))
