"""The sky-gradient removal (F20) on the GPU against tests/gradient_model.py: the sample statistics, the surface lattice,
the apply pass on every tile path, ApRemoveGradient and ap_remove_gradient end to end on the planted scene of
tests/test_gradient_model_host.py, and the three new entry points under the memory guard.

What is held to what:
  sample statistics  median, std, survivors and masked count equal the model (= the oracle) bit for bit: the list instance of the box
                     statistics kernel forms the std of the final survivors in the oracle's order (csrc/box_stats.h, kOrderedStd)
  lattice            the model's bound per node, (n + 8) 2^-53 sum |term| (any order of the sum, a 1-ulp log); the kernel's own order
                     is fixed, so two runs give the same bits, which the guard test asserts
  apply              bit for bit the model, fed the lattice the GPU produced
  end to end         samples, values, sigmas, kept set and the fitted parameters equal the model's bit for bit (the same statistics
                     into the same LAPACK calls); the output within the lattice bound through the interpolant (gain 1.25^2) of the
                     model's output, plus one float32 spacing: two float64 values that close may round to neighbouring float32
"""
import numpy as np
import pytest

from astrophotography_amd._lib import GRADIENT_TILE_H as TH, GRADIENT_TILE_W as TW            # the apply kernel's tile
from tests import gradient_model as gm
from tests import orderstat_cases as oc
from tests.test_gradient_model_host import BLOB_LEVEL, DEGREE, PER_ROW, RADIUS, planted_scene

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings('ignore::RuntimeWarning')]

torch = pytest.importorskip('torch')
F = np.float32


def _ops():
    from astrophotography_amd import ops
    return ops


def _dev(a, shift=0):
    """The array on the device; shift 1: one element past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    if not shift:
        return torch.from_numpy(a).cuda()
    flat = torch.empty(a.size + 4, dtype=torch.from_numpy(a[:0].reshape(-1)).dtype, device='cuda')
    assert flat.data_ptr() % 16 == 0
    t = flat[1:1 + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    v = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(v) == want.view(v)) | (np.isnan(got) & np.isnan(want))


def _check_stats(got, want, what, zsf=None):
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    assert np.array_equal(got[:, 2], want[:, 2]), what + ': survivor counts'
    assert np.array_equal(got[:, 3], want[:, 3]), what + ': masked counts'
    ok = _bits_equal(got[:, 0], want[:, 0])
    if zsf is not None:
        ok |= zsf & (got[:, 0] == 0) & (want[:, 0] == 0)
    assert ok.all(), '%s: medians differ at %s: %s against %s' % (what, np.flatnonzero(~ok)[:5], got[~ok, 0][:5], want[~ok, 0][:5])
    ok = _bits_equal(got[:, 1], want[:, 1])
    assert ok.all(), '%s: std differs at %s: %r against %r' % (what, np.flatnonzero(~ok)[:5], got[~ok, 1][:5], want[~ok, 1][:5])


# ---- sample statistics ----------------------------------------------------------------------------------------------------------------
SH, SW = 70, 131


def _stats_image():
    rng = np.random.default_rng(20)
    img = rng.normal(500.0, 20.0, (SH, SW)).astype(F)
    hot = rng.random(img.shape) < 0.02
    img[hot] += rng.uniform(200, 4000, hot.sum()).astype(F)
    img[3, 4], img[60, 100], img[0, 130], img[35, 66] = np.nan, np.inf, -np.inf, np.nan
    img[40:44, 90:96] = F(512.25)                                                       # ties
    mask = (rng.random(img.shape) < 0.3).astype(np.uint8)
    mask[20:33, 20:33] = 1                                                              # the box of radius <= 6 about (26, 26): fully masked
    return img, mask


CENTRES = [(0, 0), (SW - 1, 0), (0, SH - 1), (SW - 1, SH - 1), (65, 0), (0, 35), (SW - 1, 35), (65, SH - 1), (65, 35), (66, 35), (66, 36), (70, 40),
           (26, 26), (92, 41), (93, 42), (SW + 40, 10), (-33, -33), (SW + 5, SH + 5), (-3, 30), (2 ** 31 - 1, 5), (-2 ** 31, -2 ** 31)]


@pytest.mark.parametrize('r', [0, 1, 12, 32])
def test_sample_stats_equal_the_model(r):
    """Centres in the four corners and on the edges (clipped boxes), outside the image (near, far, at the ends of int32), overlapping
    boxes; no mask, a 30 % mask and a fully masked box; NaN, +inf, -inf and ties in the data; odd and even survivor counts."""
    ops = _ops()
    img, mask = _stats_image()
    d, m = _dev(img), _dev(mask)
    seen = set()
    for mk_h, mk_d in ((None, None), (mask, m)):
        for sigma, maxiters in ((3.0, 5), (2.0, 0)):
            want = gm.sample_stats(img, mk_h, CENTRES, r, sigma, maxiters)
            got = ops.sample_clipped_stats(d, mk_d, CENTRES, r, sigma, maxiters).cpu().numpy()
            _check_stats(got, want, 'r %d mask %s sigma %g maxiters %d' % (r, mk_h is not None, sigma, maxiters))
            seen |= {int(n) % 2 for n in want[:, 2] if n > 0}
            assert want[-1, 2] == 0 and np.isnan(got[-1, 0]) and got[-1, 3] == (2 * r + 1) ** 2
            if mk_h is not None and r <= 6:
                assert got[12, 2] == 0 and np.isnan(got[12, 0]) and np.isnan(got[12, 1])       # the fully masked box
    assert seen == ({1} if r == 0 else {0, 1})
    got = ops.sample_clipped_stats(d, m.to(torch.int32), CENTRES[:3], r).cpu().numpy()          # a mask of another dtype: != 0
    _check_stats(got, gm.sample_stats(img, mask, CENTRES[:3], r), 'int32 mask')


def test_sample_counts_0_1_4096():
    ops = _ops()
    img, mask = _stats_image()
    d, m = _dev(img), _dev(mask)
    got = ops.sample_clipped_stats(d, m, np.zeros((0, 2), np.int32), 5)
    assert tuple(got.shape) == (0, 4) and got.dtype == torch.float64
    assert tuple(ops.sample_clipped_stats(d, None, [], 0).shape) == (0, 4)
    one = ops.sample_clipped_stats(d, m, [(65, 35)], 12).cpu().numpy()
    _check_stats(one, gm.sample_stats(img, mask, [(65, 35)], 12), 'one sample')
    rng = np.random.default_rng(4096)
    c = np.stack([rng.integers(-3, SW + 3, 4096), rng.integers(-3, SH + 3, 4096)], axis=1).astype(np.int32)
    got = ops.sample_clipped_stats(d, m, torch.from_numpy(c).cuda(), 1).cpu().numpy()             # (a device tensor of centres)
    _check_stats(got, gm.sample_stats(img, mask, c, 1), '4096 samples')
    big = np.stack([rng.integers(0, SW, 64), rng.integers(0, SH, 64)], axis=1)
    _check_stats(ops.sample_clipped_stats(d, None, big, 32).cpu().numpy(), gm.sample_stats(img, None, big, 32), '64 samples of radius 32')


@pytest.mark.parametrize('n', [25, 24])
def test_sample_medians_on_the_crafted_key_patterns(n):
    """tests/orderstat_cases.py: every case of n values in a box of its own (radius 2: 25 pixels, the 25th masked for n = 24), so
    that the select meets ties (same_*), neighbours inside the last digit (lower_*, boundary_b0 .. b9) and pairs under different
    prefixes (boundary_b10 .. b31), at an odd and an even count, without clipping (sigma 1e30) and with it."""
    ops = _ops()
    cases = list(oc.cases(np.float32, n))
    assert len(cases) >= 300
    per_row = 32
    rows = -(-len(cases) // per_row)
    img = np.ones((5 * rows, 5 * per_row), F)
    mask = np.zeros(img.shape, np.uint8)
    centres = []
    for i, c in enumerate(cases):
        by, bx = 5 * (i // per_row), 5 * (i % per_row)
        box = np.ones(25, F)
        box[:n] = c.values
        img[by:by + 5, bx:bx + 5] = box.reshape(5, 5)
        mask[by:by + 5, bx:bx + 5] = (np.arange(25) >= n).reshape(5, 5)
        centres.append((bx + 2, by + 2))
    zsf = np.array([c.zero_sign_free for c in cases])
    d, m = _dev(img), _dev(mask)
    for sigma, maxiters in ((1e30, 1), (3.0, 5)):
        want = gm.sample_stats(img, mask, centres, 2, sigma, maxiters)
        got = ops.sample_clipped_stats(d, m, centres, 2, sigma, maxiters).cpu().numpy()
        _check_stats(got, want, 'crafted lines of %d, sigma %g' % (n, sigma), zsf)
        if sigma > 1e20:
            plain = np.array([not c.has_nan and np.isfinite(c.values).all() for c in cases])
            assert np.array_equal(want[plain, 2], np.full(plain.sum(), float(n)))


# ---- the lattice ----------------------------------------------------------------------------------------------------------------------
def _check_lattice(surface, shape, step, what):
    want, bound = gm.lattice(surface, shape, step, want_bound=True)
    got = _ops().surface_lattice(surface, shape, step)
    assert tuple(got.shape) == gm.lattice_shape(shape, step) and got.dtype == torch.float64
    got = got.cpu().numpy()
    err = np.abs(got - want)
    assert np.isfinite(got).all() and np.all(err <= bound), '%s: off by %.3g, %.2f of the bound' % (what, err.max(), float(np.max(err / np.maximum(bound, 1e-300))))
    return got


@pytest.mark.parametrize('K', [1, 3, 4096])
def test_lattice_tps_within_the_bound(K):
    """K + 3 terms in any order, at most 4 roundings a term including a 1-ulp log: (K + 8) 2^-53 (sum |w_k phi_k| + |a0| + |a1 u| +
    |a2 v|) per node.  One centre sits exactly on a node (q = 0: phi = 0, no log of 0)."""
    rng = np.random.default_rng(K)
    for shape, step in (((1, 1), 4), ((1, 1), 64), ((130, 260), 16), ((70, 131), 5)):
        x0, y0, L = gm.frame(shape)
        uv = rng.uniform(-1.0, 1.0, (K, 2))
        uv[0] = (((2 - 1) * step - x0) / L, ((1 - 1) * step - y0) / L)                 # node (iy, ix) = (1, 2)
        surface = dict(model='tps', a=np.array([1000.0, 60.0, -40.0]), w=rng.normal(0.0, 30.0, K), uv=uv, frame=(x0, y0, L))
        got = _check_lattice(surface, shape, step, 'tps K %d image %s step %d' % (K, shape, step))
        assert got.shape == ((4, 4) if shape == (1, 1) else gm.lattice_shape(shape, step))
    assert gm.lattice_shape((130, 260), 16) == (12, 20)
    none = dict(model='tps', a=np.array([5.0, 1.0, 2.0]), w=np.zeros(0), uv=np.zeros((0, 2)), frame=gm.frame((9, 9)))
    _check_lattice(none, (9, 9), 4, 'tps without a centre: the plane')


@pytest.mark.parametrize('degree', [1, 3, 6])
def test_lattice_poly_within_the_bound(degree):
    """(P + 8) 2^-53 sum |c u^i v^j| per node."""
    rng = np.random.default_rng(degree)
    P = (degree + 1) * (degree + 2) // 2
    for shape, step in (((1, 1), 4), ((130, 260), 16), ((70, 131), 64)):
        surface = dict(model='poly', degree=degree, coef=rng.normal(0.0, 50.0, P), frame=gm.frame(shape))
        _check_lattice(surface, shape, step, 'poly degree %d image %s step %d' % (degree, shape, step))


# ---- the apply pass -------------------------------------------------------------------------------------------------------------------
HEIGHTS = (1, TH - 1, TH, TH + 1, 2 * TH + 1)
WIDTHS = (1, TW - 1, TW, TW + 1, 2 * TW + 7, 2 * TW + 4)


def _apply_scene(h, w, step, seed):
    """An image with holes and a lattice (the GPU's own, of a plane that crosses zero, with an infinite and a NaN node planted)."""
    ops = _ops()
    rng = np.random.default_rng(seed)
    img = rng.normal(100.0, 30.0, (h, w)).astype(F)
    for v in (np.nan, np.inf, -np.inf):
        img[rng.integers(0, h), rng.integers(0, w)] = v
    plane = dict(model='poly', degree=2, coef=np.array([40.0, 90.0, -70.0, 15.0, -10.0, 5.0]), frame=gm.frame((h, w)))
    lat = ops.surface_lattice(plane, (h, w), step)
    ny, nx = lat.shape
    lat[int(rng.integers(0, ny)), int(rng.integers(0, nx))] = float('inf')
    lat[int(rng.integers(0, ny)), int(rng.integers(0, nx))] = float('nan')
    return img, lat


@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('step', [4, 16, 64])
def test_apply_equals_the_model_on_every_tile_path(step, shift):
    """Heights and widths about the kernel's tile (TH x TW), W with (W - 1) % step == 0 (129), an image smaller than one step (1 x 1), both
    modes, NaN and +-inf pixels, S <= 0 and S not finite under divide, with and without the surface plane, out aliasing data, the
    planes on a 16-byte boundary (shift 0: 16-byte loads where W % 4 == 0) and one element past it (the scalar path)."""
    ops = _ops()
    paths, seen = set(), set()
    for h in HEIGHTS:
        for w in WIDTHS:
            img, lat = _apply_scene(h, w, step, 1000 * h + w)
            S = gm.interpolate(lat.cpu().numpy(), (h, w), step)
            seen |= {'S <= 0'} if (S <= 0).any() else set()
            seen |= {'S not finite'} if (~np.isfinite(S)).any() else set()
            for mode, ped in (('subtract', 12.5), ('divide', 100.0)):
                want, want_s = gm.apply(img, S, mode, ped)
                d = _dev(img, shift)
                assert d.data_ptr() % 16 == 4 * shift
                got = ops.surface_apply(d, lat, step, mode, ped)
                what = '%d x %d step %d %s shift %d' % (h, w, step, mode, shift)
                assert _bits_equal(got.cpu().numpy(), want).all(), what
                out, surf = ops.surface_apply(d, lat, step, mode, ped, surface_out=True)
                assert _bits_equal(out.cpu().numpy(), want).all() and _bits_equal(surf.cpu().numpy(), want_s).all(), what + ' with the surface'
                assert torch.equal(d.cpu().view(torch.int32), torch.from_numpy(img).view(torch.int32)), what + ': the input was written'
                o2, s2 = _dev(np.zeros((h, w), F), shift), _dev(np.zeros((h, w), F), shift)
                r = ops.surface_apply(d, lat, step, mode, ped, out=o2, surface_out=s2)
                assert r[0] is o2 and r[1] is s2 and _bits_equal(o2.cpu().numpy(), want).all() and _bits_equal(s2.cpu().numpy(), want_s).all(), what
                assert ops.surface_apply(d, lat, step, mode, ped, out=d) is d                    # out aliasing data
                assert _bits_equal(d.cpu().numpy(), want).all(), what + ' in place'
                if mode == 'divide':
                    assert np.isnan(want[(S <= 0) | ~np.isfinite(S)]).all()
                    seen |= {'a finite quotient'} if np.isfinite(want).any() else set()
                paths.add((w % 4 == 0 and shift == 0))
    assert paths == ({True, False} if shift == 0 else {False}) and seen == {'S <= 0', 'S not finite', 'a finite quotient'}
    with pytest.raises(ValueError, match='lattice'):
        ops.surface_apply(_dev(np.zeros((8, 8), F)), torch.zeros((5, 6), dtype=torch.float64, device='cuda'), 4)
    with pytest.raises(ValueError, match='surface_out'):
        x = _dev(np.zeros((8, 8), F))
        ops.surface_apply(x, torch.zeros((5, 5), dtype=torch.float64, device='cuda'), 4, surface_out=x)


def test_the_library_refuses_bad_arguments():
    import ctypes as C
    from astrophotography_amd import _lib
    lib = _lib.load()
    d = torch.zeros(64, dtype=torch.float64, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.apgpu_sample_clipped_stats_f32(p(d), None, 4, 4, p(d), 1, 33, 3.0, 5, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_sample_clipped_stats_f32(p(d), None, 4, 4, p(d), 4097, 3, 3.0, 5, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_sample_clipped_stats_f32(p(d), None, 4, 4, p(d), 1, 3, -1.0, 5, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_sample_clipped_stats_f32(p(d), None, 4, 4, None, 1, 3, 3.0, 5, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_sample_clipped_stats_f32(p(d), None, 4, 4, None, 0, 3, 3.0, 5, None, None) == 0
    assert lib.apgpu_surface_lattice_f64(2, p(d), None, 1, 0.0, 0.0, 1.0, 16, 4, 4, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_surface_lattice_f64(0, p(d), None, 7, 0.0, 0.0, 1.0, 16, 4, 4, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_surface_lattice_f64(0, p(d), None, 1, 0.0, 0.0, 1.0, 3, 4, 4, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_surface_lattice_f64(0, p(d), None, 1, 0.0, 0.0, 0.0, 16, 4, 4, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_surface_lattice_f64(1, p(d), None, 2, 0.0, 0.0, 1.0, 16, 4, 4, p(d), None) == _lib.E_INVAL
    assert lib.apgpu_surface_apply_f32(p(d), p(d), 4, 4, 4, 5, 16, 0, 0.0, p(d), None, None) == _lib.E_INVAL
    assert lib.apgpu_surface_apply_f32(p(d), p(d), 4, 4, 4, 4, 16, 2, 0.0, p(d), None, None) == _lib.E_INVAL
    assert lib.apgpu_surface_apply_f32(p(d), p(d), 4, 4, 4, 4, 65, 0, 0.0, p(d), None, None) == _lib.E_INVAL
    assert lib.apgpu_surface_apply_f32(p(d), p(d), 4, 4, 4, 4, 16, 0, float('nan'), p(d), None, None) == _lib.E_INVAL
    assert lib.apgpu_surface_apply_f32(p(d), p(d), 4, 4, 4, 4, 16, 0, 0.0, p(d), p(d), None) == _lib.E_INVAL
    assert lib.apgpu_version() == 130


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
E2E = dict(samples_per_row=PER_ROW, box_radius=RADIUS, degree=DEGREE)


@pytest.fixture(scope='module')
def scene():
    img, true, disc = planted_scene(blob=BLOB_LEVEL)
    from astrophotography_amd.core.ApRemoveGradient import ApRemoveGradient
    rg = ApRemoveGradient('ERROR')
    d = torch.from_numpy(img).cuda()
    mask = rg.source_mask(d)
    return dict(img=img, true=true, disc=disc, rg=rg, dev=d, mask=mask, mask_host=mask.cpu().numpy())


def _check_against_the_model(r, sc, model_kw, mode='subtract', step=16):
    """r: what ApRemoveGradient.remove returned for the scene."""
    img = sc['img']
    m = gm.remove(img, sc['mask_host'], mode=mode, step=step, **model_kw)
    t = r['samples']
    assert np.array_equal(t[:, :2], m['centres'].astype(np.float64))
    assert _bits_equal(t[:, 2], m['stats'][:, 0]).all(), 'sample values'
    assert np.array_equal(r['kept'], m['kept']) and np.array_equal(t[:, 4] != 0, m['kept']) and r['n_used'] == m['used'].sum()
    assert _bits_equal(t[m['used'], 3], gm.sample_sigmas(np.where(m['used'], m['stats'][:, 1], np.nan), m['stats'][:, 2])[m['used']]).all(), 'sample sigmas'
    assert r['sigma_r'] == m['sigma_r'] and r['pedestal'] == m['pedestal']
    for key in ('coef',) if m['model']['model'] == 'poly' else ('a', 'w', 'uv'):
        assert _bits_equal(np.asarray(r['model'][key], np.float64), np.asarray(m['model'][key], np.float64)).all(), 'fitted ' + key
    # the model's output: the lattice bound through the interpolant, one float32 spacing for the rounding
    lat, bound = gm.lattice(m['model'], img.shape, step, want_bound=True)
    want, want_s = m['image'], m['surface']
    got = r['image'].cpu().numpy()
    scale = 1.0 if mode == 'subtract' else np.nanmax(np.abs(want)) / np.abs(lat).min()
    tol = gm.INTERPOLANT_GAIN * bound.max() * scale + np.spacing(np.abs(want))
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.all(np.abs(got - want)[~np.isnan(want)] <= tol[~np.isnan(want)])
    if r['surface'] is not None:
        s = r['surface'].cpu().numpy()
        assert np.all(np.abs(s - want_s) <= gm.INTERPOLANT_GAIN * bound.max() + np.spacing(np.abs(want_s)))
    return m


@pytest.mark.parametrize('model', ['poly', 'tps'])
def test_remove_on_the_planted_scene(scene, model):
    """The source mask is the product's own (ApMeasureBackground's ops, handed to the model as it is).  The disc's four samples are
    rejected; the surface is recovered to the bound of the host test (poly)."""
    rg = scene['rg']
    kw = dict(E2E, model=model)
    r = rg.remove(scene['dev'], **kw)
    m = _check_against_the_model(r, scene, kw)
    c = m['centres']
    on = scene['disc'][c[:, 1], c[:, 0]]
    assert on.sum() == 4 and not r['kept'][on].any()
    S = r['surface'].cpu().numpy().astype(np.float64)
    rms = float(np.sqrt(np.mean((S - scene['true']) ** 2)))
    sg = r['samples'][:, 3]
    bound = 3.0 * sg[r['kept']].mean() * np.sqrt(10.0 / r['kept'].sum())
    print('%s: rms of the surface against the planted one %.4f (bound for 10 parameters %.4f), %d of %d samples kept' % (model, rms, bound, r['kept'].sum(), len(sg)))
    if model == 'poly':
        assert rms <= bound
    # a caller's mask, divide mode, another step, in place
    kw2 = dict(E2E, model=model, k_high=4.5, k_low=4.5)
    d2 = scene['dev'].clone()
    r2 = rg.remove(d2, mask=scene['mask'], mode='divide', step=64, out=d2, want_surface=False, **kw2)
    assert r2['image'] is d2 and r2['surface'] is None
    _check_against_the_model(r2, scene, kw2, mode='divide', step=64)
    assert not r2['kept'][on].any()


def test_command_line_round_trip(scene, tmp_path):
    from astrophotography_amd import fitsio
    from astrophotography_amd.scripts import ap_remove_gradient as script
    src, out, bg, so, out2 = (str(tmp_path / n) for n in ('in.fits', 'out.fits', 'bg.fits', 'samples.yml', 'out2.fits'))
    hdr = fitsio.Header()
    hdr['OBJECT'] = 'planted'
    fitsio.write(src, scene['img'], hdr)
    flags = ['--samples_per_row', str(PER_ROW), '--box_radius', str(RADIUS), '--degree', str(DEGREE), '--loglevel', 'ERROR']
    assert script.main([src, out, '--background_out', bg, '--samples_out', so] + flags) == 0
    r = scene['rg'].remove(scene['dev'], **E2E)
    got, h = fitsio.read(out)
    assert got.dtype == F and _bits_equal(got, r['image'].cpu().numpy()).all()
    surf, hb = fitsio.read(bg)
    assert _bits_equal(surf.astype(F), r['surface'].cpu().numpy()).all() and hb['IMAGETYP'] == 'Background Sky'
    assert h['OBJECT'] == 'planted' and h['GRADMODE'] == 'SUBTRACT' and h['GRADMODL'] == 'POLY3' and h['GRADNSMP'] == r['n_used']
    assert h['GRADNREJ'] == r['n_used'] - r['kept'].sum() and r['n_used'] >= 340 and h['GRADSMTH'] == 0.0 and h['GRADSTEP'] == 16
    assert abs(h['GRADPED'] - r['pedestal']) <= 1e-9 * r['pedestal'] and abs(h['GRADRMS'] - r['sigma_r']) <= 1e-9 * r['sigma_r']
    assert any('ApRemoveGradient: subtract POLY3' in str(v) for v in h.history())
    # the sample file goes back in through --samples: the same centres, the same image
    import yaml
    doc = yaml.safe_load(open(so))['samples']
    assert len(doc) == 384 and [s['kept'] for s in doc] == r['kept'].tolist() and doc[0]['x'] == 8 and doc[0]['y'] == 8
    assert np.array_equal(np.array([np.nan if s['value'] is None else s['value'] for s in doc]), r['samples'][:, 2], equal_nan=True)
    assert script.main([src, out2, '--samples', so, '--box_radius', str(RADIUS), '--degree', str(DEGREE), '--loglevel', 'ERROR']) == 0
    again, h2 = fitsio.read(out2)
    assert _bits_equal(again, got).all() and h2['GRADNREJ'] == h['GRADNREJ']
    # tps, divide, an excluded rectangle over the disc: its four samples are not even taken
    assert script.main([src, out2, '--model', 'tps', '--smoothing', '0.5', '--mode', 'divide', '--exclude', '170,106,214,150', '--pedestal', '1000',
                        '--step', '32'] + flags) == 0
    _, h3 = fitsio.read(out2)
    assert h3['GRADMODL'] == 'TPS' and h3['GRADMODE'] == 'DIVIDE' and h3['GRADNSMP'] == r['n_used'] - 4 and h3['GRADSMTH'] == 0.5 and h3['GRADPED'] == 1000.0
    assert h3['GRADSTEP'] == 32


# ---- the guard ------------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {'apgpu_sample_clipped_stats_f32', 'apgpu_surface_lattice_f64', 'apgpu_surface_apply_f32'}


def _stats_tol(got, ref, what):
    _check_stats(got, ref, what)


def _guard_case(io, shift):
    """The three new entry points with their inputs inside poisoned slabs, against the model.  The apply pass is compared with the
    model fed the lattice of the same run (as in test_apply_equals_the_model_on_every_tile_path)."""
    ops = _ops()
    h, w, step = 37, 132, 16

    def make():
        rng = np.random.default_rng(99)
        img = rng.normal(300.0, 25.0, (h, w)).astype(F)
        img[4, 7], img[30, 100] = np.nan, np.inf
        mask = (rng.random((h, w)) < 0.2).astype(np.uint8)
        centres = np.array([(0, 0), (w - 1, h - 1), (60, 18), (61, 19), (w + 3, 5), (-9, -9), (131, 0)], np.int32)
        uv = rng.uniform(-1, 1, (40, 2))
        tps = dict(model='tps', a=np.array([300.0, 20.0, -10.0]), w=rng.normal(0, 5.0, 40), uv=uv, frame=gm.frame((h, w)))
        poly = dict(model='poly', degree=3, coef=rng.normal(0, 20.0, 10) + 30.0, frame=gm.frame((h, w)))
        return dict(img=img, mask=mask, centres=centres, tps=tps, poly=poly, stats={r: gm.sample_stats(img, mask, centres, r) for r in (0, 5, 32)},
                    lat={k: gm.lattice(s, (h, w), step, want_bound=True) for k, s in (('tps', tps), ('poly', poly))})
    d = io.once('data', make)
    img, mask = io.dev(d['img'], shift), io.dev(d['mask'], shift)
    for r in (0, 5, 32):
        io.out('sample_stats_r%d' % r, ops.sample_clipped_stats(img, mask, d['centres'], r), d['stats'][r], _stats_tol)
    for kind in ('tps', 'poly'):
        want, bound = d['lat'][kind]
        lat = ops.surface_lattice(d[kind], (h, w), step)

        def within(got, ref, what, bound=bound):
            assert np.all(np.abs(got - ref) <= bound), what
        io.out('lattice_' + kind, lat, want, within)
        S = gm.interpolate(lat.cpu().numpy(), (h, w), step)
        for mode, ped in (('subtract', 7.0), ('divide', 50.0)):
            ref, ref_s = gm.apply(d['img'], S, mode, ped)
            io.out('apply_%s_%s' % (kind, mode), ops.surface_apply(img, lat, step, mode, ped), ref)
            out, surf = io.own((h, w)), io.own((h, w))
            ops.surface_apply(img, lat, step, mode, ped, out=out, surface_out=surf)
            io.out('apply_%s_%s_out' % (kind, mode), out, ref)
            io.out('apply_%s_%s_surface' % (kind, mode), surf, ref_s)
    own = io.own((h, w), init=d['img'])                                          # in place: the caller's plane is the input and the output
    lat = ops.surface_lattice(d['poly'], (h, w), step)
    ops.surface_apply(own, lat, step, 'subtract', 1.0, out=own)
    io.out('apply_in_place', own, gm.apply(d['img'], gm.interpolate(lat.cpu().numpy(), (h, w), step), 'subtract', 1.0)[0])


@pytest.mark.parametrize('shift', [0, 1])
def test_new_entry_points_under_the_guard(shift, monkeypatch):
    """The protocol of tests/test_gpu_guard.py::test_guarded (runs A, B and C: poison 0xFF, poison 0x00, a side stream) for the three
    entry points this feature adds, through that module's runner - which also records them as covered for its own final count.
    The lattice kernel adds its terms in a fixed order, so its result too is compared between the runs bit for bit."""
    import test_gpu_guard as catalogue                                   # the module object pytest collected: its SEEN is the one counted
    fn = lambda io: _guard_case(io, shift)
    memo = {}
    default = torch.cuda.default_stream().cuda_stream
    assert torch.cuda.current_stream().cuda_stream == default
    A, sa = catalogue.run(fn, 4 * 132, 0xFF, memo, monkeypatch)
    assert {n for n, _ in sa} == NEW_ENTRY_POINTS
    assert all(s == default for _, s in sa)
    for label, got, ref, tol in A:
        catalogue.compare(got, ref, tol, '%s against the model' % label)
    B, _ = catalogue.run(fn, 4 * 132, 0x00, memo, monkeypatch)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Cr, sc = catalogue.run(fn, 4 * 132, 0xFF, memo, monkeypatch)
    assert [n for n, _ in sc] == [n for n, _ in sa] and all(s == side.cuda_stream for _, s in sc)
    for tag, other in (('B (poison 0x00)', B), ('C (side stream)', Cr)):
        assert [r[0] for r in other] == [r[0] for r in A]
        for (label, got, _, _), (_, first, _, _) in zip(other, A):
            catalogue.compare(got, first, 'bit', '%s, run %s against run A' % (label, tag))
    assert NEW_ENTRY_POINTS <= catalogue.SEEN
