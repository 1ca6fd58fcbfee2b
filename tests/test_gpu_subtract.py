"""The optimal image subtraction (F23) on the GPU against tests/subtract_model.py: the two kernels of csrc/subtract.hip,
then ops.optimal_subtract, ApSubtract and ap_subtract end to end on the planted scene of tests/test_subtract_model_host.py.  (The new
entry points under the memory guard: tests/test_gpu_diff_guard.py, which must run before tests/test_gpu_guard.py counts.)

What is held to what:
  stamps      status and pixel counts equal the model's.  The fit vectors V_n are made by the same float64 operations in the same
              order as the model's (the 1-D filters are the same bytes: ops.kernel_basis equals the model's basis bit for bit, which is
              asserted), so a Gram sum differs from the model's at most by the order of its n^2 = (2 h + 1)^2 terms: the kernel adds
              them one after the other in row-major order, as the model does, and any order of N terms stays within
              N 2^-52 sum|terms| of any other.  That is the bound asserted per entry, with sum|terms| = sum_p |w V_a| |V_b| from the
              model.  Two calls give the same bytes.
  apply       the difference and the matched image are bit for bit the model's, NaN pattern included; two calls give the same bytes.
  end to end  the stamps kept are the model's (the model's chi^2 margin to the cut is asserted first); a_0, the composite kernels and
              D within the bounds derived at the test.  The bound on D is loose (max|T| times the summed kernel bound: some 17 ADU on
              this scene, above its noise): what carries the test are the kept stamps, a_0 (3e-6) and the kernels (1e-4); the
              differences that the run prints were all 0.
"""
import functools
import os

import numpy as np
import pytest

from tests import subtract_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

MAX_BASIS = ((0.7, 1.5, 3.0), (6, 5, 4))                 # 28 + 21 + 15 = 64 functions on 18 filters
ONE_BASIS = ((1.0,), (0,))


def _ops():
    from astrophotography_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unaligned(a):
    """The array on the device as a contiguous view one element past a 16-byte boundary."""
    flat = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device='cuda')
    v = flat[1:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- stamps ---------------------------------------------------------------------------------------------------------------------------
# (name, shape, S, h, r, basis, weighted)
STAMP_CASES = [('S1-h15-r15-max-basis-weighted', (70, 75), 1, 15, 15, MAX_BASIS, True),
               ('S63-h2-r10-default-basis', (104, 128), 63, 2, 10, (sm.DEFAULT_SIGMAS, sm.DEFAULT_DEGREES), False),
               ('S65-h15-r1-one-function-weighted', (136, 168), 65, 15, 1, ONE_BASIS, True),
               ('S300-h2-r1', (64, 72), 300, 2, 1, ((0.8, 1.6), (2, 1)), False)]


@functools.lru_cache(maxsize=None)
def stamp_scene(name):
    """Template, image, mask and S stamp centres.  From 63 stamps on, the first 16 touch every edge and corner: eight whose footprint
    ends exactly on the image's edge (accepted) and eight one pixel beyond (refused); the next six carry a defect each: a NaN of T, an
    inf of I and a masked pixel in the footprint ring only (h < distance <= h + r), an inf of T on the footprint's corner, a NaN of I
    and a masked pixel inside the stamp.  The rest are random and may overlap anything."""
    _, shape, S, h, r, bas, weighted = next(c for c in STAMP_CASES if c[0] == name)
    rng = np.random.default_rng(len(name) * 1000 + S)
    H, W = shape
    F = h + r
    T = (100.0 + 50.0 * rng.random((H, W)) + 2000.0 * np.exp(-((np.arange(W)[None, :] - W / 2) ** 2 + (np.arange(H)[:, None] - H / 2) ** 2) / 50.0)).astype(np.float32)
    I = (60.0 + 0.7 * T + 5.0 * rng.standard_normal((H, W))).astype(np.float32)
    mask = np.zeros((H, W), np.uint8)
    cen = []
    planted = {}
    if S >= 63:
        for d in (0, 1):                                                                 # 0: fits exactly, 1: one pixel beyond
            cen += [(F - d, H // 2), (W - 1 - F + d, H // 2), (W // 2, F - d), (W // 2, H - 1 - F + d),
                    (F - d, F - d), (W - 1 - F + d, F - d), (F - d, H - 1 - F + d), (W - 1 - F + d, H - 1 - F + d)]
        # six defect stamps, 2 F + 1 apart, so that a defect (within F of its own stamp's centre) lies in no other's footprint, and
        # clear of the footprints of the eight accepted edge stamps
        assert W >= 10 * F + 5 and H >= 8 * F + 4
        slots = [(3 * F + 1 + (k % 3) * (2 * F + 1), 3 * F + 1 + (k // 3) * (2 * F + 1)) for k in range(6)]
        (ax, ay), (bx, by), (cx, cy), (dx, dy), (ex, ey), (fx, fy) = slots
        T[ay + h + 1, ax] = np.nan; planted[16] = sm.ST_TEMPLATE
        I[by - h - 1, bx] = np.inf; planted[17] = None                                   # the image only counts inside the stamp
        mask[cy, cx + h + 1] = 1; planted[18] = None
        T[dy - F, dx - F] = -np.inf; planted[19] = sm.ST_TEMPLATE
        I[ey + h, ex - h] = np.nan; planted[20] = sm.ST_IMAGE
        mask[fy - h, fx + h] = 7; planted[21] = sm.ST_MASK
        cen += slots
    while len(cen) < S:
        cen.append((int(rng.integers(F, W - F)), int(rng.integers(F, H - F))))
    cen = np.array(cen[:S], np.int64)
    bs = sm.basis(bas[0], bas[1], r)
    gain, rn = (1.6, 7.0) if weighted else (0.0, 0.0)
    gram, status, count = sm.stamps(T, I, cen, h, bs, mask=mask, gain=gain, readnoise=rn)
    sabs = sm.stamp_abs_sums(T, I, cen, h, bs, gain, rn)
    return dict(T=T, I=I, mask=mask, centers=cen, h=h, bs=bs, gain=gain, readnoise=rn, gram=gram, status=status, count=count, sabs=sabs,
                planted=planted)


@pytest.mark.parametrize('name', [c[0] for c in STAMP_CASES])
def test_stamps_equal_the_model(name):
    ops = _ops()
    sc = stamp_scene(name)
    bs = ops.kernel_basis(sc['bs']['sigmas'], sc['bs']['degrees'], sc['bs']['radius'])
    for k in ('filters', 'row', 'col', 'even', 'scale', 'B'):
        assert np.array_equal(bs[k], sc['bs'][k]), 'the basis differs from the model in ' + k
    S, n2 = len(sc['centers']), (2 * sc['h'] + 1) ** 2
    if S >= 63:
        st = sc['status']
        assert np.all(st[:8] == 0) and np.all(st[8:16] == sm.ST_OUTSIDE), 'the edge stamps of the scene'
        for k, want in sc['planted'].items():
            assert st[k] == (want or 0), (k, st[k], want)                            # (None: a defect in the ring only is no reason)
        assert (st == 0).sum() >= S // 3
    args = (_dev(sc['T']), _dev(sc['I']), sc['centers'], sc['h'], bs, _dev(sc['mask']), sc['gain'], sc['readnoise'])
    gram, status, count = ops.subtract_stamps(*args)
    gram2, status2, count2 = ops.subtract_stamps(*args)
    assert torch.equal(gram.view(torch.int64), gram2.view(torch.int64)) and torch.equal(status, status2) and torch.equal(count, count2)
    gram, status, count = gram.cpu().numpy(), status.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(status, sc['status']) and np.array_equal(count, sc['count'])
    assert np.all(count[status == 0] == n2) and np.all(gram[status != 0] == 0.0)
    err = np.abs(gram - sc['gram'])
    bound = n2 * 2.0 ** -52 * sc['sabs']
    print('%s: %d stamps accepted, largest error / bound = %.3g, %d of %d entries bit-equal' % (
        name, (status == 0).sum(), np.max(err[status == 0] / np.maximum(bound[status == 0], 1e-300)), (gram == sc['gram']).sum(), gram.size))
    assert np.all(err[status == 0] <= bound[status == 0])
    assert np.array_equal(gram, np.swapaxes(gram, 1, 2)), 'both triangles hold the same sums'


def test_stamps_refusals():
    ops = _ops()
    T = torch.ones((64, 64), device='cuda')
    bs = ops.kernel_basis()
    g, s, c = ops.subtract_stamps(T, T, np.zeros((0, 2)), 5, bs)
    assert g.shape == (0, 51, 51) and s.numel() == 0 and c.numel() == 0
    with pytest.raises(ValueError):
        ops.subtract_stamps(T, T[:32], [[30, 30]], 5, bs)
    with pytest.raises(ValueError):
        ops.subtract_stamps(T, T, [[30, 30]], 16, bs)
    with pytest.raises(ValueError):
        ops.subtract_stamps(T, T, [[30.5, 30]], 5, bs)
    with pytest.raises(ValueError):
        ops.subtract_stamps(T, T, [[30, 30]], 5, bs, gain=1.0, readnoise=0.0)
    with pytest.raises(ValueError):
        ops.subtract_stamps(T, T, [[30, 30]], 5, bs, mask=torch.zeros((3, 3), device='cuda'))
    with pytest.raises(ValueError):
        ops.subtract_stamps(T.cpu(), T, [[30, 30]], 5, bs)
    bad = dict(bs, row=bs['row'].copy())
    bad['row'][3] = bs['filters'].shape[0]
    from astrophotography_amd._lib import ApGpuError
    with pytest.raises(ApGpuError):
        ops.subtract_stamps(T, T, [[30, 30]], 5, bad)


# ---- apply ----------------------------------------------------------------------------------------------------------------------------
# (shape, r, kernel degree, background degree, the image is the one convolved, unaligned view)
APPLY_CASES = [((20, 30), 1, 0, 0, False, False), ((20, 30), 4, 3, 3, True, True), ((100, 130), 10, 2, 1, False, True),
               ((100, 130), 15, 2, 2, True, False), ((64, 128), 15, 3, 3, False, False), ((64, 128), 1, 0, 2, True, False),
               ((33, 67), 10, 1, 0, False, False)]


@functools.lru_cache(maxsize=None)
def apply_scene(shape, r, kdeg, bdeg, conv_image):
    rng = np.random.default_rng(shape[0] * 131 + r * 17 + kdeg * 5 + bdeg)
    H, W = shape
    S = (100.0 + 30.0 * rng.random((H, W))).astype(np.float32)
    O = (90.0 + 30.0 * rng.random((H, W))).astype(np.float32)
    for img in (S, O):                                               # NaN and +-inf, the corners included
        img[rng.integers(H, size=2), rng.integers(W, size=2)] = np.nan
        img[rng.integers(H), rng.integers(W)] = np.inf
        img[rng.integers(H), rng.integers(W)] = -np.inf
    S[0, 0], S[H - 1, W - 1], O[0, W - 1], O[H - 1, 0] = np.nan, np.inf, -np.inf, np.nan
    nt, kw = (kdeg + 1) * (kdeg + 2) // 2, 2 * r + 1
    kernels = (rng.standard_normal((nt, kw, kw)) / (kw * kw)).astype(np.float32)
    kernels[0, r, r] += 0.8
    bg = rng.standard_normal((bdeg + 1) * (bdeg + 2) // 2) * 5.0
    a0 = 0.83
    diff, matched = sm.apply(S, O, kernels, kdeg, bg, bdeg, conv_image, a0)
    return dict(S=S, O=O, kernels=kernels, bg=bg, a0=a0, diff=diff, matched=matched)


@pytest.mark.parametrize('shape, r, kdeg, bdeg, conv_image, unaligned', APPLY_CASES,
                         ids=['%dx%d-r%d-k%d-b%d-%s%s' % (c[0][0], c[0][1], c[1], c[2], c[3], 'image' if c[4] else 'template', '-unaligned' if c[5] else '')
                              for c in APPLY_CASES])
def test_apply_is_the_model_bit_for_bit(shape, r, kdeg, bdeg, conv_image, unaligned):
    ops = _ops()
    sc = apply_scene(shape, r, kdeg, bdeg, conv_image)
    put = _unaligned if unaligned else _dev
    S, O = put(sc['S']), put(sc['O'])
    diff, matched = ops.subtract_apply(S, O, sc['kernels'], kdeg, sc['bg'], bdeg, conv_image, sc['a0'], matched=True)
    diff2 = ops.subtract_apply(S, O, sc['kernels'], kdeg, sc['bg'], bdeg, conv_image, sc['a0'])
    assert torch.equal(diff.view(torch.int32), diff2.view(torch.int32)), 'two calls, with and without the matched image'
    diff, matched = diff.cpu().numpy(), matched.cpu().numpy()
    assert np.array_equal(np.isnan(diff), np.isnan(sc['diff'])) and np.array_equal(np.isnan(matched), np.isnan(sc['matched']))
    fin = np.isfinite(sc['diff'])
    assert fin.sum() >= 50, 'the case has pixels with a value'
    assert np.array_equal(diff.view(np.int32), sc['diff'].view(np.int32)), 'diff: %d pixels differ, largest %g' % (
        (diff.view(np.int32) != sc['diff'].view(np.int32)).sum(), np.nanmax(np.abs(diff - sc['diff'])))
    assert np.array_equal(matched.view(np.int32), sc['matched'].view(np.int32))
    assert np.array_equal(S.cpu().numpy().view(np.int32), sc['S'].view(np.int32)) and np.array_equal(O.cpu().numpy().view(np.int32), sc['O'].view(np.int32))


def test_apply_refusals():
    ops = _ops()
    T = torch.ones((40, 50), device='cuda')
    k = np.zeros((6, 21, 21), np.float32)
    for bad in (dict(kernels=k[:5]), dict(kernels=np.zeros((6, 20, 20), np.float32)), dict(kernels=np.zeros((6, 33, 33), np.float32)),
                dict(kernel_degree=4), dict(bg_degree=-1), dict(bg=[1.0, np.nan, 0.0]), dict(bg=[1.0]), dict(convolved_image=True, a0=0.0),
                dict(other=T[:20])):
        args = dict(convolved=T, other=T, kernels=k, kernel_degree=2, bg=[0.0, 0.0, 0.0], bg_degree=1)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.subtract_apply(**args)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
MARGIN = 1e-6                                            # the model's smallest relative distance of a stamp's chi^2 to the cut


def _host():
    from tests import test_subtract_model_host as host
    return host


def _e2e_bounds(ref, T, n2):
    """The bounds on a_0, the composite kernels and D of a fit whose Gram sums differ from the model's by at most n^2 2^-52 sum|terms|
    (the stamps test): a relative perturbation of the scaled normal equations of at most n^2 2^-52, which the solve multiplies by at
    most the model's condition number: |d (theta - theta_model)| <= rel |d theta_model|, rel = cond n^2 2^-52, in the fit's diagonal
    scaling d.  A coefficient a_{n,t} then moves by at most rel |d theta| / d_{n,t}, a composite kernel by the sum of that times |B_n|
    plus one float32 rounding, and D - evaluated by both sides with the same float32 operations in the same order - by
    max|T| sum_t sum_taps |dA_t| plus the (taps + terms + 3) roundings of 2^-24 sum_t sum_taps |A_t| max|T| that a changed operand can
    turn."""
    host = _host()
    bs = host.basis()
    rel = ref['cond'] * n2 * 2.0 ** -52
    d, theta = ref['scale_diag'], ref['theta']
    norm = rel * np.linalg.norm(d * theta)
    ntk = ref['akt'].shape[1]
    dak = np.zeros_like(ref['akt'])
    dak[0, 0] = norm / d[0]
    dak[1:] = (norm / d[1:1 + (bs['nb'] - 1) * ntk]).reshape(bs['nb'] - 1, ntk)
    dA = np.tensordot(dak.T, np.abs(bs['B']), 1) + 2.0 ** -23 * np.abs(ref['kernels'].astype(np.float64))
    tmax = float(np.nanmax(np.abs(T)))
    taps = ref['kernels'].shape[1] ** 2
    dD = tmax * dA.sum() + (taps + ntk + 3) * 2.0 ** -24 * tmax * np.abs(ref['kernels'].astype(np.float64)).sum() + 3 * norm / d[-3:].min()
    return norm / d[0], dA, dD


def test_optimal_subtract_on_the_planted_scene():
    ops, host = _ops(), _host()
    sc, ref = host.scene(), host.fitted()
    cen = host.centers_of(sc)
    assert ref['margin'] >= MARGIN, 'the model keeps its distance from the cut'
    r = ops.optimal_subtract(_dev(sc['image']), _dev(sc['template']), centers=cen, sigmas=host.SIGMAS, degrees=host.DEGREES, radius=host.RADIUS,
                             kernel_degree=host.KDEG, bg_degree=host.BDEG, half=host.HALF, matched=True)
    assert np.array_equal(r['status'], ref['status']) and np.array_equal(r['kept'], ref['kept']) and r['rounds'] == ref['rounds']
    da0, dA, dD = _e2e_bounds(ref, sc['template'], (2 * host.HALF + 1) ** 2)
    D = r['diff'].cpu().numpy()
    print('a0 = %.9f (model %.9f, bound %.3g); kernels: largest difference %.3g (bound %.3g); D: largest difference %.3g (bound %.3g)' % (
        r['a0'], ref['a0'], da0, np.abs(r['kernels'].astype(np.float64) - ref['kernels']).max(), dA.max(), np.nanmax(np.abs(D - ref['diff'])), dD))
    assert abs(r['a0'] - ref['a0']) <= da0
    assert np.all(np.abs(r['kernels'].astype(np.float64) - ref['kernels'].astype(np.float64)) <= dA)
    assert np.array_equal(np.isnan(D), np.isnan(ref['diff'])) and np.nanmax(np.abs(D - ref['diff'])) <= dD
    assert np.array_equal(np.isnan(r['matched'].cpu().numpy()), np.isnan(ref['matched']))
    inner = (slice(host.EDGE, -host.EDGE), slice(host.EDGE, -host.EDGE))
    m = float((D[inner].astype(np.float64) ** 2).sum() / (host.d_true()[inner] ** 2).sum() - 1.0)
    assert m <= host.CHI2_BOUND, 'against the planted kernel: the host test\'s bound'
    # the image convolved instead: the model's stamps and scale
    refi = host.fitted(host.SEED, host.KDEG, None, 'image')
    ri = ops.optimal_subtract(_dev(sc['image']), _dev(sc['template']), centers=cen, sigmas=host.SIGMAS, degrees=host.DEGREES, radius=host.RADIUS,
                              kernel_degree=host.KDEG, bg_degree=host.BDEG, half=host.HALF, convolve='auto', fwhm=(2.0, 3.0))
    assert ri['convolve'] == 'image' and np.array_equal(ri['kept'], refi['kept'])
    assert abs(ri['a0'] - refi['a0']) <= refi['cond'] * (2 * host.HALF + 1) ** 2 * 2.0 ** -52 * np.linalg.norm(refi['scale_diag'] * refi['theta']) / refi['scale_diag'][0]


def _star_table(sc):
    return dict(xcenter=sc['x'], ycenter=sc['y'], peak_adu=sc['peak'], aperture_sum=sc['flux'])


def test_apsubtract_and_ap_subtract_on_files(tmp_path):
    from astrophotography_amd import fitsio
    from astrophotography_amd.core.ApSubtract import CARDS, ApSubtract
    from astrophotography_amd.scripts import ap_subtract
    host = _host()
    v = int(np.argmax(host.scene()['peak']))
    sc, ref = host.scene(host.SEED, v), host.fitted(host.SEED, host.KDEG, v)
    cen = host.centers_of(sc)
    assert ref['margin'] >= MARGIN
    sub = ApSubtract(loglevel='ERROR', sigmas=host.SIGMAS, degrees=host.DEGREES, radius=host.RADIUS, kernel_degree=host.KDEG,
                     bg_degree=host.BDEG, stamp=host.HALF)
    stars = np.stack([sc['x'], sc['y'], sc['flux'], sc['peak']], 1)
    out = sub.subtract(_dev(sc['image']), _dev(sc['template']), stars=stars)
    rep = out['report']
    assert np.array_equal(rep['fit']['centers'], cen) and np.array_equal(rep['fit']['kept'], ref['kept'])
    assert rep['used'] == ref['kept'].sum() and rep['rejected'] >= 1 and rep['convolve'] == 'template'
    da0, _, dD = _e2e_bounds(ref, sc['template'], (2 * host.HALF + 1) ** 2)
    D = out['image'].cpu().numpy()
    assert abs(rep['scale'] - ref['a0']) <= da0 and np.nanmax(np.abs(D - ref['diff'])) <= dD
    # files
    img, tmpl, src, diff, diff0, mat, ker = (str(tmp_path / n) for n in ('i.fits', 't.fits', 's.fits', 'd.fits', 'd0.fits', 'm.fits', 'k.fits'))
    fitsio.write(img, sc['image'], fitsio.Header())
    fitsio.write(tmpl, sc['template'], fitsio.Header())
    fitsio.write_table(src, [('AP_L1MAG', _star_table(sc), {'xcenter': 'pix', 'ycenter': 'pix'}, None)])
    flags = ['--stars', src, '--radius', str(host.RADIUS), '--sigmas', ','.join(map(str, host.SIGMAS)), '--degrees', ','.join(map(str, host.DEGREES)),
             '--stamp', str(host.HALF), '-l', 'ERROR']
    assert ap_subtract.main([img, tmpl, diff, '--matched_out', mat, '--kernel_out', ker] + flags) == 0
    got, h = fitsio.read(diff)
    assert np.array_equal(got, D, equal_nan=True)
    for card in CARDS:
        assert card in h, card
    assert h['SUBNUSED'] == rep['used'] and abs(h['SUBSCALE'] - rep['scale']) < 1e-12 and h['SUBCONV'] == 'TEMPLATE' and h['SUBTMPL'] == 't.fits'
    cube = fitsio.read(ker)[0]
    assert cube.shape == (9, 2 * host.RADIUS + 1, 2 * host.RADIUS + 1) and np.all(np.abs(cube.sum(axis=(1, 2)) - rep['scale']) < 1e-4)
    assert fitsio.read(mat)[0].shape == got.shape
    # noise at the planted stars, the planted variable kept; the constant kernel visibly worse
    assert ap_subtract.main([img, tmpl, diff0, '--kernel_degree', '0'] + flags) == 0
    got0 = fitsio.read(diff0)[0]
    clean = host.scene()
    keep = np.arange(len(clean['x'])) != v
    others = dict(clean, x=clean['x'][keep], y=clean['y'][keep])
    r2, r0 = host.star_residual(others, got), host.star_residual(others, got0)
    print('largest residual at a constant star: degree 2 %.1f ADU, degree 0 %.1f ADU (noise 5)' % (r2, r0))
    assert r2 < r0 and r2 < 8 * 5.2
    cx, cy = int(round(sc['x'][v])), int(round(sc['y'][v]))
    assert got[cy, cx] > 20 * 5.2, 'the variable star is in the difference image'
    # a mask over one kept stamp refuses it; the noise-model weights run and leave the scale where it was
    msk = str(tmp_path / 'mask.fits')
    k = int(np.flatnonzero(ref['kept'])[0])
    m = np.zeros(sc['image'].shape, np.float32)
    m[cen[k][1], cen[k][0]] = 1.0
    fitsio.write(msk, m, fitsio.Header())
    assert ap_subtract.main([img, tmpl, diff0, '--mask', msk] + flags) == 0
    repm = sub.subtract(_dev(sc['image']), _dev(sc['template']), stars=stars, mask=_dev(m))['report']
    assert repm['refused'] == rep['refused'] + 1 and repm['fit']['status'][k] == sm.ST_MASK and not repm['fit']['kept'][k]
    hm = fitsio.read(diff0)[1]
    assert hm['SUBNUSED'] == repm['used'] and hm['SUBNREJ'] == repm['rejected'] + repm['refused']
    hdr = fitsio.Header()
    hdr['EGAIN'] = 1.5
    fitsio.write(img, sc['image'], hdr)
    assert ap_subtract.main([img, tmpl, diff0, '--gain_keyword', 'EGAIN', '--readnoise', '5'] + flags) == 0
    hg = fitsio.read(diff0)[1]
    print('scale with the noise-model weights %.5f, without %.5f' % (hg['SUBSCALE'], h['SUBSCALE']))
    assert hg['SUBSCALE'] != h['SUBSCALE'] and abs(hg['SUBSCALE'] - 0.8) < 10 * abs(ref['a0'] - 0.8) + 5e-3
    # exit statuses
    assert ap_subtract.main([img, str(tmp_path / 'missing.fits'), diff] + flags) == 1
    assert ap_subtract.main([img, tmpl, diff] + flags + ['--radius', '16']) == 1
    few = {k: a[:3] for k, a in _star_table(sc).items()}
    fitsio.write_table(src, [('AP_L1MAG', few, None, None)])
    os.remove(diff)
    assert ap_subtract.main([img, tmpl, diff] + flags) == 2 and not os.path.exists(diff)


def test_apsubtract_without_a_star_list():
    """stars=None and convolve='auto': the template's own stars (ApFindStars.from_device) and the two measured FWHMs.  The template is
    the sharper image (sigma 1.1 against a kernel that only broadens), so it is the one convolved; the stamps are whole pixels about
    the same stars as with the planted list, so the scale is held to the same distance from the truth as the model's with that list,
    times ten for the other choice of stamps, plus 5e-3."""
    from astrophotography_amd.core.ApSubtract import ApSubtract
    host = _host()
    sc, ref = host.scene(), host.fitted()
    sub = ApSubtract(loglevel='ERROR', sigmas=host.SIGMAS, degrees=host.DEGREES, radius=host.RADIUS, kernel_degree=host.KDEG,
                     bg_degree=host.BDEG, stamp=host.HALF, convolve='auto')
    out = sub.subtract(_dev(sc['image']), _dev(sc['template']))
    rep = out['report']
    print('no list: %d stamps, %d used, scale %.5f (model with the list %.5f), %s convolved' % (rep['stamps'], rep['used'], rep['scale'], ref['a0'], rep['convolve']))
    assert rep['convolve'] == 'template' and rep['used'] >= 16
    assert abs(rep['scale'] - 0.8) < 10 * abs(ref['a0'] - 0.8) + 5e-3
    assert host.star_residual(sc, out['image'].cpu().numpy()) < host.star_residual(sc, host.fitted(host.SEED, 0)['diff'])
