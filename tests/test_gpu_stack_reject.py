"""The rejection rules of small stacks on the GPU (csrc/stack_reject.hip) against their NumPy restatement
(tests/stack_reject_model.py): count, mean_f64 and std_f64 bit for bit, mean and std their float32 roundings - on every slot
count's edge, ragged pixel counts, both dtypes, the fused calibration, a pixel mask, row stripes, non-finite values, ties and
the crafted lines of tests/orderstat_cases.py; under the guard bands of tests/guard.py; and end to end on a stack with a trail."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import orderstat_cases as oc
from tests import stack_reject_model as model
from tests.guard import guarded, place, unchanged
from tests.util import assert_biteq, synth_cube, synth_masters

pytestmark = pytest.mark.gpu
F = np.float32
OUTPUTS = ('mean', 'std', 'count', 'mean_f64', 'std_f64')
RULES = (('winsorized', dict(sigma_lower=2.5, sigma_upper=3.0)), ('minmax', dict(nlow=1, nhigh=2)))


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _model(values, method, kw, pixmask=None):
    if method == 'winsorized':
        return model.winsorized(values, kw.get('sigma_lower', 3.0), kw.get('sigma_upper', 3.0), kw.get('maxiters'), pixmask=pixmask)
    return model.minmax(values, kw.get('nlow', 1), kw.get('nhigh', 1), pixmask=pixmask)


def _compare(got, ref, what):
    with np.errstate(over='ignore'):
        want = dict(count=ref['count'], mean_f64=ref['mean_f64'], std_f64=ref['std_f64'], mean=ref['mean_f64'].astype(F),
                    std=ref['std_f64'].astype(F))
    for k in OUTPUTS:
        g = got[k].cpu().numpy()
        assert_biteq(g, want[k].reshape(g.shape), '%s: %s' % (what, k))
        if k in ('mean', 'std'):                             # the NaN of a pixel without data: quiet, positive, no payload
            assert (g.view(np.uint32)[np.isnan(g)] == 0x7fc00000).all(), what


def _check(raw, method, kw, what, values=None, calib=None, pixmask=None):
    """raw: what the library is given (host array or device tensor); values: the float32 values of its columns (default: raw)."""
    from astrophotography_amd import ops
    values = np.asarray(raw, F) if values is None else values
    ref = _model(values.reshape(values.shape[0], -1), method, kw, None if pixmask is None else pixmask.reshape(-1))
    t = raw if torch.is_tensor(raw) else _dev(raw)
    got = ops.stack_reject(t, method, calib=calib, pixmask=None if pixmask is None else _dev(pixmask), outputs=OUTPUTS, **kw)
    _compare(got, ref, what)
    return ref


def _slot_counts():
    from astrophotography_amd import ops
    return sorted({int(ops.stack_kernel_name(n, calibrated=False, rejection='minmax').split('<')[1].split(',')[0]) for n in range(1, 129)})


def _calibrated(rng, raw, still_biased=True):
    """Masters for raw[N, P] and the float32 values the fused calibration forms (the oracle's ApCalibrate arithmetic)."""
    from oracle import apref
    N, P = raw.shape
    bias, dark, flat = synth_masters(rng, (P,))
    flat[0] = 0.0                                            # a zero in the flat: no division there
    if P > 1:
        flat[1] = np.nan                                     # a NaN: the whole column is not finite
    nflat, _ = apref.flat_normalize(flat)
    e = rng.uniform(0.3, 0.5, N).astype(F)
    ped = np.where(rng.random(N) < 0.3, -50.0, 0.0).astype(F)
    cal = apref.calibrate(raw.reshape(N, 1, P), bias, dark, nflat, [float(v) for v in e], [float(v) for v in ped], still_biased)
    calib = dict(bias=_dev(bias), dark=_dev(dark), nflat=_dev(nflat), exp_ratio=e, pedestal=ped, dark_still_biased=still_biased)
    return calib, np.asarray(cal, F).reshape(N, P)


@pytest.mark.parametrize('dtype', [F, np.uint16], ids=['f32', 'u16'])
@pytest.mark.parametrize('method, kw', RULES, ids=[r[0] for r in RULES])
def test_every_slot_count_at_its_edges(method, kw, dtype):
    slots = _slot_counts()
    assert slots[-1] == 128
    frames = sorted({1, 2, 3} | {n for s in slots for n in (s - 1, s, s + 1) if 1 <= n <= 128})
    rng = np.random.default_rng(1)
    P = 257
    for n in frames:
        raw = synth_cube(rng, n, (P,), nan_frac=0.02 if dtype == F else 0.0, dtype=dtype)
        _check(raw, method, kw, '%s %d frames' % (method, n))


@pytest.mark.parametrize('P', [1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize('method, kw', RULES, ids=[r[0] for r in RULES])
def test_pixel_counts_calibration_and_mask(method, kw, P):
    rng = np.random.default_rng(100 + P)
    n = 12
    for dtype in (F, np.uint16):
        raw = synth_cube(rng, n, (P,), dtype=dtype)
        _check(raw, method, kw, 'plain P = %d' % P)
        if dtype == F:
            raw = (raw + 1000.0).astype(F)
            raw[n // 2, P // 3] = np.inf
        calib, cal = _calibrated(rng, raw)
        pm = (rng.random(P) < 0.1).astype(np.uint8)
        _check(raw, method, kw, 'fused P = %d %s' % (P, np.dtype(dtype).name), values=cal, calib=calib)
        _check(raw, method, kw, 'fused + mask P = %d %s' % (P, np.dtype(dtype).name), values=cal, calib=calib, pixmask=pm)
        _check(raw, method, kw, 'mask P = %d %s' % (P, np.dtype(dtype).name), pixmask=pm)


@pytest.mark.parametrize('method, kw', RULES, ids=[r[0] for r in RULES])
def test_row_stripes(method, kw):
    """frames[:, r0:r1] of a contiguous slab is reduced in place (frame_stride > n_pixels)."""
    rng = np.random.default_rng(5)
    n, H, W = 10, 19, 67
    for dtype in (F, np.uint16):
        cube = synth_cube(rng, n, (H, W), nan_frac=0.01 if dtype == F else 0.0, dtype=dtype)
        t = _dev(cube)
        for r0, r1 in ((0, 5), (5, 6), (7, 19)):
            stripe = t[:, r0:r1]
            assert stripe.stride(0) == H * W
            _check(stripe, method, kw, 'rows %d:%d' % (r0, r1), values=cube[:, r0:r1].astype(F))


def test_nonfinite_values_and_ties():
    rng = np.random.default_rng(8)
    n, P = 20, 300
    cube = synth_cube(rng, n, (P,), nan_frac=0.15)
    cube[:, 0] = np.nan                                      # nothing finite
    cube[:, 1] = np.inf
    cube[:, 2] = [np.nan, np.inf, -np.inf, 1.0] * 5          # few finite values
    cube[1:, 3] = np.nan                                     # one value
    cube[2:, 4] = -np.inf                                    # two
    cube[:, 5] = 3.5                                         # constant
    cube[:, 6] = [0.0, -0.0] * 10                            # zeros of both signs
    cube[:, 7] = -0.0
    for kw in (dict(), dict(sigma_lower=1.0, sigma_upper=4.0), dict(maxiters=1), dict(sigma_lower=0.0, sigma_upper=0.0)):
        _check(cube, 'winsorized', kw, 'non-finite %r' % (kw,))
    for nlow, nhigh in ((1, 1), (0, 3), (4, 0), (10, 10), (0, 0), (127, 127)):
        _check(cube, 'minmax', dict(nlow=nlow, nhigh=nhigh), 'non-finite minmax %d %d' % (nlow, nhigh))
    # low-range integer data full of ties: which of the equal values goes decides the bits of the sum
    pool = np.array([1e-7, 0.3, 1.0000001, 7e6, -7e6, 3e13, -3e13, -0.0, 0.0], F)     # few values, float64 sums that round
    for n in (9, 24, 31, 100):
        ties = rng.integers(0, 4, (n, 500)).astype(F) * F(0.1) + F(1e4)
        ties[rng.random(ties.shape) < 0.1] = -0.0
        ties[rng.random(ties.shape) < 0.1] = 0.0
        wide = rng.choice(pool, (n, 500))
        for nlow, nhigh in ((1, 1), (2, 3)):
            _check(wide, 'minmax', dict(nlow=nlow, nhigh=nhigh), 'wide ties n = %d minmax %d %d' % (n, nlow, nhigh))
        _check(wide, 'winsorized', dict(sigma_lower=2.0, sigma_upper=2.0), 'wide ties n = %d winsorized' % n)
        for nlow, nhigh in ((1, 1), (3, 2), (0, 5)):
            _check(ties, 'minmax', dict(nlow=nlow, nhigh=nhigh), 'ties n = %d minmax %d %d' % (n, nlow, nhigh))
        _check(ties.astype(np.uint16), 'minmax', dict(nlow=2, nhigh=2), 'uint16 ties n = %d' % n)
        _check(ties, 'winsorized', dict(sigma_lower=1.5, sigma_upper=1.5), 'ties n = %d winsorized' % n)


@pytest.mark.parametrize('n', [5, 8, 12, 33, 64])
def test_orderstat_lines_as_columns(n):
    """The conformance table's lines, one per pixel: the middle pair sits on a digit boundary, is repeated, is a zero of
    either sign, is infinite ...  kl = kh = 0 puts both bounds ON the median - a median that is off by one key keeps another
    set; the other bounds fall between the fillers."""
    lines = [c.values for c in oc.cases(np.float32, n)]
    cube = np.ascontiguousarray(np.stack(lines, 1))
    with np.errstate(all='ignore'):
        for kl, kh in ((0.0, 0.0), (0.0, 3.0), (1.0, 1.0), (3.0, 0.5)):
            _check(cube, 'winsorized', dict(sigma_lower=kl, sigma_upper=kh), 'lines n = %d kl = %g kh = %g' % (n, kl, kh))
        for nlow, nhigh in ((1, 1), (n // 2, 0), (0, n // 2), ((n - 1) // 2, (n - 1) // 2)):
            _check(cube, 'minmax', dict(nlow=nlow, nhigh=nhigh), 'lines n = %d minmax %d %d' % (n, nlow, nhigh))


# ---------------------------------------------------------------------------------------------------------------------------
# guard bands
@pytest.fixture(scope='module')
def guard_data():
    rng = np.random.default_rng(77)
    n, P = 13, 1031
    raw = synth_cube(rng, n, (P,), dtype=np.uint16)
    calib_raw = {}
    from oracle import apref
    bias, dark, flat = synth_masters(rng, (P,))
    nflat, _ = apref.flat_normalize(flat)
    e = rng.uniform(0.3, 0.5, n).astype(F)
    cal = np.asarray(apref.calibrate(raw.reshape(n, 1, P), bias, dark, nflat, [float(v) for v in e], None, True), F).reshape(n, P)
    pm = (rng.random(P) < 0.05).astype(np.uint8)
    calib_raw.update(bias=bias, dark=dark, nflat=nflat, e=e)
    f32 = synth_cube(rng, n, (P,), nan_frac=0.02)
    return dict(raw=raw, cal=cal, pm=pm, f32=f32, refs={}, **calib_raw)


@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('method, kw', RULES, ids=[r[0] for r in RULES])
def test_guard_bands(method, kw, shift, guard_data, monkeypatch):
    """Two poisons, inputs one element off alignment, a side stream: no load outside an input reaches a result, no store
    leaves an output, no input is written, and the call runs on the current stream."""
    from astrophotography_amd import ops
    d = guard_data
    G = 64 * 1024

    def run(poison):
        with guarded(monkeypatch, G) as g:
            toks = []

            def dev(a):
                t, tok = place(a, poison, shift * a.dtype.itemsize, G)
                toks.append(tok)
                return t
            calib = dict(bias=dev(d['bias']), dark=dev(d['dark']), nflat=dev(d['nflat']), exp_ratio=d['e'], dark_still_biased=True)
            r1 = ops.stack_reject(dev(d['raw']), method, calib=calib, pixmask=dev(d['pm']), outputs=OUTPUTS, **kw)
            r2 = ops.stack_reject(dev(d['f32']), method, outputs=OUTPUTS, **kw)
            torch.cuda.current_stream().synchronize()
            for tok in toks:
                unchanged(tok)
            out = [{k: v.cpu().numpy() for k, v in r.items()} for r in (r1, r2)]
        return out, g.lib.streams()

    default = torch.cuda.default_stream().cuda_stream
    A, sa = run(0xFF)
    assert sa and all(s == default for _, s in sa)
    B, _ = run(0x00)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Cr, sc = run(0xFF)
    assert sc and all(s == side.cuda_stream for _, s in sc)
    key = (method, 'fused'), (method, 'plain')
    for i, (values, pm) in enumerate(((d['cal'], d['pm']), (d['f32'], None))):
        if key[i] not in d['refs']:
            d['refs'][key[i]] = _model(values, method, kw, pm)
        ref = d['refs'][key[i]]
        _compare({k: torch.from_numpy(v) for k, v in A[i].items()}, ref, 'run A %d' % i)
        for other, tag in ((B, 'poison 0x00'), (Cr, 'side stream')):
            for k in OUTPUTS:
                assert_biteq(other[i][k], A[i][k], '%s: %s' % (tag, k))


@pytest.mark.parametrize('flag_name', ['STACK_REJECT_WINSORIZED', 'STACK_REJECT_MINMAX'])
def test_caller_workspace_is_left_alone(flag_name, guard_data):
    """A workspace handed over with the call - the size the sigma clip would want - is neither read nor written."""
    from astrophotography_amd import _lib
    lib = _lib.load()
    d = guard_data
    n, P = d['f32'].shape
    zero = C.c_size_t(0)
    nb = lib.apgpu_stack_ws_bytes(P, C.byref(zero))
    results = []
    for poison in (0xFF, 0x00):
        ws, tok = place(np.full(nb, 0x5A, np.uint8), poison, 0)
        frames, ftok = place(d['f32'], poison, 0)
        mean = torch.empty(P, dtype=torch.float32, device='cuda')
        count = torch.empty(P, dtype=torch.int32, device='cuda')
        a = _lib.StackArgs()
        a.frames, a.dtype, a.n_frames, a.n_pixels, a.frame_stride = frames.data_ptr(), 0, n, P, P
        a.center, a.dev, a.maxiters = 0, 0, -1
        a.sigma_lower, a.sigma_upper = (2.0, 2.0) if 'WINSOR' in flag_name else (1.0, 1.0)
        a.mean, a.count = mean.data_ptr(), count.data_ptr()
        a.flags = getattr(_lib, flag_name) | _lib.STACK_EXACT_MOMENTS | _lib.STACK_MOMENTS_MEAN | _lib.STACK_SINGLE_KERNEL
        a.workspace, a.workspace_bytes = ws.data_ptr(), nb
        _lib.check(lib.apgpu_stack_sigclip(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        unchanged(tok)
        unchanged(ftok)
        results.append((mean.cpu().numpy(), count.cpu().numpy()))
    ref = (model.winsorized(d['f32'], 2.0, 2.0) if 'WINSOR' in flag_name else model.minmax(d['f32'], 1, 1))
    assert_biteq(results[0][0], ref['mean_f64'].astype(F))
    assert_biteq(results[0][1], ref['count'])
    assert_biteq(results[1][0], results[0][0])
    assert_biteq(results[1][1], results[0][1])


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: ten frames, a trail on two of them
SKY, NOISE, TRAIL = 100.0, 5.0, 400.0


@pytest.fixture(scope='module')
def trail_stack():
    rng = np.random.default_rng(2026)
    n, shape = 10, (48, 80)
    cube = rng.normal(SKY, NOISE, (n,) + shape).astype(F)
    on = np.zeros(shape, bool)
    for x in range(8, 72):
        y = 6 + x // 2
        on[y, x] = on[y + 1, x] = True
    for f in (2, 6):
        cube[f][on] += TRAIL
    return cube, on


def _trail_checks(image, count, on, rule, interior=None):
    """WINSORIZED / MINMAX(nhigh = 2): no trace of the trail.  A trail pixel's result is the mean of m of its 8 clean values,
    each N(SKY, NOISE) (a clip only narrows them): its deviation from SKY has a standard deviation of at most NOISE / sqrt(m).
    m >= 4 here; 6 standard deviations over the ~130 trail pixels are exceeded with probability 130 * 2e-9.
    CLIPPED: the two trail values inflate the std they are judged by (3 sigma of [8 x 0, 2 x 400] is 480) and stay: the mean
    is SKY + 2 * TRAIL / 10 = SKY + 80 give or take the same noise."""
    sel = on if interior is None else (on & interior)
    assert sel.sum() > 60
    img, cnt = image[sel].astype(np.float64), count[sel]
    if rule == 'CLIPPED':
        assert (cnt == 10).all()
        assert (img > SKY + 0.2 * TRAIL - 6 * NOISE / np.sqrt(10)).all()
        return
    assert (cnt <= 8).all() and (cnt >= 4).all(), (cnt.min(), cnt.max())
    assert (np.abs(img - SKY) <= 6 * NOISE / np.sqrt(cnt)).all(), float(np.abs(img - SKY).max())


def test_trail_ops_and_apstack(trail_stack):
    import astrophotography_amd as ap
    from astrophotography_amd import ops
    cube, on = trail_stack
    t = _dev(cube)
    flat = cube.reshape(10, -1)
    w = ops.stack_reject(t, 'winsorized', outputs=('mean', 'count'))
    _trail_checks(w['mean'].cpu().numpy(), w['count'].cpu().numpy(), on, 'WINSORIZED')
    assert_biteq(w['mean'].cpu().numpy().reshape(-1), model.winsorized(flat)['mean_f64'].astype(F))
    m = ops.stack_reject(t, 'minmax', nlow=0, nhigh=2, outputs=('mean', 'count'))
    _trail_checks(m['mean'].cpu().numpy(), m['count'].cpu().numpy(), on, 'MINMAX')
    assert (m['count'] == 8).all()
    c = ops.stack_sigclip(t, sigma=3.0, maxiters=5, outputs=('mean', 'count'))
    _trail_checks(c['mean'].cpu().numpy(), c['count'].cpu().numpy(), on, 'CLIPPED')
    st = ap.ApStack('CRITICAL', sigma=3.0, maxiters=None, nlow=0, nhigh=2)
    r = st.stack(t, method='winsorized', outputs=('mean', 'count'))
    assert_biteq(r['mean'].cpu().numpy(), w['mean'].cpu().numpy())
    r = st.stack(t, method='minmax', outputs=('mean', 'count', 'std'))
    assert_biteq(r['mean'].cpu().numpy(), m['mean'].cpu().numpy())
    assert_biteq(r['std'].cpu().numpy().reshape(-1), model.minmax(flat, 0, 2)['std_f64'].astype(F))


def test_trail_apstack_files(trail_stack, tmp_path):
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio
    cube, on = trail_stack
    names = []
    for i in range(cube.shape[0]):
        names.append(str(tmp_path / ('f%d.fits' % i)))
        fitsio.write(names[-1], cube[i], fitsio.Header())
    st = ap.ApStack('CRITICAL', sigma=2.5, maxiters=None, nlow=0, nhigh=2)
    st.stack_files(names, str(tmp_path / 'w.fits'), method='winsorized')
    img, h = fitsio.read(str(tmp_path / 'w.fits'))
    assert_biteq(img.reshape(-1), model.winsorized(cube.reshape(10, -1), 2.5, 2.5)['mean_f64'].astype(F))
    assert h['STACKMET'] == 'winsorized' and h['STACKSGL'] == 2.5 and h['STACKSGH'] == 2.5 and h['STACKITR'] == -1
    assert any('Winsorized' in str(v) for v in h.history())
    st.stack_files(names, str(tmp_path / 'm.fits'), method='minmax')
    img, h = fitsio.read(str(tmp_path / 'm.fits'))
    assert_biteq(img.reshape(-1), model.minmax(cube.reshape(10, -1), 0, 2)['mean_f64'].astype(F))
    assert h['STACKMET'] == 'minmax' and h['STACKNLO'] == 0 and h['STACKNHI'] == 2
    assert any('Min/max' in str(v) for v in h.history())


def test_trail_coadd_and_script(trail_stack, tmp_path):
    import yaml
    from astrophotography_amd import fitsio, ops
    from astrophotography_amd.scripts import ap_coadd
    cube, on = trail_stack
    n, (H, W) = cube.shape[0], cube.shape[1:]
    ident = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * n
    t = _dev(cube)
    res, _ = ops.resample_affine(t, ident, weight=False)
    res_h = res.cpu().numpy()
    interior = np.isfinite(res_h).all(0)
    assert interior[8:-8, 8:-8].all()
    for rule, kw in (('WINSORIZED', dict(sigma=3.0, maxiters=None)), ('MINMAX', dict(nlow=0, nhigh=2)), ('CLIPPED', dict(sigma=3.0, maxiters=5))):
        r = ops.coadd(t, ident, combine=rule, **kw)
        _trail_checks(r['image'].cpu().numpy(), r['count'].cpu().numpy(), on, rule, interior)
    r = ops.coadd(t, ident, combine='winsorized', sigma=3.0, maxiters=None)
    assert_biteq(r['image'].cpu().numpy().reshape(-1), model.winsorized(res_h.reshape(n, -1))['mean_f64'].astype(F))
    # the script: frames of one exposure, identity transforms
    names = []
    for i in range(n):
        names.append(str(tmp_path / ('c%d.fits' % i)))
        h = fitsio.Header()
        h['EXPOSURE'] = 1.0
        fitsio.write(names[-1], cube[i], h)
    with open(tmp_path / 't.yml', 'w') as fh:
        yaml.safe_dump({'transforms': {'c%d.fits' % i: ident[i] for i in range(n)}}, fh)
    for rule, extra in (('WINSORIZED', ['--sigma', '3', '--maxiters', '-1']), ('MINMAX', ['--nlow', '0', '--nhigh', '2']), ('CLIPPED', [])):
        out, wout = str(tmp_path / (rule + '.fits')), str(tmp_path / (rule + '_w.fits'))
        assert ap_coadd.main([out, *names, '--transforms', str(tmp_path / 't.yml'), '--combine', rule, '--weight_image', wout,
                              '-l', 'CRITICAL', *extra]) == 0
        img, h = fitsio.read(out)
        cnt, _ = fitsio.read(wout)
        assert h['COMBINET'] == rule
        _trail_checks(img, cnt.astype(np.int32), on, rule, interior)
        if rule == 'MINMAX':
            assert h['COMBNLO'] == 0 and h['COMBNHI'] == 2
        if rule == 'WINSORIZED':
            assert h['COMBSIG'] == 3.0 and h['COMBITR'] == -1
