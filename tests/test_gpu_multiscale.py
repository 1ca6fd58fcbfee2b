"""F13 on the GPU (csrc/multiscale.hip) against the NumPy model tests/multiscale_model.py: the step in both of its forms,
the planes and the whole call bit for bit, NaN positions included, and ApMultiscale / ap_multiscale end to end on the synthetic
scene of tests/test_multiscale_model_host.py."""
import numpy as np
import pytest

from tests import multiscale_model as mm

pytestmark = pytest.mark.gpu

F = np.float32
TH, TW = 32, 64                                                       # APGPU_STARLET_TILE_H, APGPU_STARLET_TILE_W: the tile form
CHAIN, BLOCK = 8, 256                                                 # APGPU_STARLET_CHAIN rows s apart per lane, 256 columns per workgroup: the direct form
TILE_MAX = 8                                                          # APGPU_STARLET_TILE_MAX_SPACING
SPACINGS = (1, 2, 4, 8, 16, 32)
WIDTHS = (TW - 1, TW, TW + 1, 2 * TW + 4, 2 * TW + 7, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 4, 2 * BLOCK + 7)


def _heights(s):
    return sorted({TH - 1, TH, TH + 1, 2 * TH + 9, CHAIN * s - 1, CHAIN * s, CHAIN * s + 1, 2 * CHAIN * s + 3})


def _forms(s):
    return ('auto', 'tile', 'direct') if s <= TILE_MAX else ('auto', 'direct')


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(got, want, what=''):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, 'NaN positions differ at', np.argwhere(gn != wn)[:5].tolist())
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~wn
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


def _image(rng, H, W, holes, s=1):
    img = rng.normal(300.0, 40.0, (H, W)).astype(F)
    if holes == 'isolated':
        bad = rng.random((H, W)) < 0.07
        img[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(bad.sum()))
    elif holes == 'lines':
        img[H // 2, :] = np.nan
        img[:, W // 3] = np.inf
    elif holes == 'block':
        img[5:5 + 4 * s + 7, 9:9 + 4 * s + 12] = np.nan                  # wider than the 4 s + 1 of the taps: pixels with M from far away only
    elif holes == 'seams':
        for y in sorted(set(range(TH - 1, H, TH)) | set(range(CHAIN * s - 1, H, CHAIN * s))):
            img[y:y + 2, ::3] = np.nan
        for x in sorted(set(range(TW - 1, W, TW)) | set(range(BLOCK - 1, W, BLOCK))):
            img[::2, x:x + 2] = -np.inf
        img[0, 0] = img[0, -1] = img[-1, 0] = img[-1, -1] = np.nan
        img[:2, :2] = np.nan
    elif holes == 'all':
        img[:] = np.nan
    return img


def _check_step(img, s, what):
    """c_{j+1} and w_{j+1} of one launch, in every form the spacing has."""
    import torch
    from astrophotography_amd import ops
    want = mm.step(img, s)
    with np.errstate(invalid='ignore'):
        want_w = np.where(np.isfinite(img), img - want, F(np.nan)).astype(F)
    d = _dev(img)
    for form in _forms(s):
        plane = torch.empty_like(d)
        got = ops.starlet_step(d, s, plane=plane, form=form)
        tag = '%s %s s %d %s' % (what, img.shape, s, form)
        _same_bits(got.cpu().numpy(), want, tag + ' c')
        _same_bits(plane.cpu().numpy(), want_w, tag + ' w')


@pytest.mark.parametrize('s', SPACINGS)
def test_step_shapes(s):
    """Heights and widths that straddle the tile edges of both forms, clean and with isolated non-finite pixels; images smaller than
    the halo."""
    rng = np.random.default_rng(300 + s)
    for H in _heights(s):
        for W in WIDTHS:
            _check_step(_image(rng, H, W, 'isolated' if (H + W) % 2 else 'none'), s, 'shapes')
    for shape in ((1, 1), (5, 7), (40, max(1, 2 * s - 1)), (max(1, 2 * s - 1), 70)):
        _check_step(_image(rng, shape[0], shape[1], 'none'), s, 'smaller than the halo')
    _check_step(_image(rng, 5, 7, 'isolated'), s, 'smaller than the halo')


@pytest.mark.parametrize('holes', ['isolated', 'lines', 'block', 'seams', 'all'])
def test_step_holes(holes):
    rng = np.random.default_rng(11)
    for s in SPACINGS:
        _check_step(_image(rng, 2 * TH + 86, BLOCK + 44, holes, s), s, holes)


def test_step_accumulates():
    """The fused part of the launch: threshold, gain, first / later / last step, both modes, against the model's pieces."""
    import torch
    from astrophotography_amd import ops
    rng = np.random.default_rng(12)
    img = _image(rng, 70, 150, 'isolated')
    prev = rng.normal(0.0, 50.0, img.shape).astype(F)
    d = _dev(img)
    for s in (1, 4, 16):
        cn = mm.step(img, s)
        with np.errstate(invalid='ignore'):
            w = (img - cn).astype(F)
            for mode in ('hard', 'soft'):
                for form in _forms(s):
                    tw = F(2.5) * mm.treat(w, F(30.0), mode)
                    for first, last in ((True, False), (False, False), (False, True), (True, True)):
                        want = (np.zeros_like(img) if first else prev) + tw
                        if last:
                            want = want + F(0.75) * cn
                        want = np.where(np.isfinite(img), want, F(np.nan)).astype(F)
                        acc = _dev(prev)
                        got_c = ops.starlet_step(d, s, acc=acc, threshold=30.0, gain=2.5, g_res=0.75, mode=mode, first=first, last=last, form=form)
                        tag = 'accumulate s %d %s %s first %d last %d' % (s, mode, form, first, last)
                        _same_bits(acc.cpu().numpy(), want, tag)
                        _same_bits(got_c.cpu().numpy(), cn, tag + ' c')
    acc = torch.zeros_like(d)
    assert ops.starlet_step(d, 2, out=False, acc=acc) is None             # the accumulator alone


def test_forms_agree():
    """Tile and direct form on one larger image, every output of the launch, at the spacings both are built for."""
    import torch
    from astrophotography_amd import ops
    rng = np.random.default_rng(13)
    img = _image(rng, 301, 707, 'isolated')
    img[100:140, 300:420] = np.nan
    d = _dev(img)
    for s in (1, 2, 4, 8):
        res = {}
        for form in ('tile', 'direct'):
            plane, acc = torch.empty_like(d), torch.empty_like(d)
            c = ops.starlet_step(d, s, plane=plane, acc=acc, threshold=25.0, gain=1.5, g_res=0.5, mode='soft', last=True, form=form)
            res[form] = [t.cpu().numpy() for t in (c, plane, acc)]
        for a, b, name in zip(res['tile'], res['direct'], ('c', 'w', 'acc')):
            _same_bits(a, b, 'forms s %d %s' % (s, name))


def test_planes():
    from astrophotography_amd import ops
    rng = np.random.default_rng(14)
    img = _image(rng, 2 * TH + 9, BLOCK + 13, 'isolated')
    img[20:40, 50:90] = np.nan
    for J in (1, 2, 5, 6):
        got = ops.starlet_planes(_dev(img), J).cpu().numpy()
        ws, cJ = mm.planes(img, J)
        assert got.shape == (J + 1,) + img.shape
        for j in range(J):
            _same_bits(got[j], ws[j], 'planes J %d w_%d' % (J, j + 1))
        _same_bits(got[J], cJ, 'planes J %d residual' % J)
    _same_bits(ops.starlet_plane1(_dev(img)).cpu().numpy(), mm.planes(img, 1)[0][0], 'plane 1 alone')


@pytest.mark.parametrize('mode', ['hard', 'soft'])
@pytest.mark.parametrize('J', [1, 4, 6])
def test_multiscale(J, mode):
    from astrophotography_amd import ops
    rng = np.random.default_rng(15 + J)
    img = _image(rng, 2 * TH + 45, BLOCK + 44, 'isolated')
    img[30:60, 100:170] = np.nan
    gains = (2.5, 0.0, 1.0, 1.7, 0.0, 0.6)[:J]
    k = (3.0, 0.0, 2.0, 1.0, 4.0, 0.5)[:J]
    got, rep = ops.multiscale(_dev(img), J, k, gains, 0.8, mode, sigma=40.0)
    want, wrep = mm.multiscale(img, J, k, gains, 0.8, mode, sigma=40.0)
    assert rep['J'] == J and rep['mode'] == mode and rep['sigma'] == 40.0
    assert np.array_equal(rep['t'].view(np.uint32), wrep['t'].view(np.uint32))
    _same_bits(got.cpu().numpy(), want, 'multiscale J %d %s' % (J, mode))
    # a scalar for every scale, the caller's workspace and output
    import torch
    ws, out = ops.starlet_workspace(img.shape, 'cuda'), torch.empty((img.shape[0], img.shape[1]), dtype=torch.float32, device='cuda')
    assert ws.numel() >= 8 * img.size
    got2, _ = ops.multiscale(_dev(img), J, 2.0, 1.25, 1.0, mode, sigma=40.0, ws=ws, out=out)
    assert got2.data_ptr() == out.data_ptr()
    _same_bits(out.cpu().numpy(), mm.multiscale(img, J, 2.0, 1.25, 1.0, mode, sigma=40.0)[0], 'multiscale scalars J %d %s' % (J, mode))


def _k_for(t, se):
    """A float64 k with float32(k 1.0 se) == t."""
    k = float(t) / float(se)
    for _ in range(8):
        r = F(k * 1.0 * float(se))
        if r == t:
            return k
        k = np.nextafter(k, np.inf if r < t else -np.inf)
    raise AssertionError('no k gives the threshold %r' % t)


@pytest.mark.parametrize('mode', ['hard', 'soft'])
def test_pixels_exactly_on_the_threshold(mode):
    """t_1 is the value of a positive pixel of the model's plane 1 and t_2 minus the value of a negative pixel of its plane 2: hard
    keeps those pixels, soft makes them +0, on the device as in the model."""
    from astrophotography_amd import ops
    rng = np.random.default_rng(16)
    img = _image(rng, 90, 140, 'none')
    ws, _ = mm.planes(img, 2)
    se = mm.noise_constants(2)
    p = np.argwhere((ws[0] > 30.0) & (ws[0] < 40.0))[0]
    q = np.argwhere((ws[1] < -7.0) & (ws[1] > -9.0))[0]
    t1, t2 = ws[0][p[0], p[1]], -ws[1][q[0], q[1]]
    k = (_k_for(t1, se[0]), _k_for(t2, se[1]))
    want, wrep = mm.multiscale(img, 2, k, 1.0, 1.0, mode, sigma=1.0)
    assert wrep['t'][0] == t1 and wrep['t'][1] == t2
    assert mm.treat(ws[0], t1, mode)[p[0], p[1]] == (t1 if mode == 'hard' else 0) and mm.treat(ws[1], t2, mode)[q[0], q[1]] == (-t2 if mode == 'hard' else 0)
    got, rep = ops.multiscale(_dev(img), 2, k, 1.0, 1.0, mode, sigma=1.0)
    assert rep['t'][0] == t1 and rep['t'][1] == t2
    _same_bits(got.cpu().numpy(), want, 'on the threshold, ' + mode)


def test_errors():
    import ctypes as C
    import torch
    from astrophotography_amd import _lib, ops
    rng = np.random.default_rng(17)
    d = _dev(_image(rng, 40, 70, 'none'))
    with pytest.raises(ValueError):
        ops.multiscale(torch.zeros((8, 8)), sigma=1.0)                    # a CPU tensor
    with pytest.raises(TypeError):
        ops.multiscale(d.double(), sigma=1.0)
    with pytest.raises(ValueError):
        ops.multiscale(d, 7, 3.0, sigma=1.0)
    with pytest.raises(ValueError):
        ops.multiscale(d, 4, (3, 3, 2), sigma=1.0)
    with pytest.raises(ValueError):
        ops.multiscale(d, 4, -1.0, sigma=1.0)
    with pytest.raises(ValueError):
        ops.multiscale(d, 4, 3.0, gains=float('inf'), sigma=1.0)
    with pytest.raises(ValueError):
        ops.multiscale(d, 4, 3.0, mode='garrote', sigma=1.0)
    with pytest.raises(ValueError, match='out'):
        ops.multiscale(d, sigma=1.0, out=d)
    with pytest.raises(ValueError, match='ws'):
        ops.multiscale(d, sigma=1.0, ws=ops.starlet_workspace(d.shape, 'cuda')[:-16])
    with pytest.raises(ValueError):
        ops.starlet_step(d, 4, form='lds')
    with pytest.raises(_lib.ApGpuError) as exc:
        ops.starlet_step(d, 3)
    assert exc.value.code == _lib.E_INVAL
    with pytest.raises(_lib.ApGpuError) as exc:
        ops.starlet_step(d, 64)
    assert exc.value.code == _lib.E_INVAL
    with pytest.raises(_lib.ApGpuError) as exc:
        ops.starlet_step(d, 16, form='tile')
    assert exc.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(_lib.ApGpuError) as exc:
        ops.starlet_step(d, 1, out=d)                                     # in place
    assert exc.value.code == _lib.E_INVAL
    with pytest.raises(_lib.ApGpuError) as exc:
        ops.starlet_step(d, 1, threshold=-1.0, acc=torch.empty_like(d))
    assert exc.value.code == _lib.E_INVAL
    with pytest.raises(RuntimeError, match='sigma'):                      # nothing to measure the noise from
        ops.multiscale(torch.full_like(d, float('nan')))
    lib = _lib.load()
    out, ws = torch.empty_like(d), ops.starlet_workspace(d.shape, 'cuda')
    t = np.ones(4, F)
    targ = t.ctypes.data_as(C.POINTER(C.c_float))
    rc = lib.apgpu_multiscale_f32(C.c_void_p(d.data_ptr()), 40, 70, 4, targ, targ, 1.0, 0, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                  ws.numel() - 1, None)
    assert rc == _lib.E_WORKSPACE
    rc = lib.apgpu_multiscale_f32(C.c_void_p(d.data_ptr()), 40, 70, 7, targ, targ, 1.0, 0, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                  ws.numel(), None)
    assert rc == _lib.E_INVAL


def test_unaligned_base_width_multiple_of_4():
    """A plane whose rows are a multiple of four floats but whose first pixel is not 16-byte aligned: the one branch of the shared
    staging (csrc/plane_tile.h) and of the `wide` predicate that a fresh allocation never takes.  The blur (csrc/continuum.hip), the
    tile form and the direct form give the bits of the model and of the aligned copy."""
    import torch
    from astrophotography_amd import ops
    from tests import continuum_model as cm
    H, W = TH + 1, 2 * TW + 4
    img = _image(np.random.default_rng(21), H, W, 'isolated')
    assert not np.isfinite(img).all() and np.isfinite(img).any()
    buf = torch.empty(H * W + 1, dtype=torch.float32, device='cuda')
    buf[1:].copy_(_dev(img).reshape(-1))
    shifted, aligned = buf[1:].view(H, W), _dev(img)
    assert shifted.data_ptr() % 16 != 0 and aligned.data_ptr() % 16 == 0 and shifted.is_contiguous() and W % 4 == 0
    for R in (2, 32):
        taps = cm.gauss_taps(R / 4.0, R)
        want = cm.gauss_blur(img, taps, 0.5)
        for d, tag in ((shifted, 'unaligned'), (aligned, 'aligned')):
            _same_bits(ops.gauss_blur(d, taps, 0.5).cpu().numpy(), want, 'blur R %d %s' % (R, tag))
    prev = np.random.default_rng(22).normal(0.0, 50.0, img.shape).astype(F)
    for s, form in ((1, 'tile'), (8, 'tile'), (1, 'direct')):
        cn = mm.step(img, s)
        with np.errstate(invalid='ignore'):
            w = np.where(np.isfinite(img), img - cn, F(np.nan)).astype(F)
            want_acc = np.where(np.isfinite(img), prev + F(2.5) * mm.treat((img - cn).astype(F), F(30.0), 'hard'), F(np.nan)).astype(F)
        for d, tag in ((shifted, 'unaligned'), (aligned, 'aligned')):
            plane, acc = torch.empty_like(aligned), _dev(prev)
            c = ops.starlet_step(d, s, plane=plane, acc=acc, threshold=30.0, gain=2.5, first=False, form=form)
            what = 'starlet s %d %s %s' % (s, form, tag)
            _same_bits(c.cpu().numpy(), cn, what + ' c')
            _same_bits(plane.cpu().numpy(), w, what + ' plane')
            _same_bits(acc.cpu().numpy(), want_acc, what + ' acc')


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    return mm.scene()


def test_class_reproduces_the_model(scene):
    import astrophotography_amd as ap
    d = scene['d']
    r = ap.ApMultiscale('ERROR').process(_dev(d), sigma=scene['noise'])
    want, _ = mm.multiscale(d, sigma=scene['noise'])
    rep = r['report']
    assert rep['J'] == 4 and rep['mode'] == 'hard' and rep['sigma'] == scene['noise'] and not rep['measured']
    _same_bits(r['image'].cpu().numpy(), want, 'class, sigma given')
    # the noise measured through sigclip_global: within 5 % of the scene's, and the model given that value gives the same image
    r = ap.ApMultiscale('ERROR', scales=5, k=(3, 3, 2, 1, 0), gains=(1, 1.3, 1.3, 1, 1), residual_gain=0.9, mode='soft').process(_dev(d))
    rep = r['report']
    print('measured sigma %.4f (scene %.1f; model %.4f)' % (rep['sigma'], scene['noise'], mm.estimate_sigma(d)))
    assert rep['measured'] and abs(rep['sigma'] / scene['noise'] - 1.0) <= 0.05
    want, _ = mm.multiscale(d, 5, (3, 3, 2, 1, 0), (1, 1.3, 1.3, 1, 1), 0.9, 'soft', sigma=rep['sigma'])
    _same_bits(r['image'].cpu().numpy(), want, 'class, sigma measured')
    ok = ~scene['holes']
    got = ap.ApMultiscale('ERROR').process(_dev(d))['image'].cpu().numpy()
    rms0 = np.sqrt(np.mean((d[ok].astype(np.float64) - scene['truth'][ok]) ** 2))
    rms1 = np.sqrt(np.mean((got[ok].astype(np.float64) - scene['truth'][ok]) ** 2))
    assert rms1 < 0.6 * rms0 and np.array_equal(np.isnan(got), scene['holes'])
    import torch
    with pytest.raises(RuntimeError, match='sigma'):
        ap.ApMultiscale('ERROR').process(torch.full((50, 60), float('nan'), device='cuda'))


def test_files_and_script(scene, tmp_path):
    from astrophotography_amd import fitsio
    from astrophotography_amd.scripts import ap_multiscale as script
    d = scene['d']
    hdr = fitsio.Header()
    hdr['FILTER'] = 'L'
    src, out = str(tmp_path / 'coadd.fits'), str(tmp_path / 'clean.fits')
    fitsio.write(src, d, header=hdr)
    assert script.main([src, out, '--scales', '3', '--threshold', '3,2,0', '--gain', '1,2.5,0', '--residual_gain', '0.5', '--mode', 'soft',
                        '--sigma', '5', '-l', 'ERROR']) == 0
    data, h = fitsio.read(out)
    for key in ('MSCALES', 'MSMODE', 'MSSIGMA', 'MSK1', 'MSK2', 'MSK3', 'MSG1', 'MSG2', 'MSG3', 'MSGRES'):
        assert key in h, key
    assert 'MSK4' not in h and 'MSG4' not in h
    assert (h['MSCALES'], h['MSMODE'], h['MSSIGMA'], h['MSK1'], h['MSK2'], h['MSK3'], h['MSG1'], h['MSG2'], h['MSG3'], h['MSGRES']) == \
        (3, 'SOFT', 5.0, 3.0, 2.0, 0.0, 1.0, 2.5, 0.0, 0.5)
    assert h['FILTER'] == 'L' and any('ApMultiscale' in line for line in h.history())
    want, _ = mm.multiscale(d, 3, (3, 2, 0), (1, 2.5, 0), 0.5, 'soft', sigma=5.0)
    _same_bits(np.asarray(data, F), want, 'script against the model')
    # the headline command: defaults, the noise measured
    out2 = str(tmp_path / 'clean2.fits')
    assert script.main([src, out2, '-l', 'ERROR']) == 0
    data2, h2 = fitsio.read(out2)
    assert h2['MSCALES'] == 4 and h2['MSMODE'] == 'HARD' and abs(h2['MSSIGMA'] / scene['noise'] - 1.0) <= 0.05
    assert [h2['MSK%d' % j] for j in (1, 2, 3, 4)] == [3.0, 3.0, 2.0, 1.0]
    want2, _ = mm.multiscale(d, sigma=h2['MSSIGMA'])
    _same_bits(np.asarray(data2, F), want2, 'headline image')
    allnan = str(tmp_path / 'nan.fits')
    fitsio.write(allnan, np.full((20, 30), np.nan, F))
    with pytest.raises(RuntimeError, match='sigma'):
        script.main([allnan, out2, '-l', 'ERROR'])


def test_uint16_file_is_widened_exactly(tmp_path):
    """A uint16 FITS (BZERO 32768) through the file shell: the pixels reach the kernels as their exact float32 values (0, 32767, 32768
    and 65535 are the ones a signed reading gets wrong), and the float32 output carries no BZERO / BSCALE."""
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio
    from astrophotography_amd.core import _common
    raw = np.array([[0, 32767, 32768, 65535], [65535, 0, 1, 32769], [32768, 32767, 65534, 2], [1, 65535, 0, 32768]], np.uint16)
    src, out = str(tmp_path / 'raw.fits'), str(tmp_path / 'out.fits')
    fitsio.write(src, raw)
    _, h0 = fitsio.read(src)
    assert h0['BITPIX'] == 16 and h0['BZERO'] == 32768
    log = _common.make_logger('ApMultiscale', 'ERROR')
    got, _ = _common.read_image_f32(log, src)
    assert got.dtype.is_floating_point and got.is_cuda and got.is_contiguous()
    _same_bits(got.cpu().numpy(), raw.astype(F), 'read_image_f32')
    rep = ap.ApMultiscale('ERROR', scales=2, k=0.0, gains=1.0, residual_gain=1.0).process_file(src, out, sigma=1.0)
    assert rep['J'] == 2
    data, h = fitsio.read(out)
    assert 'BZERO' not in h and 'BSCALE' not in h and h['BITPIX'] == -32
    want, _ = mm.multiscale(raw.astype(F), 2, (0.0, 0.0), (1.0, 1.0), 1.0, 'hard', sigma=1.0)
    _same_bits(np.asarray(data, F), want, 'uint16 file against the model of the widened input')
