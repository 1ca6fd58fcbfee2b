"""F13 on the host: the NumPy model tests/multiscale_model.py against what it must do - the noise constants, the
identity, pure noise, a synthetic scene - and the argument checks of ApMultiscale and ap_multiscale.  Nothing here needs a GPU."""
import numpy as np
import pytest

from tests import multiscale_model as mm

F = np.float32
SIGMA_E = (0.890796, 0.200664, 0.085508, 0.041217, 0.020425, 0.010190)


@pytest.fixture(scope='module')
def scene():
    return mm.scene()


def test_noise_constants():
    se = mm.noise_constants(6)
    print('sigma_e', se.tolist())
    assert se.shape == (6,) and se.dtype == np.float64
    assert np.all(np.abs(se - np.array(SIGMA_E)) <= 1e-5)
    assert np.array_equal(mm.noise_constants(3), se[:3])
    from astrophotography_amd import ops                                  # the host's own computation: the same numbers
    assert np.array_equal(ops.starlet_noise_constants(6), se)


def test_noise_constants_are_the_std_of_the_planes():
    """Unit white noise far from the borders: the planes' standard deviations are the constants (256^2 samples: 1.5 %)."""
    rng = np.random.default_rng(3)
    ws, _ = mm.planes(rng.normal(0.0, 1.0, (256, 256)).astype(F), 3)
    for w, se in zip(ws, mm.noise_constants(3)):
        assert abs(w[40:-40, 40:-40].std() / se - 1.0) < 0.05


@pytest.mark.parametrize('J', [1, 4, 6])
def test_identity(J):
    """k = 0 and gains 1: the planes sum to the image again, to within the 2 J + 1 float32 roundings of magnitudes <= 2 max|image|."""
    rng = np.random.default_rng(5)
    img = rng.normal(300.0, 10.0, (96, 130)).astype(F)
    img[10:14, 20:30] = np.nan
    img[50, 60] = np.inf
    for mode in ('hard', 'soft'):
        out, rep = mm.multiscale(img, J, k=0.0, gains=1.0, g_res=1.0, mode=mode, sigma=10.0)
        ok = np.isfinite(img)
        assert np.array_equal(np.isnan(out), ~ok) and np.all(rep['t'] == 0)
        err = np.abs(out[ok].astype(np.float64) - img[ok]).max()
        bound = (2 * J + 2) * 2.0 ** -23 * np.abs(img[ok]).max()
        print('identity J %d %s: max error %.3g, bound %.3g' % (J, mode, err, bound))
        assert err <= bound


def test_pure_noise():
    rng = np.random.default_rng(7)
    img = rng.normal(300.0, 10.0, (256, 256)).astype(F)
    out, rep = mm.multiscale(img, 4, k=3.0, mode='hard', sigma=10.0)
    ratio = out.std() / img.std()
    print('pure noise: output std / input std = %.4f' % ratio)
    assert ratio <= 0.20
    assert np.allclose(rep['t'], 30.0 * mm.noise_constants(4), rtol=1e-6)
    soft, _ = mm.multiscale(img, 4, k=3.0, mode='soft', sigma=10.0)
    assert soft.std() < out.std()                                         # shrinking every coefficient removes more


def test_step_is_a_normalised_convolution():
    """A constant image stays constant next to holes and borders, holes stay NaN, and far from both the step is the plain B3 blur."""
    img = np.full((40, 50), 7.25, F)
    img[5:9, 5:30] = np.nan
    img[20, 20] = -np.inf
    for s in (1, 4, 32):
        c = mm.step(img, s)
        assert np.array_equal(np.isnan(c), ~np.isfinite(img)) and np.all(c[np.isfinite(img)] == F(7.25))
    rng = np.random.default_rng(2)
    img = rng.normal(0.0, 1.0, (30, 30)).astype(F)
    c = mm.step(img, 2)
    k2 = np.outer(mm.TAPS, mm.TAPS)
    want = sum(k2[a, b] * float(img[15 + (a - 2) * 2, 11 + (b - 2) * 2]) for a in range(5) for b in range(5))
    assert abs(float(c[15, 11]) - want) < 1e-6
    one = mm.step(np.array([[3.5]], F), 8)                                # smaller than the halo: the centre tap alone
    assert one[0, 0] == F(3.5)


def test_scene_defaults_denoise(scene):
    d, truth, holes = scene['d'], scene['truth'], scene['holes']
    ok = ~holes
    out, rep = mm.multiscale(d)                                           # J = 4, k = (3, 3, 2, 1), hard, gains 1, sigma measured
    assert rep['J'] == 4 and rep['mode'] == 'hard'
    assert np.array_equal(np.isnan(out), holes)
    rms0 = np.sqrt(np.mean((d[ok].astype(np.float64) - truth[ok]) ** 2))
    rms1 = np.sqrt(np.mean((out[ok].astype(np.float64) - truth[ok]) ** 2))
    print('scene: rms against the truth %.3f -> %.3f; sigma measured %.3f (true %.1f)' % (rms0, rms1, rep['sigma'], scene['noise']))
    assert rms1 < 0.6 * rms0
    assert abs(rep['sigma'] / scene['noise'] - 1.0) <= 0.05               # the 5 % the GPU test asks of sigclip_global


def test_scene_zero_gains_remove_exactly_those_planes(scene):
    d = scene['d']
    ws, c4 = mm.planes(d, 4)
    out, _ = mm.multiscale(d, 4, k=0.0, gains=(0.0, 0.0, 1.0, 1.0), sigma=scene['noise'])
    with np.errstate(invalid='ignore'):
        want = (ws[2] + F(0)) + ws[3] + c4                                # +0 + w_3, then w_4, then the residual
    ok = ~scene['holes']
    assert np.array_equal(np.isnan(out), scene['holes'])
    assert np.array_equal(out[ok], want[ok])


def test_soft_and_hard_at_the_threshold():
    w = np.array([-2.0, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 2.0, np.nan], F)
    hard, soft = mm.treat(w, 1.0, 'hard'), mm.treat(w, 1.0, 'soft')
    assert hard.dtype == soft.dtype == F
    assert hard.tolist() == [-2.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 0.0]
    assert soft.tolist() == [-1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert np.array_equal(mm.treat(w[:8], 0.0, 'hard'), w[:8])


# ---- the class and the script: argument checks, no GPU ------------------------------------------------------------------------
def test_class_validation():
    from astrophotography_amd.core.ApMultiscale import ApMultiscale
    ms = ApMultiscale('ERROR')
    assert ms.scales == 4 and ms.k.tolist() == [3.0, 3.0, 2.0, 1.0] and ms.gains.tolist() == [1.0] * 4 and ms.mode == 'hard'
    assert ms.residual_gain == 1.0 and ms.sigma is None
    assert ApMultiscale('ERROR', scales=6).k.tolist() == [3.0, 3.0, 2.0, 1.0, 1.0, 1.0]
    assert ApMultiscale('ERROR', scales=3, k=2.5, gains=(1, 2, 0)).k.tolist() == [2.5] * 3
    for kw in (dict(scales=0), dict(scales=7), dict(scales=2.5), dict(k=(3, 3, 2)), dict(gains=(1, 1)), dict(k=-1.0), dict(k=(3, 3, 2, float('nan'))),
               dict(gains=float('inf')), dict(gains=(1, 1, 1, float('nan'))), dict(residual_gain=float('nan')), dict(mode='garrote'),
               dict(sigma=-1.0), dict(sigma=float('inf'))):
        with pytest.raises(ValueError):
            ApMultiscale('ERROR', **kw)
    import astrophotography_amd.core.ApMultiscale as module
    for key in ('MSCALES', 'MSMODE', 'MSSIGMA', 'MSK1', 'MSG1', 'MSGRES'):
        assert key in ApMultiscale.CARDS and key in module.__doc__        # one line per card group in the docstring
    with pytest.raises(ValueError):
        ms.process(np.zeros((4, 4), F))                                   # not a device tensor


def test_script_arguments():
    from astrophotography_amd.scripts import ap_multiscale as script
    p = script.command_line_opts(['in.fits', 'out.fits'])
    assert (p.input, p.output, p.scales, p.threshold, p.gain, p.residual_gain, p.mode, p.sigma, p.loglevel) == \
        ('in.fits', 'out.fits', 4, None, [1.0], 1.0, 'hard', None, 'INFO')
    p = script.command_line_opts(['a', 'b', '--scales', '5', '--threshold', '3,3,2,1,0', '--gain', '1,1.3,1.3,1,1', '--residual_gain', '0.9',
                                  '--mode', 'soft', '--sigma', '4.1', '-l', 'DEBUG'])
    assert (p.scales, p.threshold, p.gain, p.residual_gain, p.mode, p.sigma, p.loglevel) == \
        (5, [3.0, 3.0, 2.0, 1.0, 0.0], [1.0, 1.3, 1.3, 1.0, 1.0], 0.9, 'soft', 4.1, 'DEBUG')
    for bad in (['a', 'b', '--mode', 'garrote'], ['a', 'b', '--threshold', '3;2'], ['a'], ['a', 'b', '--scales', 'four']):
        with pytest.raises(SystemExit):
            script.command_line_opts(bad)
    with pytest.raises(ValueError):                                       # the class refuses what the parser cannot judge
        script.main(['a', 'b', '--scales', '9', '-l', 'ERROR'])
    with pytest.raises(ValueError):
        script.main(['a', 'b', '--scales', '3', '--gain', '1,2', '-l', 'ERROR'])


def test_ops_host_side_checks():
    from astrophotography_amd import ops
    with pytest.raises(ValueError):
        ops.starlet_noise_constants(7)
    with pytest.raises(ValueError):
        ops.starlet_noise_constants(0)
