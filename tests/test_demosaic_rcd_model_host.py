"""The NumPy statement of F10's RCD method (tests/demosaic_rcd_model.py) on the CPU: what the definition promises
before any kernel is compared with it - constant mosaics come back exactly, a mirrored mosaic gives the mirrored planes bit for
bit, the edges and stars are closer to the truth than the MHC model's, and a sample reaches no farther than the exported halo."""
import numpy as np
import pytest

from astrophotography_amd import _lib
from tests import demosaic_model as dm
from tests import demosaic_rcd_model as rm

F = np.float32
SIDE, EDGE = 96, 12                       # the scenes; the interior leaves out EDGE >= the halo on every side


def test_halo_is_the_exported_one():
    assert rm.HALO == _lib.DEMOSAIC_RCD_HALO and rm.PAD >= rm.HALO and rm.PAD % 2 == 0


@pytest.mark.parametrize('shape', [(2, 2), (2, 3), (5, 7), (33, 41)])
def test_constant_mosaics_come_back_exactly(shape):
    # eps and epssq are powers of two: every ratio is 1/2 or 1, every difference 0, every sum below 2^24 in integers
    levels = (1200, 3000, 700)
    for pat in dm.ARRANGEMENTS.values():
        got = rm.demosaic(np.full(shape, 65535, np.uint16), pat)
        assert np.array_equal(got, np.full((3,) + shape, 65535, F)), pat
        assert np.array_equal(rm.demosaic(np.full(shape, 65535, np.uint16), pat, output='rgb_u16'), np.full((3,) + shape, 65535, np.uint16))
        mosaic = np.array([levels[0], levels[1], levels[2], levels[1]], np.uint16)[dm.colour_map(shape, pat)]
        for dtype in (np.uint16, F):
            got = rm.demosaic(mosaic.astype(dtype), pat)
            for c, v in enumerate(levels):
                assert np.array_equal(got[c], np.full(shape, v, F)), (pat, dtype, c)


def _mirrored_pattern(pat, axis, n):
    """The pattern of the mosaic flipped along axis (0 rows, 1 columns) when that axis has n samples."""
    if n % 2:                                                        # the sample at 0 keeps its parity
        return tuple(pat)
    cell = np.array(pat).reshape(2, 2)
    return tuple(int(v) for v in (cell[::-1] if axis == 0 else cell[:, ::-1]).ravel())


@pytest.mark.parametrize('shape', [(5, 7), (12, 9), (8, 10), (33, 41)])
def test_mirrored_mosaic_gives_the_mirrored_planes_bit_for_bit(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for i, pat in enumerate(dm.ARRANGEMENTS.values()):
        m = rng.integers(0, 65536, shape).astype(np.uint16) if i % 2 else rng.normal(900.0, 400.0, shape).astype(F)
        gain = (1.8371, 1.0, 1.4142, 1.0007)
        want = rm.demosaic(m, pat, None, gain).view(np.uint32)
        lr = rm.demosaic(m[:, ::-1], _mirrored_pattern(pat, 1, shape[1]), None, gain)[:, :, ::-1]
        tb = rm.demosaic(m[::-1], _mirrored_pattern(pat, 0, shape[0]), None, gain)[:, ::-1]
        assert np.array_equal(lr.view(np.uint32), want), ('left-right', pat)
        assert np.array_equal(tb.view(np.uint32), want), ('top-bottom', pat)


# -- quality against the MHC model --------------------------------------------------------------------------------------------
def _scenes():
    """True colour planes [3, SIDE, SIDE]: a vertical step, a step along x + 0.6 y, 40 Gaussian stars of sigma 1.3 px."""
    yy, xx = np.indices((SIDE, SIDE)).astype(np.float64)
    dark, bright = np.array([500.0, 500.0, 500.0]), np.array([2700.0, 3000.0, 2400.0])
    scenes = {}
    for name, lit in (('vertical step', xx > 47.3), ('diagonal step', xx + 0.6 * yy > 75.2)):
        scenes[name] = (dark[:, None, None] + (bright - dark)[:, None, None] * lit).astype(F)
    rng = np.random.default_rng(40)
    img = np.zeros((3, SIDE, SIDE))
    for _ in range(40):
        y, x = rng.uniform(8, SIDE - 8, 2)
        amp = 10.0 ** rng.uniform(2.5, 4.3)
        colour = rng.uniform(0.5, 1.0, 3)
        img += (amp * colour)[:, None, None] * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * 1.3 ** 2))
    scenes['40 stars'] = (img + np.array([300.0, 500.0, 250.0])[:, None, None]).astype(F)
    return scenes


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def _errors(rgb, truth):
    inner = (slice(None), slice(EDGE, -EDGE), slice(EDGE, -EDGE))
    diff = lambda v: np.stack([v[0] - v[1], v[2] - v[1]]).astype(np.float64)
    return _rms(rgb[inner].astype(np.float64) - truth[inner]), _rms(diff(rgb)[inner] - diff(truth)[inner])


@pytest.mark.parametrize('scene', ['vertical step', 'diagonal step', '40 stars'])
def test_closer_to_the_truth_than_the_mhc_model(scene):
    truth = _scenes()[scene]
    for name in ('RGGB', 'GBRG'):
        pat = dm.ARRANGEMENTS[name]
        channel = np.array([0, 1, 2, 1])[dm.colour_map((SIDE, SIDE), pat)]
        mosaic = np.take_along_axis(truth, channel[None], 0)[0]
        rcd = _errors(rm.demosaic(mosaic, pat), truth)
        mhc = _errors(dm.demosaic(mosaic, pat, method='mhc'), truth)
        print('%s %s: RMS error RCD %.1f MHC %.1f; colour-difference RMS RCD %.1f MHC %.1f' % (scene, name, rcd[0], mhc[0], rcd[1], mhc[1]))
        assert rcd[0] < mhc[0] and rcd[1] < mhc[1], (scene, name, rcd, mhc)


def test_reach_of_a_sample_is_within_the_halo():
    rng = np.random.default_rng(9)
    m = rng.integers(1000, 60000, (41, 43)).astype(np.uint16)
    reach = 0
    for pat in dm.ARRANGEMENTS.values():
        base = rm.demosaic(m, pat).view(np.uint32)
        for r, c in ((20, 21), (21, 22)):
            for v in (0, 65535):
                p = m.copy()
                p[r, c] = v
                changed = np.argwhere((rm.demosaic(p, pat).view(np.uint32) != base).any(0))
                reach = max(reach, int(np.abs(changed - (r, c)).max()))
    print('reach of a perturbed sample: %d' % reach)
    assert 5 < reach <= rm.HALO
