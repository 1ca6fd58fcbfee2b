"""F10 on the host: the properties that pin tests/demosaic_model.py itself (a wrong coefficient or a colour slip shows here), the
white balance against golden group G18 (RawConv's own numbers), ApDebayer's argument errors, ap_debayer's flags and the bindings.
No device."""
import os

import numpy as np
import pytest

from tests import demosaic_model as dm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g18_whitebalance.npz')
F = np.float32


def _sample(planes, pattern):
    """The mosaic that sees planes [3, H, W] (R, G, B) through the arrangement."""
    k = dm.colour_map(planes.shape[1:], pattern)
    plane_of = np.array([0, 1, 2, 1])[k]
    return np.take_along_axis(planes, plane_of[None], 0)[0]


@pytest.mark.parametrize('name', sorted(dm.ARRANGEMENTS))
@pytest.mark.parametrize('method', ['bilinear', 'mhc'])
@pytest.mark.parametrize('shape', [(2, 2), (3, 2), (5, 7), (12, 10)])
def test_constant_colours_come_back_exactly(name, method, shape):
    # the reflection keeps colours, each filter's own-colour taps sum to 16/16 and its other-colour taps to 0
    a, b, c = 1234, 40000, 777
    planes = np.stack([np.full(shape, v, np.uint16) for v in (a, b, c)])
    got = dm.demosaic(_sample(planes, dm.ARRANGEMENTS[name]), dm.ARRANGEMENTS[name], method=method)
    assert got.dtype == F and got.shape == (3,) + shape
    for ch, v in enumerate((a, b, c)):
        assert np.array_equal(got[ch], np.full(shape, v, F)), (name, method, ch)


@pytest.mark.parametrize('name', sorted(dm.ARRANGEMENTS))
@pytest.mark.parametrize('method', ['bilinear', 'mhc'])
def test_linear_planes_come_back_exactly_inside(name, method):
    H, W = 13, 16
    r, c = np.indices((H, W))
    planes = np.stack([100 + 3 * r + 5 * c, 4000 + 7 * r + 2 * c, 900 + 11 * r + 13 * c]).astype(np.uint16)
    got = dm.demosaic(_sample(planes, dm.ARRANGEMENTS[name]), dm.ARRANGEMENTS[name], method=method)
    assert np.array_equal(got[:, 2:-2, 2:-2], planes[:, 2:-2, 2:-2].astype(F))
    f32 = dm.demosaic(_sample(planes, dm.ARRANGEMENTS[name]).astype(F), dm.ARRANGEMENTS[name], method=method)
    assert np.array_equal(f32, got)


def test_reflection_has_period_and_keeps_parity():
    for n in (2, 3, 5, 8):
        i = np.arange(-2 * n, 3 * n)
        f = dm.fold(i, n)
        assert f.min() == 0 and f.max() == n - 1 and np.array_equal(f & 1, i & 1)
        assert np.array_equal(f[(i >= 0) & (i < n)], np.arange(n))
    assert dm.fold(np.array([-1, -2, 5, 6]), 5).tolist() == [1, 2, 3, 2]


@pytest.mark.parametrize('name', sorted(dm.ARRANGEMENTS))
def test_superpixel_is_slicing(name):
    pat = dm.ARRANGEMENTS[name]
    rng = np.random.default_rng(5)
    m = rng.integers(0, 65536, (6, 10)).astype(np.uint16)
    black, gain = [10, 20, 30, 40], [2.0, 1.0, 1.5, 1.03125]
    got = dm.demosaic(m, pat, black, gain, 'superpixel')
    pos = {k: (p >> 1, p & 1) for p, k in enumerate(pat)}
    cell = lambda k: (np.maximum(m[pos[k][0]::2, pos[k][1]::2].astype(np.int64) - black[k], 0).astype(F) * F(gain[k]))
    assert got.shape == (3, 3, 5)
    assert np.array_equal(got[0], cell(0)) and np.array_equal(got[2], cell(2))
    assert np.array_equal(got[1], (cell(1) + cell(3)) * F(0.5))


def test_u16_clip_and_truncation_corners():
    v = np.array([-0.5, 65535.9, np.nan, 0.999, 1.0, 65534.99, np.inf, -np.inf, 70000.0], F)
    assert dm.to_u16(v).tolist() == [0, 65535, 0, 0, 1, 65534, 65535, 0, 65535]
    assert dm.to_u16(v).dtype == np.uint16


def test_sample_scaling_and_outputs():
    pat = dm.ARRANGEMENTS['GRBG']
    m = np.array([[5, 300], [100, 65535]], np.uint16)
    s = dm.demosaic(m, pat, black=[50, 10, 200, 0], gain=[2.0, 1.0, 0.5, 3.0], output='direct')
    # G1 at (0, 0): max(5 - 10, 0); R at (0, 1): (300 - 50) 2; B at (1, 0): max(100 - 200, 0); G2 at (1, 1): 65535 * 3
    assert np.array_equal(s, np.array([[0, 500], [0, 196605]], F))
    f = np.array([[np.nan, 1.5], [-3.0, np.inf]], F)
    s = dm.demosaic(f, pat, black=[0.25, 0, 0, 0], output='direct')
    assert np.isnan(s[0, 0]) and s[0, 1] == F(1.25) and s[1, 0] == 0 and np.isposinf(s[1, 1])
    rgb = dm.demosaic(m, pat, method='bilinear')
    y = dm.demosaic(m, pat, method='bilinear', output='grey')
    assert np.array_equal(y, (F(0.299) * rgb[0] + F(0.587) * rgb[1]) + F(0.114) * rgb[2])


def test_sums_use_python_integers():
    m = np.full((6, 8), 65535, np.uint16)
    sums, counts, _ = dm.channel_sums(m, dm.ARRANGEMENTS['RGGB'], [0, 1, 2, 3], [1, 4, 1, 100])
    assert counts == [6, 8, 8, 6]              # rows 1 .. 4, columns 1 .. 7: R on even rows and even columns, B on odd and odd
    assert sums == [6 * 65535, 8 * 65534, 8 * 65533, 6 * 65532]


def test_whitebalance_equals_rawconv_golden():
    from astrophotography_amd import ops
    g = np.load(GOLDEN)
    pat = tuple(int(v) for v in g['pattern'])
    assert len(g['cases']) == 12
    for name in g['cases']:
        m = g['mosaic_' + str(name)[0]]
        region = g['region_' + str(name)].tolist()
        region = None if region[0] < 0 else region
        black = g['black_' + str(name)].tolist()
        want = g['gains_' + str(name)]
        got = dm.whitebalance(m, pat, black, region)
        assert got.dtype == np.float64 and np.array_equal(got, want), (name, got, want)
        sums, counts, _ = dm.channel_sums(m, pat, black, region)
        assert np.array_equal(ops.whitebalance_from_sums(sums, counts), want)


def test_whitebalance_refuses_empty_and_dark_colours():
    from astrophotography_amd import ops
    with pytest.raises(ValueError, match='no valid pixels'):
        ops.whitebalance_from_sums([10, 10, 0, 10], [4, 4, 0, 4])
    with pytest.raises(ValueError, match='mean'):
        ops.whitebalance_from_sums([10, 0, 10, 10], [4, 4, 4, 4])


# -- ApDebayer: argument errors are raised before any device call (no device here) ---------------------------------------
def test_apdebayer_argument_errors():
    import astrophotography_amd as ap
    from astrophotography_amd.core import ApDebayer as mod
    assert 'ApDebayer' in ap.__all__ and ap.ApDebayer is mod.ApDebayer
    d = mod.ApDebayer('CRITICAL')
    mosaic = object()                                        # never looked at
    with pytest.raises(RuntimeError) as e:
        d.rgb(mosaic, (0, 1, 3, 2), wb_method='sunny')
    assert str(e.value) == ('Unexpected white balance method "sunny" not one of the allowed method: '
                            "['daylight', 'camera', 'auto', 'region', 'user']")
    for wb in ('camera', 'daylight'):
        with pytest.raises(NotImplementedError, match='LibRaw'):
            d.whitebalance(mosaic, (0, 1, 3, 2), wb)
        with pytest.raises(NotImplementedError, match='LibRaw'):
            d.grey(mosaic, (0, 1, 3, 2), wb_method=wb)
    for bad in ((0, 1, 2, 3), (0, 2, 1, 3), (0, 1, 1, 2), (0, 1, 3), (1, 1, 3, 3)):
        with pytest.raises(ValueError, match='Bayer arrangement'):
            d.rgb(mosaic, bad)
        with pytest.raises(ValueError, match='Bayer arrangement'):
            d.whitebalance(mosaic, bad, 'auto')
    with pytest.raises(ValueError, match='demosaic method'):
        d.rgb(mosaic, (0, 1, 3, 2), method='ahd')
    with pytest.raises(ValueError, match='luminance'):
        d.grey(mosaic, (0, 1, 3, 2), luminance_method='cubic')
    with pytest.raises(ValueError, match='four numbers'):
        d.whitebalance(mosaic, (0, 1, 3, 2), 'region[1, 2, 3]')
    assert d.whitebalance(mosaic, (0, 1, 3, 2), 'user[1.85, 1.0, 2.01, 1.0]').tolist() == [1.85, 1.0, 2.01, 1.0]
    assert d.whitebalance(mosaic, (0, 1, 3, 2), [2, 1, 1.5, 1]).tolist() == [2.0, 1.0, 1.5, 1.0]
    assert mod.parse_whitebalance('region[450, 463, 2850, 2863]') == ('region', [450, 463, 2850, 2863])


def test_pattern_names_and_offsets():
    from astrophotography_amd.core.ApDebayer import ARRANGEMENTS, pattern_of
    from astrophotography_amd import ops
    assert ARRANGEMENTS == dm.ARRANGEMENTS
    for name, pat in ARRANGEMENTS.items():
        assert ops.bayer_pattern(pat) == list(pat)
        assert ''.join('RGBG'[k] for k in pat) == name
    assert pattern_of('rggb') == (0, 1, 3, 2)
    assert pattern_of('RGGB', xoff=1) == (1, 0, 2, 3)          # one column in: G R / B G
    assert pattern_of('RGGB', yoff=1) == (3, 2, 0, 1)          # one row in: G B / R G (the greens keep their names)
    assert pattern_of('RGGB', 1, 1) == (2, 3, 1, 0)
    with pytest.raises(ValueError):
        pattern_of('RGBG')


def test_c_entry_points_refuse_bad_arguments_before_device_work():
    import ctypes as C
    from astrophotography_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(64)
    ptr = C.cast(buf, C.c_void_p)
    pat = lambda *v: (C.c_int32 * 4)(*v)
    call = lambda p, h=4, w=4, method=1, output=0: lib.apgpu_bayer_demosaic(ptr, _lib.APGPU_U16, 1, h, w, p, None, None, method, output, ptr, None)
    assert call(pat(0, 1, 2, 3)) == _lib.E_INVAL and b'Bayer arrangement' in lib.apgpu_last_error()
    assert call(pat(0, 1, 3, 5)) == _lib.E_INVAL
    assert call(pat(0, 1, 3, 2), h=1) == _lib.E_INVAL
    assert call(pat(0, 1, 3, 2), h=3, method=2) == _lib.E_INVAL and b'SUPERPIXEL' in lib.apgpu_last_error()
    assert call(pat(0, 1, 3, 2), method=3) == _lib.E_INVAL
    assert call(pat(0, 1, 3, 2), output=4) == _lib.E_INVAL
    black = (C.c_float * 4)(1.5, 0, 0, 0)
    assert lib.apgpu_bayer_demosaic(ptr, _lib.APGPU_U16, 1, 4, 4, pat(0, 1, 3, 2), black, None, 1, 0, ptr, None) == _lib.E_INVAL
    rect = (C.c_int64 * 4)(0, 3, 0, 3)
    assert lib.apgpu_bayer_channel_sums(ptr, _lib.APGPU_U16, 4, 4, pat(1, 0, 3, 2), None, rect, ptr, ptr, None) == _lib.E_INVAL
    assert lib.apgpu_bayer_channel_sums(ptr, _lib.APGPU_U16, 4, 4, pat(0, 1, 3, 2), None, None, ptr, ptr, None) == _lib.E_INVAL


def test_ap_debayer_flags():
    from astrophotography_amd.scripts import ap_debayer as s
    p = s.command_line_opts(['in.fits', 'out'])
    assert (p.infile, p.out_root, p.method, p.whitebalance, p.keepblack, p.pattern, p.black, p.grey, p.luminance, p.loglevel) == \
        ('in.fits', 'out', 'mhc', 'auto', False, None, None, None, 'linear', 'INFO')
    p = s.command_line_opts(['in.fits', 'out', '-m', 'bilinear', '-w', 'region[1, 2, 3, 4]', '--keepblack', '--pattern', 'grbg',
                             '--black', '256', '255', '257', '256', '--grey', 'lum.fits', '--luminance', 'direct', '-l', 'DEBUG'])
    assert (p.method, p.whitebalance, p.keepblack, p.pattern, p.black, p.grey, p.luminance, p.loglevel) == \
        ('bilinear', 'region[1, 2, 3, 4]', True, 'GRBG', [256.0, 255.0, 257.0, 256.0], 'lum.fits', 'direct', 'DEBUG')
    p = s.command_line_opts(['in.fits', 'out', '--method', 'superpixel', '--whitebalance', 'user[2, 1, 1.5, 1]', '--loglevel', 'INFO'])
    assert p.method == 'superpixel' and p.whitebalance == 'user[2, 1, 1.5, 1]'
    with pytest.raises(SystemExit):
        s.command_line_opts(['in.fits', 'out', '--pattern', 'RGBG'])
    with pytest.raises(SystemExit):
        s.command_line_opts(['in.fits'])


def test_bindings_hold_the_new_entry_points():
    from astrophotography_amd import _lib
    assert 'apgpu_bayer_demosaic' in _lib.SIGNATURES and 'apgpu_bayer_channel_sums' in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, 'apgpu_bayer_demosaic') and hasattr(lib, 'apgpu_bayer_channel_sums')
