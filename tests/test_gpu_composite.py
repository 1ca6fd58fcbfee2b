"""F9 ApComposite on the GPU (csrc/composite.hip) against the NumPy model tests/composite_model.py (PARITY UNPINNED:
STIFF is absent): the quantile levels bit for bit, the composite exactly equal in every component, and the files ApComposite and
ap_composite write."""
import os

import numpy as np
import pytest

from tests import composite_model as cm

pytestmark = pytest.mark.gpu

SCRIPT_GRID = [(gf, cs) for gf in (1.0, 1.2, 1.4) for cs in (1.0, 1.5, 2.0)]
Q = [[0.60, 0.999], [0.25, 0.75], [0.0, 1.0]]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()


def _check_levels(planes, q=Q, manual=None):
    from astrophotography_amd import ops
    levels, n = ops.quantile_levels(_dev(planes), q, manual)
    want, want_n = cm.quantile_levels(planes, q, manual)
    got = levels.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    assert np.array_equal(n.cpu().numpy(), want_n)
    return got


# -- levels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (3, 4), (67, 259), (128, 1024)])
def test_levels_bit_equal_on_shapes(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    _check_levels(rng.normal(100.0, 30.0, (3,) + shape).astype(np.float32))
    _check_levels((np.round(rng.normal(10.0, 2.0, (3,) + shape) * 8) / 8).astype(np.float32), [[0.5, 0.5]] * 3)


def test_levels_ties_across_a_digit_boundary():
    rng = np.random.default_rng(4)
    planes = rng.normal(0.0, 1.0, (3, 67, 259)).astype(np.float32)
    # 90 % of a channel is one value; the rest lies on both sides of it, among it keys that differ only in the last digit
    for c, v in enumerate((np.float32(1.0), np.float32(-2.5), np.float32(256.0))):
        flat = planes[c].ravel()
        flat[rng.random(flat.size) < 0.9] = v
        flat[:40] = np.nextafter(v, np.float32(np.inf))
        flat[40:80] = np.nextafter(v, np.float32(-np.inf))
    for q in ([[0.04, 0.96]] * 3, [[0.5, 0.951]] * 3, [[0.0499, 0.0501]] * 3, [[0.0, 1.0]] * 3):
        _check_levels(planes, q)


def test_levels_special_values_and_manual():
    rng = np.random.default_rng(6)
    planes = rng.normal(0.0, 1.0, (3, 33, 47)).astype(np.float32)
    planes[:, ::2, ::3] = 0.0
    planes[:, 1::2, ::3] = -0.0
    planes[0, :, 1::5] = np.float32(1e-41)                       # subnormals
    planes[0, :, 2::5] = np.float32(-3e-42)
    planes[1, 3] = np.nan
    planes[1, 4, ::2] = np.inf
    planes[2, 5, ::2] = -np.inf
    for q in (Q, [[0.3, 0.4]] * 3, [[0.45, 0.55]] * 3):
        _check_levels(planes, q)
    zeros = np.zeros((3, 4, 6), np.float32)
    zeros[:, :2] = -0.0
    got = _check_levels(zeros, [[0.0, 1.0]] * 3)
    assert np.signbit(got[:, 0]).all() and not np.signbit(got[:, 1]).any()
    planes[1] = np.nan                                          # an all-NaN channel
    got = _check_levels(planes)
    assert np.isnan(got[1]).all()
    manual = np.full((3, 2), np.nan, np.float32)
    manual[0, 1] = 4.5
    got = _check_levels(planes, Q, manual)
    assert got[0, 1] == np.float32(4.5)
    manual[1, 0] = -1.0                                         # a manual level on the channel without finite values
    _check_levels(planes, Q, manual)


# -- composite ------------------------------------------------------------------------------------------------------
def _tables(grid):
    return np.stack([cm.tone_table(2.2, gf) for gf, _ in grid])


def _check_composite(planes, levels, grid, bits, flip):
    from astrophotography_amd import ops
    tables, sat = _tables(grid), [cs for _, cs in grid]
    out = ops.composite_rgb(_dev(planes), _dev(np.asarray(levels, np.float32)), tables, sat, bits=bits, flip=flip)
    got = _host(out)
    want = cm.composite_rgb(planes, levels, tables, sat, bits=bits, flip=flip)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), 'differing components: %d of %d' % ((got != want).sum(), got.size)
    return got


def _field(shape, seed):
    """A star field with every special pixel of the composite in it (where the shape has room)."""
    H, W = shape
    planes = cm.star_field(shape, seed, n_stars=max(2, H * W // 300))
    levels, _ = cm.quantile_levels(planes, [[0.60, 0.999]] * 3)
    flat = planes.reshape(3, -1)
    n = flat.shape[1]
    lo = levels[:, 0]
    special = [(0, (np.nan, None, None)), (1, (None, np.inf, None)), (2, (None, None, -np.inf)),
               (3, (1e9, 1e9, 1e9)),                                                 # far above hi: Y > 1
               (4, tuple(np.nextafter(l, np.float32(np.inf)) for l in lo)),           # one ulp above lo
               (5, tuple(l + np.float32(abs(l)) * np.float32(2.0 ** -22) for l in lo)),
               (6, (3e38, lo[1], lo[2])), (7, (lo[0], lo[1], lo[2]))]
    for k, vals in special:
        if k < n:
            for c, v in enumerate(vals):
                if v is not None:
                    flat[c, (k * 7) % n] = v
    return planes, levels


@pytest.mark.parametrize('bits', [8, 16])
@pytest.mark.parametrize('width', [1, 2, 3, 4, 5, 63, 64, 65, 259])
def test_composite_equals_model_on_every_alignment(width, bits):
    for height in (1, 67):
        planes, levels = _field((height, width), seed=width * 10 + height)
        for flip in (True, False):
            _check_composite(planes, levels, [(1.0, 1.5)], bits, flip)
    planes, levels = _field((67, width), seed=width)
    _check_composite(planes, levels, SCRIPT_GRID, bits, True)


@pytest.mark.parametrize('bits', [8, 16])
def test_composite_variant_counts_and_saturation(bits):
    planes, levels = _field((67, 65), seed=21)
    grid16 = [(1.0 + 0.05 * i, 0.25 * (i % 9)) for i in range(16)]                  # colour_sat 0 .. 2, V = 16
    got = _check_composite(planes, levels, grid16, bits, True)
    grey = got[[i for i, (_, cs) in enumerate(grid16) if cs == 0.0]]
    assert len(grey) and np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 0], grey[..., 2])
    _check_composite(planes, levels, [(1.4, 2.0)], bits, False)                      # negative c_c clipped
    from astrophotography_amd import ops
    with pytest.raises(ValueError):
        ops.composite_rgb(_dev(planes), _dev(levels), _tables(grid16 + [(1.0, 1.0)]), [1.0] * 17, bits=bits)


@pytest.mark.parametrize('bits', [8, 16])
def test_composite_degenerate_levels_and_tiny_luminance(bits):
    planes, levels = _field((5, 64), seed=8)
    lv = levels.copy()
    lv[0, 1] = lv[0, 0]                                         # hi == lo: the channel contributes nothing
    _check_composite(planes, lv, SCRIPT_GRID[:3], bits, True)
    lv = levels.copy()
    lv[1] = np.nan                                              # NaN levels
    _check_composite(planes, lv, SCRIPT_GRID[:3], bits, True)
    lv[:] = np.nan
    assert not _check_composite(planes, lv, [(1.0, 1.0)], bits, True).any()
    # Y below 2^-40, in the lowest octave and at its upper knots: x = lo + Y (hi - lo) with lo = 0, hi = 1
    Y = np.concatenate([2.0 ** np.arange(-46.0, -36.0, 0.125), [2.0 ** -40, 2.0 ** -40 * (1 + 2.0 ** -23), 2.0 ** -39 * (1 - 2.0 ** -24)],
                        np.linspace(0.0, 1.25, 41)]).astype(np.float32)
    planes = np.stack([Y, Y, Y]).reshape(3, 1, -1)
    _check_composite(planes, [[0, 1]] * 3, SCRIPT_GRID, bits, False)
    _check_composite(planes * np.float32([[[3.0]], [[0.0]], [[0.0]]]), [[0, 1]] * 3, SCRIPT_GRID, bits, False)


def test_composite_rows_longer_than_a_block():
    planes, levels = _field((3, 1029), seed=9)                  # 258 groups of four per row: the workgroup seam inside a row
    _check_composite(planes, levels, [(1.2, 1.5), (1.0, 2.0)], 8, True)
    _check_composite(planes, levels, [(1.2, 1.5)], 16, False)


# -- end to end -----------------------------------------------------------------------------------------------------
def _read_tiff(path, bits):
    import struct
    raw = open(path, 'rb').read()
    off, = struct.unpack_from('<I', raw, 4)
    n, = struct.unpack_from('<H', raw, off)
    tags = {}
    for k in range(n):
        tag, ftype, count, value = struct.unpack_from('<HHII', raw, off + 2 + 12 * k)
        tags[tag] = (ftype, count, value, off + 2 + 12 * k + 8)
    W, H = tags[256][2], tags[257][2]
    nstrips = tags[273][1]
    offs = [tags[273][2]] if nstrips == 1 else struct.unpack_from('<%dI' % nstrips, raw, tags[273][2])
    return np.frombuffer(raw, '<u%d' % (bits // 8), count=H * W * 3, offset=offs[0]).reshape(H, W, 3)


@pytest.fixture(scope='module')
def fits_triplet(tmp_path_factory):
    from astrophotography_amd import fitsio
    d = tmp_path_factory.mktemp('composite')
    planes = np.stack([cm.star_field((70, 90), seed=31, dither=(0.3 * c, -0.2 * c))[c] for c in range(3)])
    for c, f in enumerate(('Red', 'Green', 'Blue')):
        fitsio.write(str(d / ('m42_%s_90x70_resamp.fits' % f)), planes[c], None)
    return d, planes


def test_composite_files_and_ap_composite(fits_triplet, monkeypatch):
    import astrophotography_amd as ap
    from astrophotography_amd.scripts import ap_composite
    d, planes = fits_triplet
    monkeypatch.chdir(d)
    levels, _ = cm.quantile_levels(planes, [[0.60, 0.999]] * 3)
    want = cm.composite_rgb(planes, levels, _tables(SCRIPT_GRID), [cs for _, cs in SCRIPT_GRID], bits=8, flip=True)
    files = ['m42_%s_90x70_resamp.fits' % f for f in ('Red', 'Green', 'Blue')]
    comp = ap.ApComposite('CRITICAL')
    written = comp.composite_files(files[0], files[1], files[2], 'one16.tiff', gamma_fac=1.2, colour_sat=1.5, bits=16)
    assert written == ['one16.tiff']
    want16 = cm.composite_rgb(planes, levels, _tables([(1.2, 1.5)]), [1.5], bits=16, flip=True)[0]
    assert np.array_equal(_read_tiff('one16.tiff', 16), want16)
    with pytest.raises(ValueError):
        comp.composite_files(files[0], files[1], files[2], ['a.tiff'], gamma_fac=[1.0, 1.2])
    # the composite_all.sh form: nine files with the script's names
    assert ap_composite.main(['m42', '90x70_resamp.fits', 'rgb', '-l', 'CRITICAL', '--copyright', 'nobody']) == 0
    names = ['m42_RedGreenBlue_90x70_resamp_gf%s_cs%s_b8.tiff' % (g, c) for g in ('10', '12', '14') for c in ('10', '15', '20')]
    assert sorted(f for f in os.listdir(d) if f.endswith('b8.tiff')) == sorted(names)
    for v, name in enumerate(names):
        assert np.array_equal(_read_tiff(name, 8), want[v]), name
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(names[4]) as im:
            assert np.array_equal(np.asarray(im), want[4])
    # the explicit form gives the same bytes as the matching variant
    assert ap_composite.main(['--red', files[0], '--green', files[1], '--blue', files[2], '-o', 'explicit.tiff', '--gamma_fac', '1.2',
                              '--colour_sat', '1.5', '--description', 'm42', '--copyright', 'nobody', '-l', 'CRITICAL']) == 0
    assert open('explicit.tiff', 'rb').read() == open(names[4], 'rb').read()
    # shapes must agree
    from astrophotography_amd import fitsio
    fitsio.write('m42_Blue_other.fits', planes[2][:, :80], None)
    with pytest.raises(RuntimeError):
        comp.composite([files[0], files[1], 'm42_Blue_other.fits'])
