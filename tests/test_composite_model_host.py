"""CPU tests of the colour composite's host side (F9 ApComposite): the NumPy model against np.quantile and against
a direct float64 evaluation with pow, the product's tone table against the model's, the TIFF writer against PIL and the TIFF
6.0 structure, and ap_composite's arguments, file names and exit status.  No device."""
import os
import struct

import numpy as np
import pytest

from tests import composite_model as cm

SCRIPT_GRID = [(gf, cs) for gf in (1.0, 1.2, 1.4) for cs in (1.0, 1.5, 2.0)]


# -- levels ---------------------------------------------------------------------------------------------------------
def _level_cases():
    rng = np.random.default_rng(11)
    ties = (np.round(rng.normal(100.0, 3.0, (3, 40, 50)) * 8) / 8).astype(np.float32)
    signed = rng.normal(0.0, 1.0, (3, 30, 31)).astype(np.float32)
    signed[:, ::3, ::4] = 0.0
    signed[:, 1::3, ::4] = -0.0
    holes = rng.normal(5.0, 2.0, (3, 17, 19)).astype(np.float32)
    holes[0, ::2] = np.nan
    holes[1, :, ::3] = np.inf
    holes[2, 3] = -np.inf
    one = np.full((3, 1, 1), 7.5, np.float32)
    return {'ties': ties, 'signed': signed, 'holes': holes, 'one': one}


@pytest.mark.parametrize('name', ['ties', 'signed', 'holes', 'one'])
def test_model_levels_are_numpy_lower_quantiles(name):
    planes = _level_cases()[name]
    for qlo, qhi in ((0.60, 0.999), (0.0, 1.0), (0.5, 0.5), (0.123456, 0.987654)):
        levels, n = cm.quantile_levels(planes, [[qlo, qhi]] * 3)
        for c in range(3):
            v = planes[c][np.isfinite(planes[c])]
            assert n[c] == v.size
            want = np.quantile(v, [qlo, qhi], method='lower')
            assert levels.dtype == np.float32 and np.array_equal(levels[c], want.astype(np.float32)), (name, c, qlo, qhi)


def test_model_levels_edge_cases():
    planes = _level_cases()['signed'].copy()
    planes[1] = np.nan                                          # an all-NaN channel
    levels, n = cm.quantile_levels(planes, [[0.6, 0.999]] * 3)
    assert n[1] == 0 and np.isnan(levels[1]).all() and np.isfinite(levels[[0, 2]]).all()
    # -0.0 and +0.0 are distinct keys: the zeros of a channel sort with the negative ones first
    z = np.zeros((3, 1, 4), np.float32)
    z[:, 0, :2] = -0.0
    levels, _ = cm.quantile_levels(z, [[0.0, 1.0]] * 3)
    assert np.signbit(levels[:, 0]).all() and not np.signbit(levels[:, 1]).any()
    # manual overrides exactly the entries that are not NaN
    manual = np.full((3, 2), np.nan, np.float32)
    manual[2, 1] = 123.25
    base, _ = cm.quantile_levels(_level_cases()['ties'], [[0.6, 0.999]] * 3)
    got, _ = cm.quantile_levels(_level_cases()['ties'], [[0.6, 0.999]] * 3, manual)
    assert got[2, 1] == np.float32(123.25)
    got[2, 1] = base[2, 1]
    assert np.array_equal(got, base)


# -- tone table and composite ---------------------------------------------------------------------------------------
def test_product_tone_table_is_the_models():
    from astrophotography_amd import ops
    for gf in (1.0, 1.2, 1.4):
        t = ops.tone_table(2.2, gf)
        assert t.dtype == np.float32 and t.shape == (cm.TABLE_LEN,) == (10241,)
        assert np.array_equal(t.view(np.uint32), cm.tone_table(2.2, gf).view(np.uint32))
    assert ops.tone_table(2.2, 1.0)[-1] == 1.0
    with pytest.raises(ValueError):
        ops.tone_table(2.2, 1.0, gamma_type='REC.709')
    with pytest.raises(ValueError):
        ops.tone_table(0.0, 1.0)


def test_table_lookup_limits():
    t = cm.tone_table(2.2, 1.0)
    Y = np.array([0.0, 2.0 ** -41, np.nextafter(np.float32(2.0 ** -40), np.float32(0)), 2.0 ** -40, 0.25, 1.0, 1.5, np.inf], np.float32)
    G = cm.table_lookup(t, Y)
    assert np.array_equal(G[:3], [0, 0, 0]) and G[3] == t[0] and G[4] == t[38 * 256] and np.array_equal(G[5:], [1, 1, 1])
    # between knots: linear interpolation of G = Y^a (a = 1 / gamma - 1) over cells of relative width h = 2^-8 is off by at most
    # h^2 / 8 |a (a - 1)| relative (the second derivative, largest at the low end of a cell); the knots and the three float32
    # operations add a rounding each.  At gamma 2.2 that is 1.6e-6 + 2.4e-7: 0.12 count at 16 bits.
    a = 1 / 2.2 - 1
    bound = (2.0 ** -8) ** 2 / 8 * abs(a * (a - 1)) + 4 * 2.0 ** -24
    Yr = np.random.default_rng(2).uniform(2.0 ** -30, 1.0, 20000).astype(np.float32)
    rel = np.abs(cm.table_lookup(t, Yr).astype(np.float64) / (Yr.astype(np.float64) ** a) - 1)
    print('largest relative error of the table %.3g (bound %.3g)' % (rel.max(), bound))
    assert rel.max() <= bound


@pytest.mark.parametrize('bits', [8, 16])
def test_model_is_within_one_count_of_the_direct_float64_evaluation(bits):
    planes = cm.star_field((96, 128), seed=5)
    levels, _ = cm.quantile_levels(planes, [[0.60, 0.999]] * 3)
    tables = np.stack([cm.tone_table(2.2, gf) for gf, _ in SCRIPT_GRID])
    got = cm.composite_rgb(planes, levels, tables, [cs for _, cs in SCRIPT_GRID], bits=bits)
    assert got.shape == (9, 96, 128, 3) and got.max() == 2 ** bits - 1 and got.min() == 0
    differing = 0
    for v, (gf, cs) in enumerate(SCRIPT_GRID):
        want = cm.composite_direct(planes, levels, 2.2, gf, cs, bits=bits)
        d = np.abs(got[v].astype(np.int64) - want)
        assert d.max() <= 1, (gf, cs, int(d.max()))
        differing += int((d != 0).sum())
    print('bits %d: %.4f %% of the components differ by one count' % (bits, 100.0 * differing / got.size))


def test_model_flip_black_and_grey():
    planes = cm.star_field((9, 7), seed=3)
    planes[1, 2, 3] = np.nan
    planes[2, 5, 1] = np.inf
    levels, _ = cm.quantile_levels(planes, [[0.2, 0.95]] * 3)
    t = cm.tone_table(2.2, 1.0)[None]
    up = cm.composite_rgb(planes, levels, t, [1.0], flip=True)[0]
    down = cm.composite_rgb(planes, levels, t, [1.0], flip=False)[0]
    assert np.array_equal(up, down[::-1])
    assert not down[2, 3].any() and not down[5, 1].any() and down.any()
    grey = cm.composite_rgb(planes, levels, t, [0.0])[0]
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 0], grey[..., 2])


# -- TIFF -----------------------------------------------------------------------------------------------------------
def _ifd(raw):
    assert raw[:4] == b'II*\0'
    off, = struct.unpack_from('<I', raw, 4)
    n, = struct.unpack_from('<H', raw, off)
    tags = {}
    for k in range(n):
        tag, ftype, count, value = struct.unpack_from('<HHI4s', raw, off + 2 + 12 * k)
        size = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8}[ftype] * count
        data = value[:size] if size <= 4 else raw[struct.unpack('<I', value)[0]:][:size]
        if ftype == 2:
            tags[tag] = data
        elif ftype == 5:
            tags[tag] = struct.unpack('<%dI' % (2 * count), data)
        else:
            tags[tag] = struct.unpack('<%d%s' % (count, {1: 'B', 3: 'H', 4: 'I'}[ftype]), data)
    assert struct.unpack_from('<I', raw, off + 2 + 12 * n)[0] == 0          # one IFD
    return tags, [struct.unpack_from('<H', raw, off + 2 + 12 * k)[0] for k in range(n)]


@pytest.mark.parametrize('bits', [8, 16])
@pytest.mark.parametrize('width', [1, 3, 640])
def test_tiff_files_open_with_pil_and_hold_the_tags(tmp_path, bits, width):
    Image = pytest.importorskip('PIL.Image')
    from astrophotography_amd import tiffio
    rng = np.random.default_rng(width + bits)
    height = 600 if width == 640 else 5                         # 640 x 600: more than one strip
    img = rng.integers(0, 2 ** bits, (height, width, 3)).astype(np.uint8 if bits == 8 else np.uint16)
    path = str(tmp_path / 'a.tiff')
    tiffio.write(path, img, description='n6888', copyright='A. N. Observer')
    raw = open(path, 'rb').read()
    tags, order = _ifd(raw)
    assert order == sorted(order)                                # TIFF 6.0: entries in ascending tag order
    assert tags[256] == (width,) and tags[257] == (height,) and tags[258] == (bits,) * 3
    assert tags[259] == (1,) and tags[262] == (2,) and tags[277] == (3,) and tags[284] == (1,) and tags[274] == (1,)
    assert tags[270] == b'n6888\0' and tags[33432] == b'A. N. Observer\0' and tags[305] == tiffio.SOFTWARE.encode() + b'\0'
    assert tags[282] == (72, 1) and tags[283] == (72, 1) and tags[296] == (2,)
    rows, offs, counts = tags[278][0], tags[273], tags[279]
    assert len(offs) == len(counts) == -(-height // rows) and sum(counts) == img.nbytes == len(raw) - offs[0]
    if width == 640:
        assert len(offs) > 1
    data = b''.join(raw[o:o + c] for o, c in zip(offs, counts))
    assert np.array_equal(np.frombuffer(data, '<u%d' % (bits // 8)).reshape(img.shape), img)
    if bits == 8:                                               # (PIL has no 16-bit RGB mode: the strips above are the check)
        with Image.open(path) as im:
            assert im.mode == 'RGB' and im.size == (width, height)
            assert np.array_equal(np.asarray(im), img)
    else:
        with Image.open(path) as im:                            # it still parses the directory
            assert im.size == (width, height) and im.tag_v2[258] == (16, 16, 16)


def test_tiff_refuses_what_it_cannot_hold(tmp_path):
    from astrophotography_amd import tiffio
    with pytest.raises(ValueError, match='4 GiB'):
        tiffio.layout(40000, 40000, 8)
    with pytest.raises(ValueError, match='4 GiB'):
        tiffio.layout(27000, 27000, 16)
    tiffio.layout(30000, 30000, 8)                              # 2.7 GB: fine
    with pytest.raises(ValueError):
        tiffio.layout(4, 4, 12)
    with pytest.raises(ValueError):
        tiffio.write(str(tmp_path / 'x.tiff'), np.zeros((4, 4), np.uint8))


# -- ap_composite ---------------------------------------------------------------------------------------------------
def test_ap_composite_arguments_and_names():
    from astrophotography_amd.scripts import ap_composite as s
    p = s.command_line_opts(['n6888', '2560x1920_resamp.fits', 'sho', 'rgb'])
    assert p.form == 'script' and (p.prefix, p.suffix, p.selections) == ('n6888', '2560x1920_resamp.fits', ['sho', 'rgb'])
    assert p.bits == 8 and p.gamma == 2.2 and p.min_level == [0.60] and p.max_level == [0.999] and not p.no_flip
    assert p.min_type == ['QUANTILE'] * 3 and p.gamma_fac is None and p.colour_sat is None
    assert s.input_names('n6888', '2560x1920_resamp.fits', 'sho') == ['n6888_SII_2560x1920_resamp.fits', 'n6888_Ha_2560x1920_resamp.fits',
                                                                     'n6888_OIII_2560x1920_resamp.fits']
    assert s.input_names('m', 's.fits', 'rgb') == ['m_Red_s.fits', 'm_Green_s.fits', 'm_Blue_s.fits']
    assert s.input_names('m', 's.fits', 'hgb') == ['m_Ha_s.fits', 'm_Green_s.fits', 'm_Blue_s.fits']
    assert s.output_name('n6888', '2560x1920_resamp.fits', 'sho', 1.2, 1.5, 8) == 'n6888_SIIHaOIII_2560x1920_resamp_gf12_cs15_b8.tiff'
    assert s.output_name('m', 'a.b.fits', 'rgb', 1.0, 2.0, 16) == 'm_RedGreenBlue_a.b_gf10_cs20_b16.tiff'
    names = [s.output_name('m', 's.fits', 'rgb', g, c, 8) for g, c in SCRIPT_GRID]
    assert len(set(names)) == 9 and names[0].endswith('gf10_cs10_b8.tiff') and names[-1].endswith('gf14_cs20_b8.tiff')
    q = s.command_line_opts(['--red', 'r.fits', '--green', 'g.fits', '--blue', 'b.fits', '-o', 'o.tiff', '--gamma_fac', '1.2',
                             '--gamma_fac', '1.4', '--colour_sat', '2', '--min_level', '0.1,0.2,0.3', '--min_type', 'manual',
                             '--max_type', 'QUANTILE,MANUAL,QUANTILE', '--bits', '16', '--no_flip'])
    assert q.form == 'files' and (q.red, q.green, q.blue, q.output) == ('r.fits', 'g.fits', 'b.fits', 'o.tiff')
    assert q.gamma_fac == [1.2, 1.4] and q.colour_sat == [2.0] and q.min_level == [0.1, 0.2, 0.3] and q.min_type == ['MANUAL'] * 3
    assert q.max_type == ['QUANTILE', 'MANUAL', 'QUANTILE'] and q.bits == 16 and q.no_flip
    assert s.variant_outputs('o.tiff', [(1.2, 2.0)], 16) == ['o.tiff']
    assert s.variant_outputs('d/o.tiff', [(1.2, 2.0), (1.4, 2.0)], 16) == ['d/o_gf12_cs20_b16.tiff', 'd/o_gf14_cs20_b16.tiff']
    for bad in (['n6888', 'suffix.fits'], ['--red', 'r.fits', '-o', 'o.tiff'], ['p', 's', 'rgb', '--red', 'r.fits'],
                ['p', 's', 'rgb', '--bits', '12'], ['p', 's', 'rgb', '--min_type', 'GREYLEVEL']):
        with pytest.raises(SystemExit) as e:
            s.command_line_opts(bad)
        assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        s.command_line_opts(['--help'])
    assert e.value.code == 0


def test_ap_composite_missing_files_exit_status(tmp_path, monkeypatch, capsys):
    from astrophotography_amd.scripts import ap_composite as s
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'm_Red_s.fits').write_bytes(b'')
    assert s.main(['m', 's.fits', 'rgb']) == 8
    out = capsys.readouterr().out
    assert 'm_Green_s.fits' in out and 'm_Blue_s.fits' in out and 'm_Red_s.fits' not in out and 'missing 2 required files' in out
    assert s.main(['m', 's.fits', 'xyz']) == 4
    assert not [f for f in os.listdir(tmp_path) if f.endswith('.tiff')]


def test_variant_grid_and_level_arguments():
    from astrophotography_amd.core import ApComposite as A
    assert A.variant_grid([1.0, 1.2, 1.4], [1.0, 1.5, 2.0]) == SCRIPT_GRID
    assert A.variant_grid(1.2, 1.5) == [(1.2, 1.5)]
    assert A._three_types('manual', 'min_type') == ['MANUAL'] * 3
    with pytest.raises(ValueError):
        A._three_types('GREYLEVEL', 'min_type')
    with pytest.raises(ValueError):
        A._three([1, 2], 'min_level')
    with pytest.raises(ValueError):
        A.ApComposite('NOT_A_LEVEL')
