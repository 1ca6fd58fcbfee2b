"""CPU-only tests: the C ABI exports what include/apgpu.h declares, the FITS module reads/writes what
astropy wrote, host-side logic of the Ap* shells, the scripts' flags and the sharding helpers."""
import os
import re
import shutil

import numpy as np
import pytest

from tests.util import GOLDEN, load_golden

ROOT = os.path.dirname(GOLDEN.rstrip('/')).rsplit('/tests', 1)[0]


def test_capi_exports_every_declared_symbol():
    from astrophotography_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'apgpu.h')).read()
    declared = set(re.findall(r'\b(apgpu_[a-z0-9_]+)\s*\(', hdr))
    declared.discard('apgpu_stack_args')
    declared.discard('apgpu_stack_ws_stats')
    assert len(declared) >= 15
    lib = _lib.load()                          # loads without a GPU; no compute call is made
    for name in sorted(declared):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, 'binding missing for ' + name
    assert set(_lib.SIGNATURES) == declared
    assert lib.apgpu_version() == 130
    assert lib.apgpu_last_error() is not None
    # argument validation happens before any device work
    assert lib.apgpu_calibrate(None, 0, None, None, None, None, None, 0, None, 1, 1, None) == _lib.E_INVAL
    assert b'NULL' in lib.apgpu_last_error()
    assert lib.apgpu_stack_sigclip(None, None) == _lib.E_INVAL
    assert lib.apgpu_flat_normalize_ws_bytes(4096 * 4096) >= 4 * 2048 + 16
    assert lib.apgpu_sigclip_global_ws_bytes(1000) >= 8000


def test_stack_args_struct_matches_header():
    import ctypes as C
    from astrophotography_amd._lib import StackArgs
    hdr = open(os.path.join(ROOT, 'include', 'apgpu.h')).read()
    body = hdr[hdr.index('typedef struct apgpu_stack_args {'):hdr.index('} apgpu_stack_args;')]
    fields = re.findall(r'^\s+(?:const\s+)?[a-z0-9_]+\s*\*?\s*\*?([a-z_0-9]+);', body, re.M)
    assert fields == [f[0] for f in StackArgs._fields_]
    assert C.sizeof(StackArgs) == 192
    # the workspace of the two-kernel scheme: about 4 bytes per pixel, a zero prefix of counters + tile flags, statistics inside it
    from astrophotography_amd import _lib
    lib = _lib.load()
    zero = C.c_size_t(0)
    nb = lib.apgpu_stack_ws_bytes(4096 * 4096, C.byref(zero))
    assert 4 * 4096 * 4096 < nb < 4.2 * 4096 * 4096 and nb % 4 == 0
    assert _lib.STACK_WS_STATS_OFFSET + 32 <= zero.value < nb and zero.value >= 16384 + 64 + 4 * (4096 * 4096 // 256)
    assert re.search(r'#define APGPU_STACK_WS_STATS_OFFSET %d\b' % _lib.STACK_WS_STATS_OFFSET, hdr)
    assert lib.apgpu_stack_ws_bytes(0, None) == 0


def test_fitsio_reads_and_rewrites_astropy_files(tmp_path):
    from astrophotography_amd import fitsio
    g = load_golden('g1_calibrate.npz')
    raw, h = fitsio.read(os.path.join(GOLDEN, 'g1_c0_raw.fits'))
    assert raw.dtype == np.uint16 and np.array_equal(raw, g['raw_u16_64x64'])
    assert h['BZERO'] == 32768 and h['EXPTIME'] == 120.0 and h['NAXIS1'] == 64
    for name, key in (('bias', 'bias_64x64'), ('dark', 'dark_64x64'), ('flat', 'flat_64x64')):
        d, _ = fitsio.read(os.path.join(GOLDEN, f'g1_c0_{name}.fits'))
        assert d.dtype == np.float32 and np.array_equal(d, g[key])
    cal, hc = fitsio.read(os.path.join(GOLDEN, 'g1_c0_cal.fits'))
    assert np.array_equal(cal, g['c0_out'].astype(np.float32))
    assert hc['BIASCORR'] is True and hc['BIASFILE'] == 'bias.fits' and hc['BUNIT'] == 'adu'
    assert hc.comment('DARKCORR') == 'True if scaled dark subtracted.'
    assert hc.history()[0].startswith('Processed by ApCalibrate 0.5.1')
    # byte-identical rewrite of both files
    for fn, data, hh in (('g1_c0_raw.fits', raw, h), ('g1_c0_cal.fits', cal, hc)):
        out = tmp_path / fn
        fitsio.write(str(out), data, hh)
        assert out.read_bytes() == open(os.path.join(GOLDEN, fn), 'rb').read()
    # header edits: update, append, delete, history, long strings, numbers
    hh = hc.copy()
    hh['BUNIT'] = ('electrons', 'Pixel value units')
    hh['NEWKEY'] = (3, 'an int')
    hh['FLT'] = 0.5
    del hh['FLATFILE']
    hh['HISTORY'] = 'second history line'
    out = tmp_path / 'edit.fits'
    fitsio.write(str(out), cal.astype(np.float64), hh)
    d2, h2 = fitsio.read(str(out))
    assert d2.dtype == np.float64 and h2['BITPIX'] == -64
    assert h2['BUNIT'] == 'electrons' and h2['NEWKEY'] == 3 and h2['FLT'] == 0.5 and 'FLATFILE' not in h2
    assert len(h2.history()) == 2
    assert len(out.read_bytes()) % 2880 == 0
    # uint8 mask round trip, no BZERO
    m = (np.arange(35).reshape(5, 7) % 4).astype(np.uint8)
    fitsio.write(str(tmp_path / 'm.fits'), m, None)
    m2, hm = fitsio.read(str(tmp_path / 'm.fits'))
    assert m2.dtype == np.uint8 and np.array_equal(m, m2) and 'BZERO' not in hm
    with pytest.raises(OSError):
        (tmp_path / 'bad.fits').write_bytes(b'not a fits file' * 300)
        fitsio.read(str(tmp_path / 'bad.fits'))


def test_fitsio_image_extensions(tmp_path):
    """Primary + IMAGE extensions (the CCDData layout ApMasterCal writes: MASK uint8, UNCERT float64)."""
    from astrophotography_amd import fitsio
    rng = np.random.default_rng(5)
    prim = rng.normal(size=(7, 9))
    mask = (rng.random((7, 9)) > 0.8).astype(np.uint8)
    unc = rng.random((7, 9))
    h = fitsio.Header()
    h['BUNIT'] = 'adu'
    out = tmp_path / 'ccd.fits'
    fitsio.write(str(out), prim, h, extensions=[('MASK', mask, None), ('UNCERT', unc, {'UTYPE': ('StdDevUncertainty', '')})])
    assert out.stat().st_size % 2880 == 0
    d, hh = fitsio.read(str(out))
    assert hh['EXTEND'] is True and hh['BITPIX'] == -64 and np.array_equal(d, prim)
    m, mh = fitsio.read_extension(str(out), 'mask')
    assert mh['XTENSION'].strip() == 'IMAGE' and mh['PCOUNT'] == 0 and mh['GCOUNT'] == 1 and mh['BITPIX'] == 8
    assert m.dtype == np.uint8 and np.array_equal(m, mask)
    u, uh = fitsio.read_extension(str(out), 'UNCERT')
    assert uh['UTYPE'] == 'StdDevUncertainty' and np.array_equal(u, unc)
    with pytest.raises(KeyError):
        fitsio.read_extension(str(out), 'NOPE')
    # rewriting the primary with the header it was read with keeps the extensions byte for byte
    fitsio.write(str(tmp_path / 'again.fits'), d, hh)
    assert (tmp_path / 'again.fits').read_bytes() == out.read_bytes()


def test_fitsio_scaled_integers(tmp_path):
    from astrophotography_amd import fitsio
    h = fitsio.Header()
    h['XSCALE'] = 2.0
    h['XZERO'] = 10.0
    # a scaled int16 file: written plain, then the two placeholder cards are renamed in the file image
    data = np.array([[1, -2], [300, 4]], np.int16)
    fitsio.write(str(tmp_path / 's.fits'), data, h)
    raw = (tmp_path / 's.fits').read_bytes().replace(b'XSCALE  =', b'BSCALE  =').replace(b'XZERO   =', b'BZERO   =')
    (tmp_path / 's.fits').write_bytes(raw)
    d, hh = fitsio.read(str(tmp_path / 's.fits'))
    assert hh['BSCALE'] == 2.0
    assert d.dtype == np.float32 and np.array_equal(d, data.astype(np.float32) * 2 + 10)
    # the scaling keywords describe the source file's storage: physical values written back must not inherit them
    fitsio.write(str(tmp_path / 't.fits'), d, hh)
    d2, h2 = fitsio.read(str(tmp_path / 't.fits'))
    assert 'BSCALE' not in h2 and 'BZERO' not in h2 and np.array_equal(d2, d)
    # int16 data with a header read from a uint16 file: BZERO = 32768 must not survive (it would shift the data)
    u, hu = fitsio.read(os.path.join(GOLDEN, 'g1_c0_raw.fits'))
    assert hu['BZERO'] == 32768
    i16 = (u[:4, :4].astype(np.int32) - 1000).astype(np.int16)
    fitsio.write(str(tmp_path / 'i.fits'), i16, hu)
    d3, h3 = fitsio.read(str(tmp_path / 'i.fits'))
    assert d3.dtype == np.int16 and np.array_equal(d3, i16) and 'BZERO' not in h3


def test_fitsio_long_strings_and_non_ascii(tmp_path):
    """CONTINUE long-string cards (a full path in DATAFILE, core/ApFindBadPixels.py:154) and non-ASCII header bytes."""
    from astrophotography_amd import fitsio
    h = fitsio.Header()
    path = '/data/observatory/' + 'sub/' * 25 + "master_dark_it's-300s.fits"
    h['DATAFILE'] = (path, 'Name of the dark the mask was made from')
    h['NOTE'] = ('25\u00b0C', 'sensor \u00b0')
    fitsio.write(str(tmp_path / 'l.fits'), np.zeros((2, 2), np.uint8), h)
    raw = (tmp_path / 'l.fits').read_bytes()
    assert len(raw) % 2880 == 0 and b"CONTINUE  '" in raw and raw[:2880 * 2].decode('ascii')      # pure ASCII, whole blocks
    for i in range(0, raw.index(b'END' + b' ' * 77), 80):
        card = raw[i:i + 80].decode('ascii')
        if card.startswith(('DATAFILE', 'CONTINUE')):
            assert card.rstrip().count("'") % 2 == 0                                            # every quote is closed
    _, h2 = fitsio.read(str(tmp_path / 'l.fits'))
    assert h2['DATAFILE'] == path and h2.comment('DATAFILE').startswith('Name of the dark')
    assert h2['NOTE'] == '25?C'
    # a stray non-ASCII byte in a file from capture software reads as '?' and the file can be rewritten
    patched = raw.replace(b'25?C', b'25\xb0C')
    (tmp_path / 'n.fits').write_bytes(patched)
    d3, h3 = fitsio.read(str(tmp_path / 'n.fits'))
    assert h3['NOTE'] == '25?C'
    h3['NEWKEY'] = 1
    fitsio.write(str(tmp_path / 'n2.fits'), d3, h3)
    assert fitsio.read(str(tmp_path / 'n2.fits'))[1]['NOTE'] == '25?C'
    # a long string under a HIERARCH keyword: the first piece is shorter than 67 characters, every card stays 80 bytes
    h4 = fitsio.Header()
    h4['LONGKEYWORD1'] = ('x' * 100 + "it's" + 'y' * 80, 'comment')
    fitsio.write(str(tmp_path / 'h.fits'), np.zeros((2, 2), np.uint8), h4)
    assert (tmp_path / 'h.fits').stat().st_size % 2880 == 0
    assert fitsio.read(str(tmp_path / 'h.fits'))[1]['LONGKEYWORD1'] == 'x' * 100 + "it's" + 'y' * 80


def test_user_badpix_yaml_semantics(tmp_path):
    """1-based inclusive -> 0-based half-open, out-of-range entries skipped, slots counted
    (ApFindBadPixels.py:70-158) - host logic only, no device."""
    from astrophotography_amd.core import _common
    from astrophotography_amd.core.ApFindBadPixels import ApFindBadPixels
    obj = ApFindBadPixels.__new__(ApFindBadPixels)
    obj._logger = _common.make_logger('ApFindBadPixels', 'CRITICAL')
    obj._imdata = np.zeros((300, 500), np.float32)
    y = tmp_path / 'u.yml'
    shutil.copy(os.path.join(GOLDEN, 'user_badpixels.yml'), y)
    cols, rows, rects = obj._read_user_badpix(y)
    assert cols == [12, 13, 17] and rows is None and len(rects) == 3
    r, n = obj._rects_from_user(cols, rows, rects)
    assert r == [[0, 300, 11, 12], [0, 300, 12, 13], [0, 300, 16, 17], [0, 1, 0, 1], [4, 6, 6, 12], [199, 300, 399, 420]]
    g = load_golden('g2_findbadpix.npz')
    assert n == int(g['d1_nbad_user'])
    r, n = obj._rects_from_user([0, 501, 500], [301, 1], [[1, 301, 1, 2], [1, 2, 0, 3], [1, 2, 3]])
    assert r == [[0, 300, 499, 500], [0, 1, 0, 500]] and n == 300 + 500
    (tmp_path / 'partial.yml').write_text('bad_rows:\n- 3\n')
    assert obj._read_user_badpix(tmp_path / 'partial.yml') == [None, [3], None]


def test_error_conventions_without_device(tmp_path):
    import astrophotography_amd as ap
    with pytest.raises(ValueError):
        ap.ApImArith('NOT_A_LEVEL')
    ia = ap.ApImArith('CRITICAL')
    with pytest.raises(ValueError):
        ia._sanitize_operation('POW')
    assert ia._sanitize_operation(' sub ') == 'SUB'
    with pytest.raises(RuntimeError):
        ap.ApFixBadPixels('CRITICAL').fix_files(str(tmp_path / 'nope.fits'), str(tmp_path / 'm.fits'), str(tmp_path / 'o.fits'))
    with pytest.raises(RuntimeError):
        ap.ApMasterCal(str(tmp_path / 'missing_dir'), 'master*', 'UNKNOWN', 0.5, 'CRITICAL')
    with pytest.raises(AttributeError):
        ap.NoSuchClass


def test_mastercal_file_checks(tmp_path):
    """Consistency checks and CCD-TEMP filter of ApMasterCal (ap_combine_darks.py:150-287) - headers only."""
    from astrophotography_amd import fitsio
    from astrophotography_amd.core.ApMasterCal import ApMasterCal
    d = tmp_path / 'darks'
    d.mkdir()

    def mk(name, temp=-20.0, exptime=300.0, imagetyp='Dark Frame', shape=(4, 6)):
        h = fitsio.Header()
        for k, v in (('TELESCOP', 'T05'), ('IMAGETYP', imagetyp), ('EXPTIME', exptime), ('SET-TEMP', -20.0),
                     ('CCD-TEMP', temp), ('DATE-OBS', '2020-01-01T00:00:00'), ('FILTER', 'none')):
            h[k] = v
        fitsio.write(str(d / name), np.zeros(shape, np.uint16), h)
    mk('d1.fits'), mk('d2.fit', temp=-19.8), mk('d3.fits', temp=-18.0), mk('master_dark.fits')
    mc = ApMasterCal(str(d), 'master*', 'UNKNOWN', 0.5, 'CRITICAL')
    assert mc._values('file') == ['d1.fits', 'd2.fit']                 # master* excluded, warm frame dropped
    kw = mc._generate_final_keywords()
    assert kw['IMAGETYP'][0] == 'MASTER DARK' and kw['TELESCOP'][0] == 'T05' and kw['IFILE001'] == 'd2.fit'
    assert kw['SET-TEMP'][0] == -20.0
    mk('d4.fits', exptime=60.0)
    with pytest.raises(RuntimeError):
        ApMasterCal(str(d), 'master*', 'UNKNOWN', 0.5, 'CRITICAL')


def test_scripts_keep_the_reference_flags():
    from astrophotography_amd.scripts import ap_calibrate, ap_combine_darks, ap_find_badpix, ap_fix_badpix, ap_imarith, ap_stack
    a = ap_calibrate.command_line_opts(['raw.fits', 'b.fits', 'd.fits', 'out.fits', '--master_flat', 'f.fits',
                                        '--master_badpix', 'm.fits', '--normflat', 'n.fits', '--deltapix', '3',
                                        '--fixcosmic', '--dark_still_biased', '-l', 'DEBUG'])
    assert (a.raw_image, a.master_bias, a.master_dark, a.calibrated_image) == ('raw.fits', 'b.fits', 'd.fits', 'out.fits')
    assert a.deltapix == 3 and a.fixcosmic and a.dark_still_biased and a.loglevel == 'DEBUG' and a.normflat == 'n.fits'
    assert ap_calibrate.command_line_opts(['r', 'b', 'd', 'o']).deltapix == 2
    f = ap_find_badpix.command_line_opts(['dark.fits', 'bp.fits'])
    assert f.sigma == 4.0 and f.user_badpix is None
    assert ap_find_badpix.command_line_opts(['dark.fits', 'bp.fits', '--sigma', '5']).sigma == 5.0
    i = ap_imarith.command_line_opts(['a.fits', 'SUB', '3.5', 'o.fits', '--units', 'adu'])
    assert (i.operation, i.value, i.units) == ('SUB', '3.5', 'adu')
    assert ap_fix_badpix.command_line_opts(['a.fits', 'm.fits', 'o.fits']).deltapix == 2
    c = ap_combine_darks.command_line_opts(['dir', 'master.fits'])
    assert (c.exclude_pattern, c.telescop, c.temptol) == ('master*', 'UNKNOWN', 0.5)
    s = ap_stack.command_line_opts(['o.fits', 'a.fits', 'b.fits', '--method', 'median'])
    assert s.input_images == ['a.fits', 'b.fits'] and s.method == 'median' and s.sigma == 3.0
    from astrophotography_amd.scripts import ap_measure_background
    b = ap_measure_background.command_line_opts(['cal.fits', 'bg.fits'])
    assert (b.nbg_cols, b.nbg_rows, b.min_bgwidth, b.min_bgheight, b.bg_filter_width, b.bg_badbox_pctile, b.bg_sigmaclip, b.srclist) == \
        (16, 16, 48, 48, 3, 25.0, 3.0, None)
    from astrophotography_amd.scripts import ap_fix_cosmic_rays
    cr = ap_fix_cosmic_rays.command_line_opts(['in.fits', 'out.fits', '--crmaskim', 'm.fits'])
    assert (cr.input, cr.output, cr.crmaskim, cr.crdiffim) == ('in.fits', 'out.fits', 'm.fits', None)
    for mod in (ap_calibrate, ap_find_badpix, ap_imarith, ap_fix_badpix, ap_combine_darks, ap_measure_background, ap_fix_cosmic_rays):
        with pytest.raises(SystemExit) as e:
            mod.command_line_opts(['--help'])
        assert e.value.code == 0


def test_background_mesh_host_logic():
    """The mesh-sized host steps of ApMeasureBackground against SciPy / the restatement: box geometry as the reference
    computes it (core/ApMeasureBackground.py:251-329), spline prefilter = scipy.ndimage.spline_filter, 3 x 3 nanmedian,
    inverse-distance fill."""
    from scipy import ndimage
    from astrophotography_amd.core import ApMeasureBackground as M
    from oracle import background_ref as br
    rng = np.random.default_rng(8)
    for shp in ((16, 16), (5, 7), (1, 4), (3, 1), (2, 2), (32, 20)):
        mesh = rng.normal(500, 20, shp)
        np.testing.assert_allclose(M._bspline3_prefilter(mesh), ndimage.spline_filter(mesh, order=3, mode='reflect'), rtol=0, atol=1e-11)
    m = rng.normal(0, 1, (6, 9))
    good = rng.random((6, 9)) > 0.3
    mm = np.where(good, m, np.nan)
    assert np.array_equal(M._nanmedian_filter(mm, 3), br.median_filter_mesh(mm, 3), equal_nan=True)
    assert np.array_equal(M._fill_excluded(mm, good), br.fill_excluded(mm, good))
    obj = M.ApMeasureBackground('CRITICAL')
    obj._set_bgbox_size(4096, 4096, None, None, None, None)
    assert obj._boxsize == (258, 258)                    # 2 * (1 + int(4096 / 32)) = 258, 16 * 258 >= 4096
    obj._set_bgbox_size(600, 760, 8, 8, None, None)
    assert obj._boxsize == (76, 96)
    obj._set_bgbox_size(2672, 4008, 16, 16, 48, 48)
    assert obj._boxsize == (168, 252)


def test_sharding_helpers():
    from astrophotography_amd import parallel
    assert parallel.stripe_rows(4096, 8) == [(i * 512, (i + 1) * 512) for i in range(8)]
    s = parallel.stripe_rows(10, 3)
    assert s == [(0, 4), (4, 7), (7, 10)]
    assert parallel.stripe_rows(2, 8) == [(0, 1), (1, 2)]
    got = [parallel.shard_frames(256, 8, r) for r in range(8)]
    assert got == [(r * 32, (r + 1) * 32) for r in range(8)]
    got = [parallel.shard_frames(10, 4, r) for r in range(4)]
    assert got == [(0, 3), (3, 6), (6, 8), (8, 10)]


def test_tan_wcs_matches_astropy_golden():
    """G10: pixel <-> sky of astrophotography_amd.wcs.TanWcs against astropy.wcs.WCS (CD matrix, CDELT + CROTA2,
    CDELT + PC near the pole)."""
    import json
    from astrophotography_amd.wcs import TanWcs
    g = load_golden('g10_wcs.npz')
    for i in range(int(g['ncases'])):
        w = TanWcs.from_header(json.loads(str(g[f'hdr{i}'])))
        pix, sky = g[f'pix{i}'], g[f'sky{i}']
        ra, dec = w.pix2sky(pix[:, 0], pix[:, 1])
        dra = (ra - sky[:, 0] + 180.0) % 360.0 - 180.0
        assert np.abs(dra * np.cos(np.deg2rad(dec))).max() < 1e-11 and np.abs(dec - sky[:, 1]).max() < 1e-11
        x, y = w.sky2pix(sky[:, 0], sky[:, 1])
        assert np.abs(x - pix[:, 0]).max() < 1e-8 and np.abs(y - pix[:, 1]).max() < 1e-8
    with pytest.raises(ValueError):
        TanWcs.from_header({'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN'})
    with pytest.raises(ValueError):
        TanWcs.from_header(dict(json.loads(str(g['hdr0'])), A_ORDER=2))


def test_tile_affines_follow_the_exact_map():
    """The per-tile affine form of TAN -> TAN stays within 1e-3 pixel of the exact map over every tile, for an
    arcsecond-scale grid with rotation, offset and a scale change; identical WCSs give the identity."""
    from astrophotography_amd import wcs
    out = wcs.TanWcs.from_center(303.0272359, 38.3549333, 1.8, (1080, 1920))
    th = np.deg2rad(7.0)
    s = 1.75 / 3600.0
    inp = wcs.TanWcs((1000.3, 520.8), (303.05, 38.34), [[-s * np.cos(th), s * np.sin(th)], [s * np.sin(th), s * np.cos(th)]])
    A = wcs.tile_affines(out, inp, (1080, 1920))
    assert A.shape == (68, 30, 6)
    rng = np.random.default_rng(3)
    x, y = rng.uniform(0, 1919, 4000), rng.uniform(0, 1079, 4000)
    t = A[(y.astype(int) // 16), (x.astype(int) // 64)]
    xin, yin = t[:, 0] * x + t[:, 1] * y + t[:, 2], t[:, 3] * x + t[:, 4] * y + t[:, 5]
    ra, dec = out.pix2sky(x, y)
    xe, ye = inp.sky2pix(ra, dec)
    assert np.abs(xin - xe).max() < 1e-3 and np.abs(yin - ye).max() < 1e-3
    I = wcs.tile_affines(out, out, (1080, 1920))
    np.testing.assert_allclose(I[..., [0, 4]], 1.0, atol=1e-9)
    np.testing.assert_allclose(I[..., [1, 2, 3, 5]], 0.0, atol=1e-6)


def test_oversampling_geometry_host_logic():
    """OVERSAMPLING n geometry on the host: the fine-grid transform maps sub-pixel centres, the oversampled WCS keeps the sky
    position of every block of n x n fine pixels, the fill of excluded mesh boxes equals the oracle's."""
    import numpy as np
    from astrophotography_amd import ops, wcs
    A = np.array([[1.01, -0.02, 3.5, 0.02, 0.99, -1.25]])
    for n in (2, 4):
        fine, shape = ops.oversampled_affines(A, n, (10, 12))
        assert shape == (10 * n, 12 * n)
        f = fine.numpy()[0]
        for (i, j, a, b) in ((0, 0, 0, 0), (3, 7, 1, n - 1), (9, 11, n - 1, 0)):
            cx, cy = j + (b + 0.5) / n - 0.5, i + (a + 0.5) / n - 0.5           # sub-pixel centre in output coordinates
            want = (A[0, 0] * cx + A[0, 1] * cy + A[0, 2], A[0, 3] * cx + A[0, 4] * cy + A[0, 5])
            u, v = n * j + b, n * i + a
            got = (f[0] * u + f[1] * v + f[2], f[3] * u + f[4] * v + f[5])
            assert abs(got[0] - want[0]) < 1e-12 and abs(got[1] - want[1]) < 1e-12
        w = wcs.TanWcs.from_center(83.8, -5.4, 2.0, (40, 50))
        wf = w.oversampled(n)
        # the centre of the n x n block of output pixel (x, y) is that pixel's own centre
        for (x, y) in ((0.0, 0.0), (17.0, 31.0), (49.0, 39.0)):
            ra, dec = w.pix2sky(x, y)
            raf, decf = wf.pix2sky(n * x + (n - 1) / 2.0, n * y + (n - 1) / 2.0)
            assert abs(ra - raf) < 1e-10 and abs(dec - decf) < 1e-10
        # one-pass OVERSAMPLING takes one fine-grid transform per OUTPUT tile (16 x 64 output = 16 n x 64 n fine pixels)
        win = wcs.TanWcs.from_center(83.81, -5.41, 2.1, (60, 70))
        out_shape = (40, 150)
        tiles = wcs.tile_affines(wf := wcs.TanWcs.from_center(83.8, -5.4, 2.0, out_shape).oversampled(n), win,
                                 (out_shape[0] * n, out_shape[1] * n), tile_scale=n)
        assert tiles.shape == ((out_shape[0] + 15) // 16, (out_shape[1] + 63) // 64, 6)
        for (ty, tx) in ((0, 0), (2, 2), (1, 1)):
            for (du, dv) in ((0, 0), (64 * n - 1, 16 * n - 1), (10, 3)):
                u, v = tx * 64 * n + du, ty * 16 * n + dv
                ra, dec = wf.pix2sky(float(u), float(v))
                xe, ye = win.sky2pix(ra, dec)
                a = tiles[ty, tx]
                assert abs(a[0] * u + a[1] * v + a[2] - xe) < 2e-3 and abs(a[3] * u + a[4] * v + a[5] - ye) < 2e-3
    from astrophotography_amd.core.ApMeasureBackground import _fill_excluded
    from oracle import background_ref as br
    rng = np.random.default_rng(5)
    mesh = rng.normal(100, 5, (9, 11))
    good = rng.random((9, 11)) > 0.2
    mesh_nan = np.where(good, mesh, np.nan)
    assert np.array_equal(_fill_excluded(mesh_nan, good), br.fill_excluded(mesh_nan, good))


def test_coadd_output_gain_bookkeeping():
    from astrophotography_amd.core.ApResample import ApResample
    g = [1.5, 1.5, 1.5, 1.5]
    f = [1 / 30.0] * 4
    assert abs(ApResample('CRITICAL', combine='SUM')._output_gain(g, [1.0] * 4, None) - 1.5 / 4) < 1e-12
    assert abs(ApResample('CRITICAL', combine='AVERAGE')._output_gain(g, f, None) - 4 * 1.5 * 30) < 1e-9
    # equal weights = plain average; one dominant weight -> the gain of that frame alone
    assert abs(ApResample('CRITICAL', combine='WEIGHTED')._output_gain(g, f, [2, 2, 2, 2]) - 4 * 45.0) < 1e-9
    assert abs(ApResample('CRITICAL', combine='WEIGHTED')._output_gain(g, f, [1, 1e-9, 1e-9, 1e-9]) - 45.0) < 1e-6
    assert ApResample('CRITICAL', combine='MEDIAN')._output_gain([1.5, None], [1, 1], None) is None


def test_oracle_one_pass_oversampling_equals_fine_resample_plus_block_mean():
    """Pins apref_resample_oversampled_f32 (the restatement the GPU's one-pass OVERSAMPLING kernel is checked against) to the
    oracle pieces it replaces: apref_resample_affine_f32 on the n-times finer grid, then a float64 row-major block mean."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    from oracle import apref
    rng = np.random.default_rng(9)
    N, H, W = 2, 80, 100
    out_shape = (50, 70)
    frames = rng.normal(200, 20, (N, H, W)).astype(np.float32)
    frames[0, 40, 50] = np.nan
    mask = (rng.random((H, W)) < 0.003).astype(np.uint8)
    th = np.deg2rad([0.7, -2.0])
    A = np.stack([1.1 * np.cos(th), -1.1 * np.sin(th), [5.0, 9.0], 1.1 * np.sin(th), 1.1 * np.cos(th), [7.0, 3.0]], 1)
    for n in (2, 3):
        off = 0.5 / n - 0.5
        fine_aff = np.stack([A[:, 0] / n, A[:, 1] / n, A[:, 2] + (A[:, 0] + A[:, 1]) * off,
                             A[:, 3] / n, A[:, 4] / n, A[:, 5] + (A[:, 3] + A[:, 4]) * off], 1)
        fs = np.array([0.5, 1.75], np.float32)
        got, wt = apref.resample_oversampled(frames, fine_aff, n, fscale=fs, mask=mask, out_shape=out_shape, conserve_flux=True)
        fine, _ = apref.resample_affine(frames, fine_aff, fscale=fs, mask=mask, out_shape=(out_shape[0] * n, out_shape[1] * n),
                                        conserve_flux=True)
        want = np.empty_like(got)
        for f in range(N):
            for y in range(out_shape[0]):
                for x in range(out_shape[1]):
                    acc = 0.0
                    for a in range(n):
                        for b in range(n):
                            acc += float(fine[f, y * n + a, x * n + b])
                    want[f, y, x] = np.float32(acc * (1.0 / (n * n)))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or np.array_equal(got, want, equal_nan=True)
        assert np.array_equal(wt, np.isfinite(got).astype(np.uint8))
        assert np.isfinite(got).mean() > 0.5


def test_sort_networks_pass_the_zero_one_principle(tmp_path):
    """The float32 columns are sorted by networks of 2-, 3- and 4-sorters found by search (csrc/stack_sort.h, make_opnet):
    tools/netsearch/verify_opnet.cpp checks every slot count's network - complete and pruned to what the float32 clip
    reads - on the 0-1 inputs its pre-sorted structure allows (each 16-block exhaustively)."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    exe = str(tmp_path / 'verify_opnet')
    r = subprocess.run([hipcc, '-O2', '-std=c++17', '-fconstexpr-steps=100000000', '-I', os.path.join(ROOT, 'include'), '-I',
                        os.path.join(ROOT, 'astrophotography_amd', 'csrc'), os.path.join(ROOT, 'tools', 'netsearch', 'verify_opnet.cpp'),
                        '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout[-3000:]
    assert 'NP  64 T 4:  750 instructions' in r.stdout          # the headline kernel's network (890 with sort4 + Batcher)


def test_np_exact_header_equals_numpy(tmp_path):
    """csrc/np_exact.h is the one statement of numpy's summation order and of the order-preserving float key that the
    bit-exact statistics kernels share.  tools/np_exact_check.cpp runs it on the host; NumPy itself is the reference,
    everything bit for bit: np.add.reduce (leaf, tree and 8192-element pieces, on both sides of every boundary), the sum of
    squared deviations, the NaN-as-zero sum with its NaN count, and the key (strictly monotone, inverted exactly)."""
    import struct
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    exe = str(tmp_path / 'np_exact_check')
    r = subprocess.run([hipcc, '--cuda-host-only', '-O2', '-std=c++17', '-ffp-contract=off', '-I', os.path.join(ROOT, 'astrophotography_amd', 'csrc'),
                        os.path.join(ROOT, 'tools', 'np_exact_check.cpp'), '-o', exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]

    rng = np.random.default_rng(20261018)
    lengths = list(range(301)) + [511, 512, 513, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 5776, 8191, 8192, 8193, 8192 + 129, 20000]
    records = []                                                            # (kind, array, m)
    for dt in (np.float32, np.float64):
        for n in lengths:
            records.append(('S', (rng.standard_normal(n) * 1e3).astype(dt), None))
        mixed = rng.choice([-1.0, 1.0], 20000) * np.exp2(rng.uniform(-30, 30, 20000))
        records.append(('S', mixed.astype(dt), None))
        for n in (7, 8, 129, 4097):
            a = (rng.standard_normal(n) * 1e3).astype(dt)
            a[rng.choice(n, max(1, n // 50), replace=False)] = np.nan
            records.append(('S', a, None))
        fi, bits = np.finfo(dt), np.dtype(dt).itemsize * 8
        ut = np.uint32 if dt is np.float32 else np.uint64
        special = np.array([0.0, fi.smallest_subnormal, fi.smallest_normal - fi.smallest_subnormal, fi.smallest_normal, 1.0, fi.max,
                            np.inf], dtype=dt)
        pats = rng.integers(0, 2 ** bits, 10000, dtype=ut, endpoint=False).view(dt)
        records.append(('K', np.concatenate([special, -special, pats[~np.isnan(pats)]]).astype(dt), None))
    path = str(tmp_path / 'records.bin')
    with open(path, 'wb') as fh:
        for i, (kind, a, _) in enumerate(records):
            with np.errstate(all='ignore'):
                m = a.dtype.type(a.mean()) if a.size and kind == 'S' else a.dtype.type(0)
            records[i] = (kind, a, m)
            fh.write(struct.pack('<iiqd', ord(kind), a.itemsize, a.size, float(m) if np.isfinite(m) else 0.0))
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(records)

    n_sums = n_nan = 0
    for (kind, a, m), line in zip(records, lines):
        dt, ut = a.dtype.type, (np.uint32 if a.itemsize == 4 else np.uint64)
        f = line.split()
        assert f[0] == kind
        bits_of = lambda v: int(np.asarray(v, dtype=dt).view(ut))
        if kind == 'S':
            got_sum, got_sq, got_nansum, got_nans = int(f[1], 16), int(f[2], 16), int(f[3], 16), int(f[4])
            if np.isnan(a).any():
                assert got_nansum == bits_of(np.nansum(a)) and got_nans == int(np.isnan(a).sum()), a.size
                n_nan += 1
            else:
                d = a - m
                assert got_sum == bits_of(np.add.reduce(a)), (a.dtype, a.size)
                assert got_sq == bits_of(np.add.reduce(d * d)), (a.dtype, a.size)
                assert got_nansum == got_sum and got_nans == 0
                n_sums += 1
        else:
            keys = np.array([int(x, 16) for x in f[1::2]], dtype=np.uint64)
            back = np.array([int(x, 16) for x in f[2::2]], dtype=np.uint64)
            assert np.array_equal(back, a.view(ut).astype(np.uint64))                   # from(to(x)) == x, bitwise
            assert a[0] == 0 and a[7] == 0 and np.signbit(a[7]) and keys[7] < keys[0]   # to(-0) < to(+0)
            _, first = np.unique(a.view(ut), return_index=True)
            order = first[np.argsort(keys[first], kind='stable')]
            v, k = a[order], keys[order]
            assert np.all(k[1:] > k[:-1])
            zeros = (v[:-1] == 0) & (v[1:] == 0) & np.signbit(v[:-1]) & ~np.signbit(v[1:])
            assert np.all((v[1:] > v[:-1]) | zeros)                                     # sorted by key = sorted by value
    assert n_sums == 2 * (len(lengths) + 1) and n_nan == 8


def test_mad_window_crossing_equals_scan():
    """stack_reduce.h:mad_std_window (round 4) finds the minimum over the windows [L, L + k1] of max(|x_L - med|, |x_(L+k1) - med|)
    by a binary search for the crossing of the two end deviations instead of scanning every window.  The same two procedures in
    NumPy on random sorted columns (ties, constant runs, outliers, every count 1 .. 64): identical values, and equal to
    astropy's definition median(|x - median(x)|)."""
    rng = np.random.default_rng(77)

    def scan(x):
        n = len(x)
        k1 = (n - 1) >> 1
        med = 0.5 * (float(x[(n - 1) >> 1]) + float(x[n >> 1]))
        dl = np.abs(x.astype(np.float64) - med)
        f = [max(dl[L], dl[L + k1]) for L in range(0, n - k1)]
        g = [max(dl[L - 1], dl[L + k1]) for L in range(1, n - k1)]
        return min(f), (min(g) if g else np.inf)

    def search(x):
        n = len(x)
        k1 = (n - 1) >> 1
        bk = n - k1
        med = 0.5 * (float(x[(n - 1) >> 1]) + float(x[n >> 1]))
        d = lambda i: abs(float(x[min(max(i, 0), n - 1)]) - med)
        lo, hi = 0, bk - 1
        while lo < hi:
            mid = (lo + hi) >> 1
            if d(mid + k1) >= d(mid):
                hi = mid
            else:
                lo = mid + 1
        DL = lambda L: d(L) if L >= 0 else np.inf
        DR = lambda L: d(L + k1) if L < bk else np.inf
        m1 = min(max(DL(lo - 1), DR(lo - 1)), max(DL(lo), DR(lo)))
        m2 = min(max(DL(lo - 2), DR(lo - 1)), max(DL(lo - 1), DR(lo)), max(DL(lo), DR(lo + 1)))
        return m1, m2

    for trial in range(4000):
        n = int(rng.integers(1, 65))
        kind = trial % 4
        if kind == 0:
            x = rng.normal(500, 20, n)
        elif kind == 1:
            x = rng.integers(0, 4, n).astype(np.float64)     # heavy ties
        elif kind == 2:
            x = np.concatenate([rng.normal(0, 1, n - n // 3), rng.normal(0, 1, n // 3) * 1e6])
        else:
            x = np.full(n, 7.0)
        x = np.sort(x.astype(np.float32))
        s1, s2 = scan(x)
        b1, b2 = search(x)
        assert b1 == s1, (trial, n)
        if n % 2 == 0:
            assert b2 == s2, (trial, n)
            mad = 0.5 * (b1 + b2)
        else:
            mad = b1
        assert mad == np.median(np.abs(x.astype(np.float64) - np.median(x.astype(np.float64)))), (trial, n)


def test_fitsio_header_only_read_and_write_pool(tmp_path):
    """Round 6, the per-frame flow on files: fitsio.read(want_data=False) reads the header blocks and the bytes behind the data unit
    (extensions, kept verbatim) without the data unit - same Header, same tail as the full read; fitsio.WritePool hands file writes to
    its threads from per-slot staging buffers, keeps at most `workers` in flight, and wait() re-raises the first error after every
    write has finished."""
    import threading
    import time
    from astrophotography_amd import fitsio
    a = (np.arange(37 * 53) % 65536).astype(np.uint16).reshape(37, 53)
    h = fitsio.Header()
    h['OBJECT'] = 'm31'
    h['EXPTIME'] = 3.5
    p = str(tmp_path / 'a.fits')
    fitsio.write(p, a, h, extensions=[('BADPIX', np.ones((4, 5), np.uint8), None)])
    d1, h1 = fitsio.read(p)
    d0, h0 = fitsio.read(p, want_data=False)
    assert d0 is None and np.array_equal(d1, a)
    assert h0.tostring() == h1.tostring() and h0._tail == h1._tail and len(h0._tail) == 2 * 2880
    q = str(tmp_path / 'b.fits')
    fitsio.write(q, np.ones((8, 8), np.float32), h)
    assert fitsio.read(q, want_data=False)[1]._tail == b'' and fitsio.getheader(q)['EXPTIME'] == 3.5

    class HostPool(fitsio.WritePool):                       # the pool's mechanics without pinned memory (no device here)
        def staging(self, nbytes):
            slot = self._free.get()
            slot[0] = bytearray(nbytes)
            return slot

    pool = HostPool(workers=2)
    inflight, peak, done = [0], [0], []
    lock = threading.Lock()

    def job(i):
        with lock:
            inflight[0] += 1
            peak[0] = max(peak[0], inflight[0])
        time.sleep(0.02)
        with lock:
            inflight[0] -= 1
            done.append(i)

    for i in range(7):
        pool.submit(pool.staging(16), lambda i=i: job(i))   # staging() blocks while both slots are being written out
    pool.wait()
    assert sorted(done) == list(range(7)) and peak[0] <= 2
    pool.submit(pool.staging(1), lambda: 1 / 0)
    pool.submit(pool.staging(1), lambda: job(99))
    with pytest.raises(ZeroDivisionError):
        pool.wait()
    assert 99 in done                                       # the write behind the failing one still happened
    pool.close()
