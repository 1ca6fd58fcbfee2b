"""F10's RCD method on the GPU (rcd_kernel of csrc/demosaic.hip) against the NumPy model tests/demosaic_rcd_model.py:
bit for bit in every output, input type and arrangement, on shapes where every tap folds and on the seams of the kernel's tile;
slabs, views, non-finite samples, exact constants, one call under the guard bands of tests/guard.py, and the files ApDebayer and
ap_debayer write."""
import numpy as np
import pytest

from astrophotography_amd import _lib
from tests import demosaic_model as dm
from tests import demosaic_rcd_model as rm
from tests.test_gpu_demosaic import GAINS, _dev, _host, _mosaic, _same_bits

pytestmark = pytest.mark.gpu

F = np.float32
TH, TW, HALO = _lib.DEMOSAIC_RCD_TILE_H, _lib.DEMOSAIC_RCD_TILE_W, _lib.DEMOSAIC_RCD_HALO
OUTPUTS = ('rgb', 'rgb_u16', 'grey')
SMALL = [(2, 2), (2, 3), (3, 2), (5, 7), (11, 9)]                     # every tap folds, some more than once
# one tile; one tile plus and minus 1 in each direction; two tiles plus 3 in both
SEAMS = [(TH, TW), (TH + 1, TW), (TH - 1, TW), (TH, TW + 1), (TH, TW - 1), (2 * TH + 3, 2 * TW + 3)]
U16_BLACK, F32_BLACK = [256, 250, 300, 255], [900.5, 850.25, 1000.0, 870.125]


def _want(mosaic, pattern, black, gain):
    """The model's three outputs from one evaluation."""
    rgb = rm.demosaic(mosaic, pattern, black, gain)
    return {'rgb': rgb, 'rgb_u16': dm.to_u16(rgb), 'grey': dm.luma(rgb)}


def _check(mosaic, pattern, black=None, gain=None):
    from astrophotography_amd import ops
    d = _dev(mosaic)
    want = _want(mosaic, pattern, black, gain)
    for output in OUTPUTS:
        got = _host(ops.bayer_demosaic(d, pattern, black, gain, 'rcd', output))
        _same_bits(got, want[output], (mosaic.shape, str(mosaic.dtype), pattern, output))
    return want


def test_seams_come_from_the_exported_tile():
    assert rm.HALO == HALO and max(max(s) for s in SEAMS) < 600 and max(s[0] for s in SEAMS) < 300


@pytest.mark.parametrize('shape', SMALL + SEAMS)
def test_rcd_bit_equal(shape):
    for i, (name, pat) in enumerate(sorted(dm.ARRANGEMENTS.items())):
        _check(_mosaic(shape, 100 + i, np.uint16), pat)
        _check(_mosaic(shape, 200 + i, F), pat)


@pytest.mark.parametrize('shape', [(5, 7), (11, 9), (TH + 1, TW - 1), (2 * TH + 3, 2 * TW + 3)])
def test_gains_and_blacks_keep_bit_equality(shape):
    for i, (name, pat) in enumerate(sorted(dm.ARRANGEMENTS.items())):
        gain = GAINS[i % 2]
        u = _mosaic(shape, 300 + i, np.uint16)
        u.ravel()[::3] //= 256                                   # many samples below the black levels
        _check(u, pat, U16_BLACK, gain)
        _check(_mosaic(shape, 400 + i, F), pat, F32_BLACK, gain)


def test_direct_ignores_the_method():
    from astrophotography_amd import ops
    m = _mosaic((9, 13), 5, np.uint16)
    pat = dm.ARRANGEMENTS['GRBG']
    _same_bits(_host(ops.bayer_demosaic(_dev(m), pat, U16_BLACK, GAINS[0], 'rcd', 'direct')), dm.demosaic(m, pat, U16_BLACK, GAINS[0], output='direct'))


def test_slab_equals_single_frames():
    import torch
    from astrophotography_amd import ops
    pat, gain, black = dm.ARRANGEMENTS['GBRG'], GAINS[1], [10, 20, 30, 40]
    for dtype, shape in ((np.uint16, (3, TH + 2, TW + 6)), (F, (3, 19, 37))):
        slab = _mosaic(shape, 7, dtype)
        d = _dev(slab)
        want = [_want(slab[f], pat, black, gain) for f in range(3)]
        for output in OUTPUTS:
            got = ops.bayer_demosaic(d, pat, black, gain, 'rcd', output)
            assert got.shape[0] == 3 and got.dim() == (4 if output.startswith('rgb') else 3)
            bits = torch.int16 if output == 'rgb_u16' else torch.int32
            for f in range(3):
                one = ops.bayer_demosaic(d[f], pat, black, gain, 'rcd', output)
                assert torch.equal(got[f].view(bits), one.view(bits))
                _same_bits(_host(one), want[f][output])


def test_out_views_and_unaligned_rows():
    import torch
    from astrophotography_amd import ops
    pat, gain = dm.ARRANGEMENTS['BGGR'], GAINS[0]
    for shape in ((TH + 2, TW + 2), (9, 13)):                    # W = 66, 13: rows start off 16-byte boundaries
        for dtype in (np.uint16, F):
            m = _mosaic(shape, 600, dtype)
            d = _dev(m)
            wants = _want(m, pat, None, gain)
            for output in OUTPUTS:
                want = wants[output]
                odt = torch.uint16 if output == 'rgb_u16' else torch.float32
                for shift in (1, 3):                             # a view that starts 1 or 3 elements into an aligned buffer
                    buf = torch.zeros(want.size + 8, dtype=odt, device='cuda')
                    out = buf[shift:shift + want.size].view(want.shape)
                    assert out.data_ptr() % 16 != 0
                    res = ops.bayer_demosaic(d, pat, None, gain, 'rcd', output, out=out)
                    assert res.data_ptr() == out.data_ptr()
                    _same_bits(_host(out), want, (shape, output, shift))
                    flat = _host(buf)
                    assert not flat[:shift].any() and not flat[shift + want.size:].any()          # nothing outside the view


def test_non_finite_samples_stay_within_the_halo():
    from astrophotography_amd import ops
    shape = (2 * TH + 6, 2 * TW + 12)
    # a corner, an edge, the interior, both sides of the tile seams (rows TH - 1 | TH, columns TW - 1 | TW)
    nans = ((0, 0), (0, TW + 26), (TH + 18, TW + 36), (TH - 1, TW - 1), (TH, TW))
    pinf, ninf = (20, 30), (TH + 1, TW + 1)
    bad = np.array(nans + (pinf, ninf))
    rr, cc = np.indices(shape)
    far = np.ones(shape, bool)
    for r, c in bad:
        far &= np.maximum(np.abs(rr - r), np.abs(cc - c)) > HALO
    assert far.any()
    for i, (name, pat) in enumerate(sorted(dm.ARRANGEMENTS.items())):
        m = _mosaic(shape, 500 + i, F)
        for r, c in nans:
            m[r, c] = np.nan
        m[pinf] = np.inf
        m[ninf] = -np.inf                                        # below black: the sample is 0
        want = _check(m, pat, black=[1, 2, 3, 4], gain=GAINS[0])
        got = _host(ops.bayer_demosaic(_dev(m), pat, [1, 2, 3, 4], GAINS[0], 'rcd'))
        assert np.isfinite(got[:, far]).all() and np.isfinite(want['rgb'][:, far]).all()
        assert not np.isfinite(got[:, TH + 18, TW + 36]).all()


@pytest.mark.parametrize('shape', [(6, 10), (TH + 4, 2 * TW + 8)])
def test_constant_mosaics_are_exact(shape):
    from astrophotography_amd import ops
    levels = (1200, 3000, 700)
    full = _dev(np.full(shape, 65535, np.uint16))
    for pat in dm.ARRANGEMENTS.values():
        got = _host(ops.bayer_demosaic(full, pat, method='rcd'))
        assert np.array_equal(got, np.full((3,) + shape, 65535, F)), pat
        assert np.array_equal(_host(ops.bayer_demosaic(full, pat, method='rcd', output='rgb_u16')), np.full((3,) + shape, 65535, np.uint16))
        mosaic = np.array([levels[0], levels[1], levels[2], levels[1]], np.uint16)[dm.colour_map(shape, pat)]
        for dtype in (np.uint16, F):
            got = _host(ops.bayer_demosaic(_dev(mosaic.astype(dtype)), pat, method='rcd'))
            for c, v in enumerate(levels):
                assert np.array_equal(got[c], np.full(shape, v, F)), (pat, dtype, c)


def test_guarded_on_a_side_stream(monkeypatch):
    """Inputs in poisoned slabs at shift 0 and one element, ops' own and caller-owned outputs, on a side stream: nothing outside the
    output is written, the input is not written, and the result does not depend on what lies around the input."""
    import torch
    from astrophotography_amd import ops
    from tests.guard import current, guarded, intact, place, unchanged
    pat, gain = dm.ARRANGEMENTS['GRBG'], GAINS[1]
    cases = [(shape, dtype, black) for shape in ((5, 7), (TH + 3, TW + 6)) for dtype, black in ((np.uint16, U16_BLACK), (F, F32_BLACK))]
    wants = {}
    runs = {}
    stream = torch.cuda.Stream()
    for poison in (0xFF, 0x00):
        results = []
        with guarded(monkeypatch) as g, torch.cuda.stream(stream):
            for shape, dtype, black in cases:
                m = _mosaic(shape, 77, dtype)
                key = (shape, np.dtype(dtype).name)
                if key not in wants:
                    wants[key] = _want(m, pat, black, gain)
                for shift in (0, m.dtype.itemsize):
                    t, tok = place(m, poison, shift)
                    for output in OUTPUTS:
                        want = wants[key][output]
                        own, otok = place(np.zeros(want.shape, want.dtype), poison, want.dtype.itemsize if shift else 0, what='out')
                        ops.bayer_demosaic(t, pat, black, gain, 'rcd', output, out=own)
                        mine = ops.bayer_demosaic(t, pat, black, gain, 'rcd', output)
                        results.append((key, shift, output, tok, otok, mine, want))
            stream.synchronize()
        assert g.lib.names() == {'apgpu_bayer_demosaic'}
        assert all(s == stream.cuda_stream and s != 0 for _, s in g.lib.streams()) and len(g.lib.streams()) == len(results) * 2
        runs[poison] = []
        for key, shift, output, tok, otok, mine, want in results:
            unchanged(tok)
            intact(otok)
            own = current(otok).view(want.dtype).reshape(want.shape)
            _same_bits(own, want, (key, shift, output, 'out='))
            _same_bits(_host(mine), want, (key, shift, output))
            runs[poison].append(own.tobytes())
    assert runs[0xFF] == runs[0x00]


def test_apdebayer_and_ap_debayer_write_rcd(tmp_path):
    import astrophotography_amd as ap
    from astrophotography_amd import fitsio, ops
    from astrophotography_amd.scripts import ap_debayer
    pat = dm.ARRANGEMENTS['GRBG']
    m = _mosaic((34, 70), 901, np.uint16) // 2
    black, gains = [256, 250, 300, 255], [2, 1, 1.5, 1]
    d = ap.ApDebayer('CRITICAL')
    direct = ops.bayer_demosaic(_dev(m), pat, black, gains, 'rcd')
    _same_bits(_host(direct), rm.demosaic(m, pat, black, gains))
    _same_bits(_host(d.rgb(_dev(m), pat, 'rcd', gains, True, black)), _host(direct))
    _same_bits(_host(d.rgb(_dev(m), pat, 'rcd', gains, True, black, as_uint16=True)), _host(ops.bayer_demosaic(_dev(m), pat, black, gains, 'rcd', 'rgb_u16')))
    _same_bits(_host(d.grey(_dev(m), pat, 'rcd', gains, True, black)), _host(ops.bayer_demosaic(_dev(m), pat, black, gains, 'rcd', 'grey')))
    with pytest.raises(ValueError, match='method'):
        d.rgb(_dev(m), pat, 'ahd')

    hdr = fitsio.Header()
    hdr['BAYERPAT'] = ('GRBG', 'Bayer pattern')
    src, root, grey = str(tmp_path / 'mosaic.fits'), str(tmp_path / 'out'), str(tmp_path / 'lum.fits')
    fitsio.write(src, m, hdr)
    assert ap_debayer.main([src, root, '-m', 'rcd', '-w', 'user[2, 1, 1.5, 1]', '--black', '256', '250', '300', '255', '-l', 'CRITICAL']) == 0
    for c, colour in enumerate('rgb'):
        data, h = fitsio.read('%s_%s.fits' % (root, colour))
        assert h['DEBAYER'] == 'RCD' and h['WBBLUE'] == 1.5
        _same_bits(np.asarray(data), _host(direct)[c], colour)
    names = d.debayer_files(src, root, method='rcd', wb_method=gains, black=black, grey=grey)
    assert names == [grey]
    data, h = fitsio.read(grey)
    assert h['DEBAYER'] == 'RCD'
    _same_bits(np.asarray(data), _host(ops.bayer_demosaic(_dev(m), pat, black, gains, 'rcd', 'grey')))
