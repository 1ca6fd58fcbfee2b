"""F5 ApAutoBadcols / ap_auto_badcol on the host: the CLI, the stdout format against the reference's recorded stdout
(G13) and the argument checks of the new C entry points.  No GPU."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from tests.util import GOLDEN, load_golden


def _meta():
    return json.loads(str(load_golden('g13_autobadcol.npz')['_meta']))


def test_script_defaults_and_help():
    from astrophotography_amd.scripts import ap_auto_badcol as s
    a = s.command_line_opts(['img.fits'])
    assert (a.fitsimage, a.sigma, a.window, a.loglevel) == ('img.fits', 5.0, 11, 'INFO')
    a = s.command_line_opts(['img.fits', '--sigma', '4', '--window', '7', '-l', 'DEBUG'])
    assert (a.sigma, a.window, a.loglevel) == (4.0, 7, 'DEBUG')
    assert isinstance(a.sigma, float) and isinstance(a.window, int)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit) as e:
        s.command_line_opts(['--help'])
    assert e.value.code == 0
    assert 'FITSIMAGE.FITS' in buf.getvalue() and '--window' in buf.getvalue()


def test_format_report_matches_reference_stdout():
    """The formatter, fed the reference's own index lists, reproduces the reference script's stdout byte for byte."""
    from astrophotography_amd.scripts import ap_auto_badcol as s
    m = _meta()
    assert len(m['runs']) == 4
    seen_cols = 0
    for run in m['runs']:
        ref = run['stdout']
        path = os.path.join(GOLDEN, run['file'])
        a = s.command_line_opts([path] + run['argv'])
        # the reference's index lists, read back from its stdout (1-based) - the GPU test computes them
        cols, rows, key = [], [], None
        for line in ref.splitlines()[1:]:
            if line.startswith('bad_'):
                key = line.split(':')[0]
            elif line.startswith('- '):
                (cols if key == 'bad_columns' else rows).append(int(line[2:]) - 1)
        badcols = np.array(cols, np.int64) if cols else None
        badrows = np.array(rows, np.int64) if rows else None
        seen_cols += len(cols)
        out = s.format_report(path, a.sigma, a.window, badcols, badrows)
        assert out == ref.replace(m['placeholder'], path), (run, out)
    assert seen_cols > 0


def test_format_report_empty_and_none():
    from astrophotography_amd.scripts import ap_auto_badcol as s
    out = s.format_report('x.fits', 5.0, 11, None, np.zeros(0, np.int64))
    assert out == '# Auto bad columns from x.fits, sigma=5.0, window_len=11\n# No bad columns detected.\nbad_rows: {}\n'
    out = s.format_report('x.fits', 4.0, 7, np.array([0, 9]), None)
    assert out == '# Auto bad columns from x.fits, sigma=4.0, window_len=7\nbad_columns:\n- 1\n- 10\n# No bad rows detected.\n'


def test_report_is_user_badpix_yaml(tmp_path):
    """The stdout is what ApFindBadPixels.add_user_badpix reads (bad_columns / bad_rows, 1-based)."""
    from astrophotography_amd.scripts import ap_auto_badcol as s
    from astrophotography_amd.core.ApFindBadPixels import ApFindBadPixels
    y = tmp_path / 'auto.yml'
    y.write_text(s.format_report('x.fits', 5.0, 11, np.array([3, 40]), None))
    obj = ApFindBadPixels.__new__(ApFindBadPixels)
    import logging
    obj._logger = logging.getLogger('t')
    cols, rows, rects = obj._read_user_badpix(y)
    assert cols == [4, 41] and rows is None and rects is None


def test_capi_rejects_bad_arguments_before_device_work():
    import ctypes as C
    from astrophotography_amd import _lib
    lib = _lib.load()                          # loads without a GPU; every call below fails its argument checks
    dummy = C.c_void_p(16)                     # never dereferenced: validation comes first
    E = _lib.E_INVAL
    assert lib.apgpu_axis_nanmedian(None, _lib.APGPU_F32, 1, 4, 4, 0, dummy, None) == E
    assert b'NULL' in lib.apgpu_last_error()
    assert lib.apgpu_axis_nanmedian(dummy, _lib.APGPU_F32, 1, 4, 4, 0, None, None) == E
    assert lib.apgpu_axis_nanmedian(dummy, _lib.APGPU_F32, 0, 4, 4, 0, dummy, None) == E
    assert lib.apgpu_axis_nanmedian(dummy, _lib.APGPU_F32, 1, 0, 4, 0, dummy, None) == E
    assert lib.apgpu_axis_nanmedian(dummy, _lib.APGPU_F32, 1, 4, 0, 1, dummy, None) == E
    assert lib.apgpu_axis_nanmedian(dummy, _lib.APGPU_F32, 1, 4, 4, 2, dummy, None) == E
    assert lib.apgpu_axis_nanmedian(dummy, 7, 1, 4, 4, 0, dummy, None) == E
    assert lib.apgpu_sliding_clipped_stats_ws_bytes(_lib.APGPU_F32, 1, 4096, 11) >= 4096 * 11 * 4 // 64
    assert lib.apgpu_sliding_clipped_stats_ws_bytes(_lib.APGPU_F32, 1, 4096, 0) == 0
    assert lib.apgpu_sliding_clipped_stats_ws_bytes(_lib.APGPU_F64, 0, 4096, 11) == 0

    def sl(values=dummy, dtype=_lib.APGPU_F32, n=1, L=16, w=11, outs=(dummy,) * 4, ws=dummy, ws_bytes=1 << 30):
        return lib.apgpu_sliding_clipped_stats(values, dtype, n, L, w, 3.0, 5, 5.0, *outs, ws, ws_bytes, None)
    assert sl(values=None) == E
    for i in range(4):
        outs = [dummy] * 4
        outs[i] = None
        assert sl(outs=tuple(outs)) == E
    assert sl(ws=None) == E
    assert sl(w=0) == E
    assert b'window_len' in lib.apgpu_last_error()
    assert sl(w=-3) == E
    assert sl(n=0) == E
    assert sl(L=0) == E
    assert sl(dtype=_lib.APGPU_U16) == E
    assert sl(ws_bytes=0) == _lib.E_WORKSPACE
    assert lib.apgpu_version() == 130


def test_class_is_exported_lazily():
    import astrophotography_amd as ap
    assert 'ApAutoBadcols' in ap.__all__
    cls = ap.ApAutoBadcols
    obj = cls('CRITICAL')
    with pytest.raises(ValueError):
        cls('NOT_A_LEVEL')
    with pytest.raises(ValueError):
        obj.process(np.zeros(5, np.float32))
    with pytest.raises(ValueError):
        obj.process_slab(np.zeros((4, 5), np.float32))


def test_np_clip_stats_reproduces_astropy_g16():
    """tests/util.np_clip_stats, the numpy restatement the GPU tests of the sliding statistics compare with, against astropy's
    own sigma_clipped_stats on the float32 vectors of golden group G16 (12 .. 1252 values, stars and non-finite values among
    them): mean, median and std of its survivors equal astropy's, bit for bit."""
    import json
    import warnings
    from tests.util import assert_biteq, load_golden, np_clip_stats
    g = load_golden('g16_annulus.npz')
    meta = json.loads(str(g['_meta']))
    assert len(meta) >= 30
    for m in meta:
        v = g['c%d_values' % m['case']]
        assert v.dtype == np.float32 and m['stat_dtype'] == 'float32'
        x = np_clip_stats(v)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            got = np.array([np.mean(x), np.median(x), np.std(x)], np.float64)
        assert_biteq(got, np.asarray(g['c%d_stats' % m['case']], np.float64), m['name'])
