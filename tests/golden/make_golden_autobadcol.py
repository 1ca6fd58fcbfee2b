#!/opt/conda/bin/python3.9 -B
"""Golden-vector generator G13: ApAutoBadcols (core/ApAutoBadcols.py:143-258) and scripts/ap_auto_badcol.py:76-116.

RUN ONLY IN THE BUILD CONTAINER, like make_golden.py (same bootstrap):

    /opt/conda/bin/python3.9 -B tests/golden/make_golden_autobadcol.py

For every case it calls the reference's own code - np.nanmedian(data, axis=0 / 1) exactly as process() does
(:196, :200), ApAutoBadcols._sliding_stats_1d and ApAutoBadcols.process - and records the inputs, both median
arrays, the sliding clipped mean / std, nsig and the flags of _process (:225-227) and the index lists.
Two FITS fixtures (int16 with BZERO 32768 and a PEDESTAL, float32) get the reference script's stdout, from
main([...]) under redirect_stdout, for the default flags and one non-default pair (the reference parses --sigma /
--window without type=, so the non-default run is made with the values converted, which is what the
port's CLI does).  The reference's CPU time for one 4096^2 float32 frame is recorded in the metadata.
"""
import contextlib
import io
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402  (the bootstrap: numpy shims, stubs, bottleneck off, the reference)

np = mg.np
fits = mg.fits
ap = mg.ap

from AstroPhotography.scripts import ap_auto_badcol as ref_script      # noqa: E402

PLACEHOLDER = '{FITSFILE}'


def ref_case(data, window_len, nsigma):
    ab = ap.ApAutoBadcols('CRITICAL')
    out = {}
    for axis, tag in ((0, 'cols'), (1, 'rows')):
        m = np.nanmedian(data, axis=axis)
        mean, std = ab._sliding_stats_1d(m, window_len)
        with np.errstate(divide='ignore', invalid='ignore'):
            nsig = np.abs(m - mean) / std
        out['med_' + tag] = m
        out['mean_' + tag] = mean
        out['std_' + tag] = std
        out['nsig_' + tag] = nsig
        out['flag_' + tag] = (nsig >= nsigma).astype(np.uint8)
    badcols, badrows = ab.process(data, nsigma, window_len)
    out['badcols'] = np.zeros(0, np.int64) if badcols is None else np.asarray(badcols, np.int64)
    out['badrows'] = np.zeros(0, np.int64) if badrows is None else np.asarray(badrows, np.int64)
    out['badcols_none'] = np.array(badcols is None)
    out['badrows_none'] = np.array(badrows is None)
    return out


def sky(rng, H, W, dtype=np.float32, level=1000.0, noise=10.0):
    return (level + noise * rng.standard_normal((H, W))).astype(dtype)


def cases():
    rng = np.random.default_rng(13)
    cs = []

    d = sky(rng, 64, 96)
    d[:, 17] += 300.0                       # hot column
    d[:, 60] -= 250.0                       # cold column
    d[40, :] += 200.0                       # hot row
    cs.append(('f32_even', d, 11))

    d = sky(rng, 65, 97)
    d[:, 3] += 150.0
    d[11, :] -= 300.0
    cs.append(('f32_odd', d, 3))

    d = sky(rng, 63, 50, np.float64)
    d[:, 25] += 80.0
    d[0, :] += 500.0                        # a bad first row (edge window)
    cs.append(('f64', d, 11))

    d = np.clip(sky(rng, 64, 80, np.float64, 2000.0, 30.0), 0, 65535).astype(np.uint16)
    d[:, 71] = 60000
    d[20, :] //= 2
    cs.append(('u16', d, 11))

    d = np.clip(sky(rng, 41, 33, np.float64, 30000.0, 300.0), 0, 65535).astype(np.uint16)
    cs.append(('u16_odd', d, 5))

    # both numpy median paths on both axes: columns of 640 values (np.median) and rows of 48 (np.ma.median), and back
    d = sky(rng, 640, 48)
    d[:, 9] += 100.0
    d[300, :] += 150.0
    d[5::7, 30] = np.nan
    cs.append(('f32_640x48', d, 11))
    d = sky(rng, 48, 640)
    d[:, 600] -= 120.0
    d[7, :] += 90.0
    d[13, 2::5] = np.nan
    cs.append(('f32_48x640', d, 11))
    d = sky(rng, 640, 48, np.float64)
    d[::3, 4] = np.nan
    d[100, :] += 70.0
    cs.append(('f64_640x48', d, 11))
    d = sky(rng, 48, 640, np.float64)
    d[:, 333] += 60.0
    cs.append(('f64_48x640', d, 11))

    # non-finite values: NaN, +-inf, an all-NaN column and row, an all-inf column (odd and even counts)
    d = sky(rng, 40, 60)
    d[:, 5] = np.nan
    d[17, :] = np.nan
    d[3, 8] = np.inf
    d[::2, 9] = np.inf
    d[1::2, 9] = -np.inf                    # even count, -inf / +inf in the middle: NaN median
    d[:, 12] = np.inf
    d[::3, 20] = -np.inf
    d[5:9, 31] = np.nan
    cs.append(('f32_nonfinite', d, 11))
    d = sky(rng, 41, 61)
    d[:, 7] = 3.0e38                        # odd count < 600: np.ma.median's x + x overflows to inf
    d[2, :] = -3.0e38
    cs.append(('f32_overflow_ma', d, 11))
    d = sky(rng, 601, 6)
    d[:, 2] = 3.0e38                        # odd count >= 600: np.median keeps the value
    cs.append(('f32_overflow_large', d, 3))

    # lines of length 1
    cs.append(('f32_1xW', sky(rng, 1, 50), 11))
    cs.append(('f32_Hx1', sky(rng, 50, 1), 11))
    cs.append(('f64_1x1', sky(rng, 1, 1, np.float64), 11))

    # constant regions: std == 0 -> nsig inf (bad) or nan (not bad)
    d = np.full((30, 40), 500.0, np.float32)
    d[:, 25:] += rng.standard_normal((30, 15)).astype(np.float32)
    d[:, 10] = 700.0
    d[4, :20] = 100.0
    cs.append(('f32_constant', d, 5))

    # window lengths 1, 31, 101 and longer than the line (a window of 1 is one value: std 0 everywhere)
    base = sky(rng, 120, 200)
    base[:, 77] += 60.0
    base[50, :] += 45.0
    for w in (1, 31, 101, 401):
        cs.append(('f32_w%d' % w, base, w))
    cs.append(('f32_even_window', base, 10))   # an even window: hw = 4 (int((10 - 1) / 2))
    d = sky(rng, 160, 140, np.float64)
    d[:, 30] += 40.0
    cs.append(('f64_w1001', d, 1001))
    d = sky(rng, 140, 180)
    d[:, 90] += 50.0
    cs.append(('f32_w201_tree', d, 201))      # windows of more than 128 values: numpy's pairwise tree
    return cs


def fits_fixtures(rng):
    """Two small FITS files: int16 + BZERO 32768 (uint16 data) with a PEDESTAL, and float32."""
    u = np.clip(1500.0 + 25.0 * rng.standard_normal((70, 90)), 0, 65535).astype(np.uint16)
    u[:, 33] += 900
    u[:, 34] += 400
    u[51, :] -= 600
    hdu = fits.PrimaryHDU(u)
    hdu.header['PEDESTAL'] = -100.0
    p16 = os.path.join(HERE, 'g13_autobadcol_u16.fits')
    hdu.writeto(p16, overwrite=True)
    f = (800.0 + 12.0 * rng.standard_normal((61, 77))).astype(np.float32)
    f[:, 5] -= 200.0
    f[:, 70] += 55.0
    f[20, :] += 100.0
    f[44, :] += 30.0
    pf = os.path.join(HERE, 'g13_autobadcol_f32.fits')
    fits.PrimaryHDU(f).writeto(pf, overwrite=True)
    return [p16, pf]


def ref_stdout(path, argv_extra):
    """The reference script's stdout with `path` replaced by PLACEHOLDER.  The non-default run gives the parsed values
    their types (the reference's argparse has no type= for --sigma / --window and fails on any user value)."""
    orig = ref_script.command_line_opts

    def typed(argv):
        a = orig(argv)
        a.sigma = float(a.sigma)
        a.window = int(a.window)
        return a
    ref_script.command_line_opts = typed if argv_extra else orig
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            rc = ref_script.main([path] + argv_extra)
    finally:
        ref_script.command_line_opts = orig
    assert rc == 0
    return buf.getvalue().replace(path, PLACEHOLDER)


def main():
    arrs = {}
    names = []
    stored = {}                             # one input shared by several cases is stored once (`data_from`)
    for name, data, w in cases():
        r = ref_case(data, w, 5.0)
        names.append(name)
        if id(data) in stored:
            arrs[name + '/data_from'] = np.array(stored[id(data)])
        else:
            stored[id(data)] = name
            arrs[name + '/data'] = data
        arrs[name + '/window'] = np.array(w)
        arrs[name + '/nsigma'] = np.array(5.0)
        for k, v in r.items():
            arrs[name + '/' + k] = v
    arrs['_cases'] = np.array(json.dumps(names))

    rng = np.random.default_rng(1313)
    paths = fits_fixtures(rng)
    runs = []
    for p in paths:
        for extra in ([], ['--sigma', '4', '--window', '7']):
            runs.append(dict(file=os.path.basename(p), argv=extra, stdout=ref_stdout(p, extra)))

    # the reference's CPU time for one 4096^2 float32 frame (process(), end to end)
    frame = sky(np.random.default_rng(4096), 4096, 4096)
    ab = ap.ApAutoBadcols('CRITICAL')
    t0 = time.perf_counter()
    ab.process(frame)
    dt = time.perf_counter() - t0
    meta = dict(placeholder=PLACEHOLDER, runs=runs,
                reference_cpu_seconds_4096x4096_f32=round(dt, 2),
                reference_cpu_note='ApAutoBadcols.process on one 4096x4096 float32 frame, single run, measured on the '
                                   'CPU of the container that generated these fixtures (numpy %s, astropy %s)'
                                   % (mg.VERSIONS['numpy'], mg.VERSIONS['astropy']))
    arrs['_meta'] = np.array(json.dumps(meta))
    # the four 640-value cases (both numpy median paths) go to a second archive: one file would pass the 1 MiB limit
    big = [n for n in names if '640' in n]
    second = {k: v for k, v in arrs.items() if k.split('/')[0] in big}
    second['_cases'] = np.array(json.dumps(big))
    first = {k: v for k, v in arrs.items() if k not in second}
    first['_cases'] = np.array(json.dumps([n for n in names if n not in big]))
    mg.save('g13_autobadcol.npz', **first)
    mg.save('g13_autobadcol_paths.npz', **second)
    print('reference CPU time for one 4096^2 f32 frame: %.2f s' % dt)


if __name__ == '__main__':
    main()
