#!/opt/conda/bin/python3.9 -B
"""Golden group G16: the annulus statistic of ApFindStars.aperture_photometry (core/ApFindStars.py:384-388), computed by astropy.

RUN ONLY IN THE BUILD CONTAINER:   /opt/conda/bin/python3.9 -B tests/golden/make_golden_findstars.py

photutils is absent, astropy (4.3.1) is not.  Of the star finder only this is astropy's own arithmetic:
    _, median_sigclip, _ = sigma_clipped_stats(annulus_data_1d)        (sigma 3, maxiters 5, median centre, std)
on the float32 values of the annulus pixels, a 1-D array (axis=None: astropy's _sigmaclip_noaxis, numpy's float32 reductions).
This script runs that call on annulus-like sample vectors - sky noise, a neighbouring star's wing, NaN / inf entries, all values
equal, two values only, 12 to about 1100 values - and records the inputs and astropy's (mean, median, std);
tests/test_findstars_model_host.py holds tests/findstars_model.annulus_clip to them and tests/test_gpu_findstars.py the HIP
kernel.  The values are stored in the archive: nothing depends on a random stream being the same under two interpreters.

It also writes a small source table with the project's own FITS table writer, opens it with astropy.io.fits and records what
astropy reads (column names, formats, values): the structure check of fitsio.write_table.
"""
import importlib.util
import json
import os
import sys
import tempfile
import warnings

warnings.filterwarnings('ignore')
import numpy as np

for nm, fn in [('asscalar', lambda a: a.item()), ('alen', len), ('msort', lambda a: np.sort(a, axis=0)),
               ('product', np.prod), ('cumproduct', np.cumprod), ('sometrue', np.any), ('alltrue', np.all),
               ('float', float), ('int', int), ('bool', bool), ('object', object), ('complex', complex), ('str', str)]:
    if not hasattr(np, nm):
        setattr(np, nm, fn)
import astropy
import astropy.stats.sigma_clipping as sc
sc.HAS_BOTTLENECK = False
from astropy.io import fits
from astropy.stats import sigma_clipped_stats

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def annulus(rng, n, sky, noise, quant=None):
    v = rng.normal(sky, noise, n)
    if quant:
        v = np.rint(v / quant) * quant
    return v


def main():
    rng = np.random.default_rng(1601)
    cases = []

    def add(name, v):
        cases.append((name, np.asarray(v, np.float32)))

    # annulus sizes of r = 6 .. 24 (fwhm 3 .. 12), whole and cut by an image edge
    for n in (12, 13, 40, 127, 128, 129, 150, 151, 260, 600, 601, 1004, 1100):
        add('sky_%d' % n, annulus(rng, n, 300.0, 6.0))
    for n in (150, 1004):
        add('sky_quant_%d' % n, annulus(rng, n, 300.0, 6.0, quant=0.125))          # ties
    for n, amp in ((150, 400.0), (260, 3000.0), (1004, 20000.0)):                  # a neighbouring star's wing in the annulus
        v = annulus(rng, n, 300.0, 6.0)
        k = n // 9
        v[5:5 + k] += amp * np.exp(-0.5 * (np.arange(k) / (0.3 * k)) ** 2)
        add('wing_%d' % n, v)
    v = annulus(rng, 150, 300.0, 6.0)
    v[[3, 77, 149]] = np.nan
    add('nan_150', v)
    v = annulus(rng, 260, -4.0, 2.0)
    v[[0, 100]] = [np.inf, -np.inf]
    v[50] = np.nan
    add('nonfinite_260_negative_sky', v)
    add('all_nan_12', np.full(12, np.nan))
    add('all_equal_150', np.full(150, 123.25))
    add('all_equal_but_one_151', np.r_[np.full(150, 123.25), 9000.0])
    add('two_values', [10.0, 11.5])
    add('two_levels_128', np.r_[np.full(64, 5.0), np.full(64, 9.0)])
    add('one_value', [42.0])
    add('three_values_outlier', [1.0, 1.0, 1.0e6])
    v = annulus(rng, 600, 1000.37, 30.0)
    v[rng.random(600) < 0.05] -= 400.0                                             # low outliers
    add('low_outliers_600', v)
    add('sky_zero_mean_1004', annulus(rng, 1004, 0.0, 1.0))
    add('big_values_601', annulus(rng, 601, 60000.0, 250.0, quant=1.0))

    out, meta = {}, []
    for k, (name, v) in enumerate(cases):
        assert v.dtype == np.float32 and v.ndim == 1
        mean, median, std = sigma_clipped_stats(v)
        out['c%d_values' % k] = v
        out['c%d_stats' % k] = np.array([mean, median, std], np.float64)
        meta.append(dict(case=k, name=name, n=int(v.size), stat_dtype=str(np.asarray(median).dtype)))
        print('%-28s n=%4d  mean %-12r median %-12r std %r' % (name, v.size, mean, median, std))

    # ---- the FITS table written by the project, read by astropy ----
    spec = importlib.util.spec_from_file_location('ap_fitsio', os.path.join(ROOT, 'astrophotography_amd', 'fitsio.py'))
    fio = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fio)
    cols = {'id': np.arange(1, 6, dtype=np.int32), 'xcenter': np.linspace(1.5, 99.25, 5), 'ycenter': np.linspace(7.0, 55.5, 5),
            'aperture_sum': np.array([1e5, 2.5e4, 300.125, -4.0, np.nan]), 'peak_adu': np.arange(5, dtype=np.float32) * 100.5,
            'psbl_sat': np.array([True, False, False, True, False]), 'npix': np.array([25, 25, 121, 121, 2 ** 40], np.int64)}
    kw = {'IMG_FILE': ('frame.fits', 'Name of image file searched for stars'), 'AP_NDET': (5, 'Number of sources detected in the image.'),
          'AP_BGMED': (301.5, '[ADU] Median source-masked background level')}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'srclist.fits')
        fio.write_table(path, [('AP_XYPOS', {'X': cols['xcenter'] + 1.0, 'Y': cols['ycenter'] + 1.0}, {'X': 'pix', 'Y': 'pix'},
                                [('COMMENT', 'Uses FITS 1-based pixel coordinate system.')]),
                               ('AP_L1MAG', cols, {'xcenter': 'pix', 'ycenter': 'pix'}, None)], header=kw)
        with fits.open(path) as hl:
            hl.verify('exception')
            assert [h.name for h in hl] == ['PRIMARY', 'AP_XYPOS', 'AP_L1MAG'], [h.name for h in hl]
            assert hl[0].header['AP_NDET'] == 5 and hl[0].header['AP_BGMED'] == 301.5 and hl[0].header['IMG_FILE'] == 'frame.fits'
            t = hl['AP_L1MAG']
            names = list(t.columns.names)
            formats = [str(f) for f in t.columns.formats]
            assert names == list(cols), names
            for n in names:
                a, b = np.asarray(t.data[n]), cols[n]
                assert np.array_equal(a, b, equal_nan=(b.dtype.kind == 'f')), (n, a, b)
            assert t.columns['xcenter'].unit == 'pix'
            assert np.array_equal(hl['AP_XYPOS'].data['X'], cols['xcenter'] + 1.0)
        out['table_names'] = np.array(json.dumps(names))
        out['table_formats'] = np.array(json.dumps(formats))
        print('astropy reads the table:', names, formats)

    out['_meta'] = np.array(json.dumps(meta))
    out['_versions'] = np.array(json.dumps(dict(astropy=astropy.__version__, numpy=np.__version__, python=sys.version.split()[0],
                                                 bottleneck='disabled', photutils='absent: only the annulus statistic is astropy\'s')))
    path = os.path.join(HERE, 'g16_annulus.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 200000, size
    print('wrote g16_annulus.npz', len(meta), 'cases', size, 'bytes')


if __name__ == '__main__':
    main()
