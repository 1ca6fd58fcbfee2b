#!/opt/conda/bin/python3.9 -B
"""Golden group G17: the Gaussian PSF fits of ApMeasureStars (core/ApMeasureStars.py), computed by the reference class itself.

RUN ONLY IN THE BUILD CONTAINER:   /opt/conda/bin/python3.9 -B tests/golden/make_golden_measurestars.py

ApMeasureStars needs astropy.modeling and scipy (both present: astropy 4.3.1) and imports photutils and regions without
using them: those two get stub modules.  Synthetic float32 frames of integer-valued Poisson counts and hand-made photometry
tables go through the class (fwhm_plot_file=None, quiet=True); the frame, the input tables, the whole result table, the fitted
background level (read from the fitted model by wrapping _do_single_fit: the class does not keep it) and median_fwhm for
'both', 'x' and 'y' are stored.

How far astropy's end point is from the minimum is measured, not assumed: every fit is polished by
scipy.optimize.least_squares(method='lm', jac='3-point', xtol=ftol=gtol=1e-15) and compared in the canonical form
(A, x, y, sigma_major, sigma_minor, theta_major mod pi, B) - the model does not change under (sx, sy, th) -> (sy, sx, th +- pi/2)
nor under th -> th + pi.  The maxima over the group go into _meta: d_par (|astropy - polished| / astropy's error), the relative
chi^2 difference, and the distance from 1 of the ratio of astropy's errors to those of the 3-point Jacobian at the polished
point.  The tests derive their bounds from these numbers.

astropy (4.3.1, LevMarLSQFitter) scales the covariance by chi^2 / (len(y) - n_free) and len(y) of the 2-D grid is its number
of rows: the reference's errors are those of dof = box_width - n_free, not box_width^2 - n_free.  The polished errors use the same
scaling, so the recorded ratio compares like with like.  The frames are stored as int32 counts (the class gets them as float32).
"""
import importlib
import io
import json
import math
import os
import sys
import types
import warnings
from contextlib import redirect_stdout

warnings.filterwarnings('ignore')
import numpy as np

for nm, fn in [('asscalar', lambda a: a.item()), ('alen', len), ('msort', lambda a: np.sort(a, axis=0)),
               ('product', np.prod), ('cumproduct', np.cumprod), ('sometrue', np.any), ('alltrue', np.all),
               ('float', float), ('int', int), ('bool', bool), ('object', object), ('complex', complex), ('str', str)]:
    if not hasattr(np, nm):
        setattr(np, nm, fn)


class _Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith('__'):
            raise AttributeError(k)
        return _Stub(self.__name__ + '.' + k)


for m in ['photutils', 'regions', 'matplotlib', 'matplotlib.pyplot', 'matplotlib.patches', 'yaml']:
    try:
        importlib.import_module(m)
    except Exception:
        sys.modules[m] = _Stub(m)

import astropy
import scipy
import astropy.stats.sigma_clipping as sc
sc.HAS_BOTTLENECK = False
from astropy.table import Table
from scipy.optimize import least_squares

# the class's own file, not the package: the package's __init__ imports every class and their third-party modules
import importlib.util
_spec = importlib.util.spec_from_file_location('ref_ApMeasureStars', '/root/reference/AstroPhotography/core/ApMeasureStars.py')
ams = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ams)
ApMeasureStars = ams.ApMeasureStars

HERE = os.path.dirname(os.path.abspath(__file__))
S2F = 2.35482
PHOT_COLS = ('id', 'xcenter', 'ycenter', 'aperture_sum', 'peak_adu', 'psbl_sat', 'bgmed_per_pix', 'adu_per_sec', 'magnitude')
RESULT_FLOAT = ('xcenter', 'ycenter', 'peak_adu', 'bgmed_per_pix', 'magnitude', 'nn_dist', 'dx', 'dy', 'radius', 'xmin', 'xmax', 'ymin',
                'ymax', 'xc_fit', 'xc_err', 'yc_fit', 'yc_err', 'ampl', 'ampl_err', 'fwhm_x', 'fwhm_x_err', 'fwhm_y', 'fwhm_y_err',
                'theta', 'theta_err', 'axrat', 'axrat_err', 'rchisq')
RESULT_COLS = RESULT_FLOAT + ('circular', 'fit_ok', 'bg_fit', 'bg_err', 'nfev_last')

# the fitted models of the run in progress, one per star index (the last call per star is the last stage run)
_captured = {}
_orig_single_fit = ApMeasureStars._do_single_fit


def _capturing_single_fit(self, fitter, input_mod, data_arr, weights_arr, x_grid, y_grid, max_iterations, index):
    out = _orig_single_fit(self, fitter, input_mod, data_arr, weights_arr, x_grid, y_grid, max_iterations, index)
    std = out[0][1].amplitude.std
    _captured[index] = (float(out[0][1].amplitude.value), float(std) if (out[3] and std is not None) else 0.0,
                        int(fitter.fit_info['nfev']))
    return out


ApMeasureStars._do_single_fit = _capturing_single_fit


def star(x, y, ampl, fwhm, ratio=1.0, angle=0.0, sat=False, in_srclist=True, name=None):
    return dict(x=float(x), y=float(y), ampl=float(ampl), fwhm=float(fwhm), ratio=float(ratio), angle=float(angle), sat=bool(sat),
                in_srclist=bool(in_srclist), name=name)


def render(H, W, bg, stars, rng, subtract_sky):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.full((H, W), float(bg))
    for s in stars:
        smaj = s['fwhm'] / S2F
        smin = smaj / s['ratio']
        c, sn = math.cos(s['angle']), math.sin(s['angle'])
        u = (xx - s['x']) * c + (yy - s['y']) * sn
        v = -(xx - s['x']) * sn + (yy - s['y']) * c
        img += s['ampl'] * np.exp(-0.5 * (u * u / smaj ** 2 + v * v / smin ** 2))
    counts = rng.poisson(img).astype(np.float64)
    if subtract_sky:
        counts -= float(int(bg))
    return counts.astype(np.float32)


def tables(stars, bg_table, rng):
    """The photometry tables of ApFindStars, by hand: brightest first, ids in that order."""
    rows = []
    for s in stars:
        smaj = s['fwhm'] / S2F
        flux = 2.0 * math.pi * s['ampl'] * smaj * smaj / s['ratio']
        rows.append(dict(xcenter=s['x'] + rng.uniform(-0.15, 0.15), ycenter=s['y'] + rng.uniform(-0.15, 0.15), aperture_sum=flux,
                         peak_adu=s['ampl'] * rng.uniform(0.85, 1.1), psbl_sat=s['sat'],
                         bgmed_per_pix=bg_table + rng.uniform(-1.0, 1.0), adu_per_sec=flux / 30.0,
                         magnitude=-2.5 * math.log10(flux / 30.0), in_srclist=s['in_srclist'], name=s['name']))
    rows.sort(key=lambda r: -r['adu_per_sec'])
    for k, r in enumerate(rows):
        r['id'] = k + 1
    full = {c: np.array([r[c] for r in rows]) for c in PHOT_COLS}
    keep = np.array([r['in_srclist'] for r in rows], bool)
    src = {c: v[keep] for c, v in full.items()}
    names = {r['name']: r['id'] for r in rows if r['name']}
    return src, full, names


def weights_of(cut):
    """ApMeasureStars.py:319-329, as the class computes them (float32 arithmetic of a float32 cut-out)."""
    var_arr = np.where(cut > 0, cut, 1)
    mean_variance = np.mean(var_arr[var_arr != 1])
    rms_stddev = math.sqrt(mean_variance)
    std_arr = np.where(var_arr != 1, np.sqrt(var_arr), rms_stddev)
    return 1.0 / std_arr, std_arr


def gauss(p, xg, yg):
    A, xm, ym, sx, sy, th, B = p
    cost2, sint2, sin2t = math.cos(th) ** 2, math.sin(th) ** 2, math.sin(2.0 * th)
    a = 0.5 * (cost2 / sx ** 2 + sint2 / sy ** 2)
    b = 0.5 * (sin2t / sx ** 2 - sin2t / sy ** 2)
    c = 0.5 * (sint2 / sx ** 2 + cost2 / sy ** 2)
    dx, dy = xg - xm, yg - ym
    return A * np.exp(-(a * dx * dx + b * dx * dy + c * dy * dy)) + B


def canonical(p, e=None):
    """(A, x, y, sx, sy, th, B) -> (A, x, y, s_major, s_minor, th_major mod pi, B); the errors follow their parameters."""
    A, xm, ym, sx, sy, th, B = p
    sx, sy = abs(sx), abs(sy)
    ex, ey = (e[3], e[4]) if e is not None else (0.0, 0.0)
    if sy > sx:
        sx, sy, ex, ey, th = sy, sx, ey, ex, th + 0.5 * math.pi
    th = th % math.pi
    out = np.array([A, xm, ym, sx, sy, th, B])
    if e is None:
        return out
    return out, np.array([e[0], e[1], e[2], ex, ey, e[5], e[6]])


def angle_diff(a, b):
    d = (a - b) % math.pi
    return min(d, math.pi - d)


def run_case(name, H, W, init_fwhm, bg, stars, seed, subtract_sky=False, ones=0):
    rng = np.random.default_rng(seed)
    img = render(H, W, bg, stars, rng, subtract_sky)
    if ones:                                     # some pixels exactly 1: the class takes them for "no variance"
        for s in stars[:ones]:
            img[int(round(s['y'])) + 4, int(round(s['x'])) - 3] = 1.0
    bg_table = 0.0 if subtract_sky else float(bg)
    src, full, names = tables(stars, bg_table, rng)
    assert np.array_equal(img, np.rint(img))
    out = {'img_counts': img.astype(np.int16 if subtract_sky else np.uint16), 'init_fwhm': np.float64(init_fwhm), 'init_bglevel': np.float64(bg_table)}
    out['src_table'] = np.column_stack([np.asarray(src[c], np.float64) for c in PHOT_COLS])      # columns: PHOT_COLS (in _meta)
    out['full_table'] = np.column_stack([np.asarray(full[c], np.float64) for c in PHOT_COLS])
    meta = dict(name=name, shape=[H, W], init_fwhm=init_fwhm, named_stars=names, reference_raises=None, designed_failures=[])
    _captured.clear()
    try:
        with redirect_stdout(io.StringIO()):
            m = ApMeasureStars(img, Table(src), init_fwhm, bg_table, Table(full), None, None, 'CRITICAL', True)
    except Exception as exc:                     # no candidate survives: the class indexes None
        meta['reference_raises'] = type(exc).__name__
        meta['designed_failures'].append('%s: no candidate survives, the reference raises %s' % (name, type(exc).__name__))
        meta['n_fit'] = 0
        print('%-12s reference raises %s' % (name, type(exc).__name__))
        return out, meta, None
    t = m.results_table()
    n = len(t)
    meta['n_fit'] = n
    meta['box_width'] = int(m._box_width_pix)
    meta['edge_excl'] = int(m._edge_excl_pix)
    out['trim_id'] = np.asarray(m._init_srcs['id'], np.int64)
    out['trim_nn_dist'] = np.asarray(m._init_srcs['nn_dist'], np.float64)
    out['trim_region'] = np.array([str(r) for r in m._init_srcs['region']])
    out['res_id'] = np.asarray(t['id'], np.int64)
    out['res_region'] = np.array([str(r) for r in t['region']])
    res = {c: np.asarray(t[c], np.float64) for c in RESULT_FLOAT}
    res['circular'] = np.asarray(t['circular'], np.float64)
    res['fit_ok'] = np.asarray(t['fit_ok'], np.float64)
    res['bg_fit'] = np.array([_captured[i][0] for i in range(n)])
    res['bg_err'] = np.array([_captured[i][1] for i in range(n)])
    res['nfev_last'] = np.array([_captured[i][2] for i in range(n)], np.float64)
    out['res_table'] = np.column_stack([res[c] for c in RESULT_COLS])                              # columns: RESULT_COLS (in _meta)
    with redirect_stdout(io.StringIO()):
        for d in ('both', 'x', 'y'):
            out['median_fwhm_' + d] = np.array(m.median_fwhm(d), np.float64)
    ok = res['fit_ok'] != 0
    assert ok.sum() >= 0.9 * n, (name, int(ok.sum()), n)
    for i in np.nonzero(~ok)[0]:
        meta['designed_failures'].append('%s: star id %d is not fit_ok in the reference' % (name, int(t['id'][i])))

    # ---- astropy's distance from the minimum ----
    Wb = meta['box_width']
    xg, yg = np.mgrid[0:Wb, 0:Wb].astype(np.float64)
    stats = dict(d_par=0.0, d_chi2=0.0, d_err=0.0)
    pol = np.zeros((n, 7))
    for i in range(n):
        if not ok[i]:
            continue
        x0, y0 = int(t['xmin'][i]), int(t['ymin'][i])
        cut = img[y0:y0 + Wb, x0:x0 + Wb]
        w, _ = weights_of(cut)
        w = w.astype(np.float64)
        z = cut.astype(np.float64)
        p_ast = np.array([t['ampl'][i], t['xc_fit'][i] - x0, t['yc_fit'][i] - y0, t['fwhm_x'][i] / S2F, t['fwhm_y'][i] / S2F, t['theta'][i],
                          res['bg_fit'][i]])
        e_ast = np.array([t['ampl_err'][i], t['xc_err'][i], t['yc_err'][i], t['fwhm_x_err'][i] / S2F, t['fwhm_y_err'][i] / S2F,
                          t['theta_err'][i], res['bg_err'][i]])
        resid = lambda p: np.ravel(w * (gauss(p, xg, yg) - z))
        r = least_squares(resid, p_ast, method='lm', jac='3-point', xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
        pol[i] = r.x
        chi_a, chi_p = float(np.sum(resid(p_ast) ** 2)), float(np.sum(r.fun ** 2))
        cov = np.linalg.inv(r.jac.T @ r.jac) * chi_p / (Wb - 7)      # astropy's dof: len(y) of the 2-D grid, its row count
        e_pol = np.sqrt(np.diag(cov))
        ca, cea = canonical(p_ast, e_ast)
        cp, cep = canonical(r.x, e_pol)
        d = np.abs(ca - cp) / cea
        round_star = (ca[3] - ca[4]) < 3.0 * math.hypot(cea[3], cea[4])
        d[5] = 0.0 if round_star else angle_diff(ca[5], cp[5]) / cea[5]
        de = np.abs(cea / cep - 1.0)
        if round_star:
            de[5] = 0.0
        stats['d_par'] = max(stats['d_par'], float(d.max()))
        stats['d_chi2'] = max(stats['d_chi2'], abs(chi_a - chi_p) / chi_p)
        stats['d_err'] = max(stats['d_err'], float(de.max()))
    out['res_polished'] = pol
    meta.update(stats)
    print('%-12s n_fit %2d ok %2d  d_par %.2e  d_chi2 %.2e  d_err %.2e  median both %s' % (
        name, n, int(ok.sum()), stats['d_par'], stats['d_chi2'], stats['d_err'], np.round(out['median_fwhm_both'], 4)))
    return out, meta, t


def grid(xs, ys):
    return [(x, y) for y in ys for x in xs]


def main():
    cases = []
    shapes = [(1.0, 0.0), (1.2, 0.4), (1.5, 1.0), (1.3, 2.2), (1.0, 0.0), (1.5, 2.9), (1.1, 1.6)]

    # c0: init FWHM 3 (box 18, edge 10), 144 x 176: close pairs, the four edge limits, a possibly saturated star
    H, W, f = 144, 176, 3.3
    st = []
    amp = iter(np.geomspace(22000.0, 900.0, 64))
    k = 0
    for (x, y) in grid((31, 50, 69, 88, 107, 126, 145), (30, 51, 72, 93, 114)):
        if (x, y) in ((69, 51), (126, 93), (88, 72), (107, 72)):
            continue
        r, a = shapes[k % len(shapes)]
        st.append(star(x + 0.37 * ((k * 7) % 5 - 2) / 2, y + 0.41 * ((k * 3) % 5 - 2) / 2, next(amp), f, r, a))
        k += 1
    st.append(star(67.5, 51.0, 9000.0, f, name='pair_under_a'))          # 17.5 from the grid star at (50, 51): both trimmed
    st.append(star(125.5, 93.0, 9500.0, f, 1.2, 0.7, name='pair_over_a'))   # 18.5 from the grid star at (107, 93): both kept
    st.append(star(88.0, 72.0, 60000.0, f, sat=True, name='psbl_sat'))
    st.append(star(105.0, 72.0, 30000.0, f, name='neighbour_of_sat'))    # 17 from a star that is only in the full list
    st.append(star(8.7, 40.0, 40000.0, f, name='left_out'))
    st.append(star(9.3, 100.0, 41000.0, f, 1.3, 0.3, name='left_in'))
    st.append(star(165.3, 40.0, 42000.0, f, name='right_out'))
    st.append(star(164.7, 100.0, 43000.0, f, 1.2, 1.9, name='right_in'))
    st.append(star(60.0, 9.6, 44000.0, f, name='bottom_out'))
    st.append(star(120.0, 10.4, 45000.0, f, 1.4, 2.5, name='bottom_in'))
    st.append(star(60.0, 133.4, 46000.0, f, name='top_out'))
    st.append(star(120.0, 132.7, 47000.0, f, 1.1, 1.2, name='top_in'))
    st.append(star(150.0, 12.0, 300.0, f, in_srclist=False, name='faint_full_only'))
    cases.append(('c0_fwhm3', H, W, 3.0, 100.0, st, 1701, {}))

    # c1: init FWHM 1.5 (box 12, the minimum; edge 6): sharp stars
    st = []
    k = 0
    amp = iter(np.geomspace(30000.0, 1500.0, 80))
    for (x, y) in grid(range(14, 170, 16), range(14, 136, 16)):
        r, a = shapes[(k + 3) % len(shapes)]
        st.append(star(x + 0.45 * ((k * 7) % 5 - 2) / 2, y + 0.43 * ((k * 3) % 5 - 2) / 2, next(amp), 1.9, min(r, 1.3), a))
        k += 1
    cases.append(('c1_fwhm1p5', 144, 176, 1.5, 120.0, st, 1702, {}))

    # c2: init FWHM 5 (box 30, edge 16): regions with three candidates (TL, TR) and a region with none (BR)
    st = []
    k = 0
    amp = iter(np.geomspace(26000.0, 2500.0, 32))
    pos = [(88, 72), (110, 94), (110, 50),                                       # CN (radius 36)
           (30, 86), (30, 120), (62, 126),                                       # TL
           (146, 80), (146, 120), (112, 127),                                    # TR
           (28, 40), (62, 18), (58, 52)]                                         # BL (the last falls just inside CN)
    for (x, y) in pos:
        r, a = shapes[(k + 1) % len(shapes)]
        st.append(star(x + 0.3, y - 0.2, next(amp), 5.6, r, a))
        k += 1
    cases.append(('c2_fwhm5', 144, 176, 5.0, 100.0, st, 1703, {}))

    # c3: a sky-subtracted frame (background about 0: many pixels <= 0, some exactly 1)
    st = []
    k = 0
    amp = iter(np.geomspace(15000.0, 600.0, 40))
    for (x, y) in grid((31, 50, 69, 88, 107, 126, 145), (30, 51, 72, 93, 114)):
        r, a = shapes[(k + 5) % len(shapes)]
        st.append(star(x - 0.41 * ((k * 7) % 5 - 2) / 2, y + 0.39 * ((k * 3) % 5 - 2) / 2, next(amp), 3.0, r, a))
        k += 1
    cases.append(('c3_skysub', 144, 176, 3.0, 12.0, st, 1704, dict(subtract_sky=True, ones=12)))

    # c4: bright to faint: peak signal-to-noise from about 150 down to about 3 on a sky of 100 (noise 10)
    st = []
    k = 0
    amp = iter(np.geomspace(25000.0, 32.0, 25))
    for (x, y) in [(88, 72), (70, 60), (106, 84), (72, 92), (104, 50),
                   (30, 88), (52, 118), (22, 124), (70, 126), (44, 80),
                   (150, 88), (126, 118), (156, 124), (104, 126), (132, 78),
                   (150, 56), (126, 26), (156, 20), (100, 20), (132, 46),
                   (26, 56), (50, 26), (20, 22), (76, 22), (44, 48)]:
        r, a = shapes[k % len(shapes)]
        st.append(star(x + 0.25, y + 0.35, next(amp), 3.4, r, a))
        k += 1
    cases.append(('c4_faint', 144, 176, 3.0, 100.0, st, 1705, {}))

    # c5: a 12 x 12 frame corner: no candidate survives the edge limits
    cases.append(('c5_corner12', 12, 12, 1.5, 100.0, [star(5.6, 6.2, 5000.0, 1.9)], 1706, {}))

    out, metas = {}, []
    for k, (name, H, W, fw, bg, st, seed, kw) in enumerate(cases):
        o, meta, _ = run_case(name, H, W, fw, bg, st, seed, **kw)
        for key, v in o.items():
            out['c%d_%s' % (k, key)] = v
        meta['case'] = k
        metas.append(meta)
    fitted = [m for m in metas if m['n_fit']]
    summary = dict(cases=metas, phot_cols=list(PHOT_COLS), result_cols=list(RESULT_COLS),
                   d_par_max=max(m['d_par'] for m in fitted), d_chi2_max=max(m['d_chi2'] for m in fitted),
                   d_err_max=max(m['d_err'] for m in fitted),
                   designed_failures=[d for m in metas for d in m['designed_failures']],
                   versions=dict(astropy=astropy.__version__, numpy=np.__version__, scipy=scipy.__version__,
                                 python=sys.version.split()[0], bottleneck='disabled'))
    assert any(m['reference_raises'] for m in metas)
    out['_meta'] = np.array(json.dumps(summary))
    path = os.path.join(HERE, 'g17_measurestars.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('d_par_max %.3e  d_chi2_max %.3e  d_err_max %.3e' % (summary['d_par_max'], summary['d_chi2_max'], summary['d_err_max']))
    print('designed failures:', summary['designed_failures'])
    print('wrote g17_measurestars.npz', len(metas), 'cases', size, 'bytes')
    assert size < 200000, size


if __name__ == '__main__':
    main()
