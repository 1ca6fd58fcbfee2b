"""Host float64 helpers for the ApMeasureStars tests: the G17 archive as tables, the reference's weights, astropy's
Gaussian2D + Const2D with its analytic Jacobian, and the canonical form in which two fits are compared.

The model does not change under (sx, sy, theta) -> (sy, sx, theta +- pi/2) nor under theta -> theta + pi, so fits are compared as
(A, x, y, sigma_major, sigma_minor, theta_major mod pi, B)."""
import json
import math

import numpy as np

from tests.util import load_golden

S2F = 2.35482
_cache = {}


def golden():
    """(archive, meta): loaded once and shared; nothing in it is modified."""
    if 'g' not in _cache:
        g = load_golden('g17_measurestars.npz')
        _cache['g'] = ({k: g[k] for k in g.files}, json.loads(str(g['_meta'])))
    return _cache['g']


def case(k):
    """dict(img float32, src, full (dicts of columns), res (dict of columns or None), meta, init_fwhm, init_bglevel, medians)."""
    g, meta = golden()
    pc, rc = meta['phot_cols'], meta['result_cols']
    pre = 'c%d_' % k

    def table(a):
        t = {c: a[:, i].copy() for i, c in enumerate(pc)}
        t['id'] = t['id'].astype(np.int64)
        t['psbl_sat'] = t['psbl_sat'] != 0
        return t
    out = dict(img=g[pre + 'img_counts'].astype(np.float32), src=table(g[pre + 'src_table']), full=table(g[pre + 'full_table']),
               meta=meta['cases'][k], init_fwhm=float(g[pre + 'init_fwhm']), init_bglevel=float(g[pre + 'init_bglevel']), res=None)
    if pre + 'res_table' in g:
        a = g[pre + 'res_table']
        out['res'] = {c: a[:, i].copy() for i, c in enumerate(rc)}
        out['res']['id'] = g[pre + 'res_id']
        out['res']['region'] = g[pre + 'res_region']
        out['res']['fit_ok'] = out['res']['fit_ok'] != 0
        out['res']['circular'] = out['res']['circular'] != 0
        out['trim'] = dict(id=g[pre + 'trim_id'], nn_dist=g[pre + 'trim_nn_dist'], region=g[pre + 'trim_region'])
        out['medians'] = {d: g[pre + 'median_fwhm_' + d] for d in ('both', 'x', 'y')}
    return out


def fitted_cases():
    return [k for k, m in enumerate(golden()[1]['cases']) if m['n_fit']]


def weights_of(cut):
    """ApMeasureStars.py:319-329 in the arithmetic of a float32 cut-out: (weights, standard deviations), float32."""
    cut = np.asarray(cut, np.float32)
    var_arr = np.where(cut > 0, cut, np.float32(1))
    mean_variance = np.mean(var_arr[var_arr != 1])
    rms = np.float32(math.sqrt(mean_variance))
    std_arr = np.where(var_arr != 1, np.sqrt(var_arr), rms).astype(np.float32)
    return (np.float32(1.0) / std_arr), std_arr


def model_and_jacobian(p, Wb):
    """p = (A, x_mean, y_mean, sx, sy, theta, B): model [Wb, Wb] and Jacobian [7, Wb, Wb]; x is the ROW index."""
    A, xm, ym, sx, sy, th, B = p
    xg, yg = np.mgrid[0:Wb, 0:Wb].astype(np.float64)
    cost2, sint2, sin2t, cos2t = math.cos(th) ** 2, math.sin(th) ** 2, math.sin(2 * th), math.cos(2 * th)
    a = 0.5 * (cost2 / sx ** 2 + sint2 / sy ** 2)
    b = 0.5 * (sin2t / sx ** 2 - sin2t / sy ** 2)
    c = 0.5 * (sint2 / sx ** 2 + cost2 / sy ** 2)
    dx, dy = xg - xm, yg - ym
    E = np.exp(-(a * dx * dx + b * dx * dy + c * dy * dy))
    g = A * E
    J = np.stack([E, g * (2 * a * dx + b * dy), g * (b * dx + 2 * c * dy),
                  g * (cost2 * dx * dx + sin2t * dx * dy + sint2 * dy * dy) / sx ** 3,
                  g * (sint2 * dx * dx - sin2t * dx * dy + cost2 * dy * dy) / sy ** 3,
                  -g * (cos2t * (1 / sx ** 2 - 1 / sy ** 2) * dx * dy + b * (dy * dy - dx * dx)), np.ones_like(g)])
    return g + B, J


def gauss_newton_step(p, cut):
    """(the Gauss-Newton step at p, the standard errors there with astropy's scaling) for the weighted fit of the cut-out."""
    Wb = cut.shape[0]
    w, _ = weights_of(cut)
    w = w.astype(np.float64)
    m, J = model_and_jacobian(p, Wb)
    r = (w * (m - cut.astype(np.float64))).ravel()
    Jw = (J * w).reshape(7, -1)
    JtJ = Jw @ Jw.T
    step = -np.linalg.solve(JtJ, Jw @ r)
    err = np.sqrt(np.diag(np.linalg.inv(JtJ)) * (r @ r) / (Wb - 7))
    return step, err


def params(t, i, x0, y0):
    """Row i of a result table -> (p, e) in the cut-out frame, order (A, x_mean, y_mean, sx, sy, theta, B)."""
    p = np.array([t['ampl'][i], t['xc_fit'][i] - x0, t['yc_fit'][i] - y0, t['fwhm_x'][i] / S2F, t['fwhm_y'][i] / S2F, t['theta'][i],
                  t['bg_fit'][i]])
    e = np.array([t['ampl_err'][i], t['xc_err'][i], t['yc_err'][i], t['fwhm_x_err'][i] / S2F, t['fwhm_y_err'][i] / S2F,
                  t['theta_err'][i], t['bg_err'][i]])
    return p, e


def canonical(p, e):
    """-> (A, x, y, s_major, s_minor, theta_major mod pi, B), the errors following their parameters, and whether x and y
    were exchanged."""
    A, xm, ym, sx, sy, th, B = p
    sx, sy, ex, ey = abs(sx), abs(sy), e[3], e[4]
    swapped = sy > sx
    if swapped:
        sx, sy, ex, ey, th = sy, sx, ey, ex, th + 0.5 * math.pi
    return np.array([A, xm, ym, sx, sy, th % math.pi, B]), np.array([e[0], e[1], e[2], ex, ey, e[5], e[6]]), swapped


def angle_diff(a, b):
    d = (a - b) % math.pi
    return min(d, math.pi - d)
