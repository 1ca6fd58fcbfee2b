#!/opt/conda/bin/python3.9 -B
"""Golden group G20: pixel <-> sky of RA---TAN-SIP / DEC--TAN-SIP headers, computed by astropy.wcs itself.

RUN ONLY IN THE BUILD CONTAINER:   /opt/conda/bin/python3.9 -B tests/golden/make_golden_sip.py

Three headers, SIP orders 2, 3 and 4, a few pixels of distortion 2000 px from CRPIX; the order-3 one also carries the inverse
polynomials AP / BP (a coarse fit made here: astrophotography_amd.wcs.SipWcs uses them as a starting point only).  Per header 200
pixel positions, their sky positions by all_pix2world, the positions all_world2pix(tolerance=1e-12, maxiter=50) gives back, and
astropy's own round-trip error (the floor of what the test can ask of the way back).  The archive holds header values, arrays and
versions: data from astropy, nothing else.
"""
import json
import os
import warnings

warnings.filterwarnings('ignore')
import numpy as np

for nm, fn in [('asscalar', lambda a: a.item()), ('alen', len), ('msort', lambda a: np.sort(a, axis=0)),
               ('product', np.prod), ('cumproduct', np.cumprod), ('sometrue', np.any), ('alltrue', np.all),
               ('float', float), ('int', int), ('bool', bool), ('object', object), ('complex', complex), ('str', str)]:
    if not hasattr(np, nm):
        setattr(np, nm, fn)
import astropy
from astropy.io import fits
from astropy.wcs import WCS

HERE = os.path.dirname(os.path.abspath(__file__))


def sip_terms(order, amplitude_px, rng, reach=2000.0):
    """{(p, q): coefficient} for 2 <= p + q <= order: each total degree adds about amplitude_px / (order - 1) at `reach` pixels."""
    terms = {}
    for t in range(2, order + 1):
        w = rng.uniform(-1.0, 1.0, size=t + 1)
        w *= amplitude_px / (order - 1) / np.abs(w).sum() / reach ** t
        for q in range(t + 1):
            terms[(t - q, q)] = float(w[q])
    return terms


def fit_inverse(a, b, order, half=2000.0):
    """AP / BP of `order` by least squares on a grid: u = U + AP(U, V) with U = u + A(u, v)."""
    g = np.linspace(-half, half, 41)
    u, v = [c.ravel() for c in np.meshgrid(g, g)]
    f = sum(c * u ** p * v ** q for (p, q), c in a.items())
    h = sum(c * u ** p * v ** q for (p, q), c in b.items())
    U, V = u + f, v + h
    keys = [(t - q, q) for t in range(order + 1) for q in range(t + 1)]
    D = np.stack([U ** p * V ** q for p, q in keys], axis=1)
    ap = np.linalg.lstsq(D, u - U, rcond=None)[0]
    bp = np.linalg.lstsq(D, v - V, rcond=None)[0]
    return {k: float(c) for k, c in zip(keys, ap)}, {k: float(c) for k, c in zip(keys, bp)}


def main():
    rng = np.random.default_rng(2020)
    base = [
        dict(CRPIX1=2048.5, CRPIX2=2048.5, CRVAL1=303.0272359, CRVAL2=38.3549333, CD1_1=-4.9e-4, CD1_2=1.2e-5, CD2_1=1.3e-5, CD2_2=4.95e-4),
        dict(CRPIX1=1900.0, CRPIX2=2200.25, CRVAL1=10.68, CRVAL2=-41.27, CD1_1=-2.4e-4, CD1_2=-5.4e-5, CD2_1=-5.4e-5, CD2_2=2.4e-4),
        dict(CRPIX1=2100.75, CRPIX2=1990.5, CRVAL1=359.9, CRVAL2=72.0, CD1_1=-3.2e-4, CD1_2=2.4e-4, CD2_1=2.4e-4, CD2_2=3.2e-4),
    ]
    out = dict(versions=json.dumps({'astropy': astropy.__version__, 'numpy': np.__version__}), ncases=len(base))
    for i, (c, order) in enumerate(zip(base, (2, 3, 4))):
        c = dict(c, CTYPE1='RA---TAN-SIP', CTYPE2='DEC--TAN-SIP', A_ORDER=order, B_ORDER=order)
        a, b = sip_terms(order, 4.0, rng), sip_terms(order, 3.0, rng)
        for (p, q), v in a.items():
            c['A_%d_%d' % (p, q)] = v
        for (p, q), v in b.items():
            c['B_%d_%d' % (p, q)] = v
        if order == 3:
            ap, bp = fit_inverse(a, b, order)
            c.update(AP_ORDER=order, BP_ORDER=order)
            for (p, q), v in ap.items():
                c['AP_%d_%d' % (p, q)] = v
            for (p, q), v in bp.items():
                c['BP_%d_%d' % (p, q)] = v
        h = fits.Header()
        for k, v in c.items():
            h[k] = v
        w = WCS(h)
        assert w.sip is not None
        pix = np.column_stack([rng.uniform(0, 4096, 200), rng.uniform(0, 4096, 200)])
        sky = w.all_pix2world(pix, 0)
        back = w.all_world2pix(sky, 0, tolerance=1e-12, maxiter=50)
        plain = w.wcs_pix2world(pix, 0)                                 # without the distortion: how much it moves the sky
        out['hdr%d' % i] = json.dumps(c)
        out['pix%d' % i], out['sky%d' % i], out['back%d' % i] = pix, sky, back
        out['roundtrip%d' % i] = float(np.abs(back - pix).max())
        shift = np.hypot((sky[:, 0] - plain[:, 0]) * np.cos(np.deg2rad(sky[:, 1])), sky[:, 1] - plain[:, 1]) / np.sqrt(abs(c['CD1_1'] * c['CD2_2'] - c['CD1_2'] * c['CD2_1']))
        out['distortion_px%d' % i] = float(shift.max())
        print('case %d: order %d, distortion up to %.2f px, astropy round trip %.2e px' % (i, order, shift.max(), np.abs(back - pix).max()))
    np.savez_compressed(os.path.join(HERE, 'g20_sip_wcs.npz'), **out)


if __name__ == '__main__':
    main()
