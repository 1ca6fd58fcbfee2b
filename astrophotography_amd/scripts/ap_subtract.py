#!/usr/bin/env python3
"""ap_subtract - optimal image subtraction with a spatially varying kernel (ApSubtract):

    ap_subtract image.fits template.fits diff.fits --stars stars.fits

DIFF.FITS = IMAGE - (TEMPLATE convolved with the fitted kernel + the fitted background), both inputs on one pixel grid.  With a
narrow-band image and a continuum image, `ap_subtract ha.fits r.fits line.fits` is the spatially varying alternative to
ap_continuum_subtract.  The exit status is 0 (done), 1 (bad input) or 2 (no fit: fewer usable stamps than the spatial terms need)."""
import argparse
import logging
import os


def _floats(s):
    return [float(v) for v in s.split(',')]


def _ints(s):
    return [int(v) for v in s.split(',')]


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_subtract', description='Subtract a PSF-matched, scaled template from an image (Alard & Lupton kernel fit).')
    parser.add_argument('image', help='Input FITS image.')
    parser.add_argument('template', help='Input FITS template (reference epoch, or continuum image) on the same pixel grid.')
    parser.add_argument('diff', help='Output FITS difference image.')
    parser.add_argument('--stars', default=None, metavar='LIST', help='FITS table of stars found by ap_find_stars (extension AP_L1MAG). Default: search the template.')
    parser.add_argument('--convolve', default='template', choices=['template', 'image', 'auto'], help='The image the kernel convolves. Default: template')
    parser.add_argument('--radius', default=10, type=int, metavar='PIXELS', help='Kernel radius, 1 .. 15. Default: 10')
    parser.add_argument('--sigmas', default=[0.7, 1.5, 3.0], type=_floats, metavar='S1,S2,..', help='Widths of the basis Gaussians. Default: 0.7,1.5,3.0')
    parser.add_argument('--degrees', default=[6, 4, 2], type=_ints, metavar='D1,D2,..', help='Polynomial degree of each Gaussian. Default: 6,4,2')
    parser.add_argument('--kernel_degree', default=2, type=int, help='Degree of the kernel variation over the field, 0 .. 3. Default: 2')
    parser.add_argument('--bg_degree', default=1, type=int, help='Degree of the background, 0 .. 3. Default: 1')
    parser.add_argument('--stamp', default=15, type=int, metavar='PIXELS', help='Half-size of the stamps, 1 .. 15. Default: 15')
    parser.add_argument('--regions', default=[4, 4], type=_ints, metavar='NX,NY', help='Grid of regions the stamps are chosen in. Default: 4,4')
    parser.add_argument('--per_region', default=5, type=int, help='Stamps per region. Default: 5')
    parser.add_argument('--mask', default=None, metavar='MASK.FITS', help='Non-zero pixels refuse the stamps they fall in.')
    parser.add_argument('--gain_keyword', default=None, metavar='KEY', help='Header card of the gain (e-/ADU): weigh by the noise model. Give --readnoise with it.')
    parser.add_argument('--readnoise', default=0.0, type=float, metavar='ADU', help='Read noise of the noise model. Default: 0')
    parser.add_argument('--matched_out', default=None, metavar='MATCHED.FITS', help='Write the matched template (convolved, scaled, background added).')
    parser.add_argument('--kernel_out', default=None, metavar='KERNEL.FITS', help='Write the kernel at a 3 x 3 lattice of positions as a cube.')
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    return parser.parse_args(argv)


def main(args=None):
    p = command_line_opts(args)
    from astrophotography_amd import ops
    from astrophotography_amd.core.ApSubtract import BAD_INPUT, DONE, NO_FIT, ApSubtract
    log = logging.getLogger('ap_subtract')
    for name in (p.image, p.template, p.stars, p.mask):
        if name is not None and not os.path.isfile(name):
            log.error('ap_subtract: cannot find %s' % name)
            return BAD_INPUT
    try:
        if len(p.regions) != 2:
            raise ValueError('--regions takes NX,NY')
        sub = ApSubtract(loglevel=p.loglevel, sigmas=p.sigmas, degrees=p.degrees, radius=p.radius, kernel_degree=p.kernel_degree,
                         bg_degree=p.bg_degree, stamp=p.stamp, regions=p.regions, per_region=p.per_region, convolve=p.convolve,
                         gain_keyword=p.gain_keyword, readnoise=p.readnoise)
        sub.subtract_files(p.image, p.template, p.diff, stars=p.stars, mask_file=p.mask, matched_out=p.matched_out, kernel_out=p.kernel_out)
    except ops.SubtractNoFit as exc:
        log.error('ap_subtract: no fit: %s' % (exc,))
        return NO_FIT
    except (ValueError, OSError, KeyError, RuntimeError) as exc:            # a bad argument, a missing file, a list without the table, no measurable star
        log.error('ap_subtract: %s' % (exc,))
        return BAD_INPUT
    return DONE


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
