#!/usr/bin/env python3
"""ap_continuum_subtract - the line emission of a narrow-band co-add: the continuum image is brought to the same PSF, scaled and
subtracted, on the GPU (ApContinuumSubtract).

    ap_continuum_subtract ha.fits r.fits line.fits
    ap_continuum_subtract ha.fits r.fits line.fits --method stars --stars r_stars.fits --fwhm 2.6,3.4

Both images must be on one pixel grid (ap_coadd --center/--pixelscale/--image_size); the result goes on to ap_composite.  The scale,
the offset and the residual of the stars are logged and written to the output header (CSUBSCAL, CSUBOFF, ...)."""
import argparse
import logging


def _fwhm_pair(text):
    try:
        a, b = (float(v) for v in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('expected NARROW,CONT (two numbers), got %r' % text) from None
    return a, b


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_continuum_subtract', description='Subtracts a PSF-matched, scaled continuum image from a '
                                     'narrow-band image: OUTPUT = NARROW - s CONTINUUM - b.')
    parser.add_argument('narrow', metavar='NARROW.FITS', help='Narrow-band image (float32 co-add, NaN = no data).')
    parser.add_argument('continuum', metavar='CONTINUUM.FITS', help='Continuum (broad-band) image on the same pixel grid.')
    parser.add_argument('output', metavar='OUTPUT.FITS', help='Output line image (float32, overwritten).')
    parser.add_argument('--method', default=None, choices=['stars', 'pixels'],
                        help='How the scale is found. stars: the clipped median flux ratio of the stars. pixels: a clipped straight-line '
                             'fit over all pixels. Default: stars when a star list is given, pixels otherwise.')
    parser.add_argument('--scale', default=None, type=float, help='Use this scale s instead of fitting it.')
    parser.add_argument('--offset', default=None, type=float, help='Use this offset b instead of fitting it.')
    parser.add_argument('--fwhm', default=None, type=_fwhm_pair, metavar='NARROW,CONT',
                        help='FWHM of the two images in pixels. Default: measured from the stars of each image.')
    parser.add_argument('--no_psf_match', default=False, action='store_true', help='Do not blur the sharper image. Default: False')
    parser.add_argument('--stars', default=None, metavar='LIST', help='Source list written by ap_find_stars, in the common grid.')
    parser.add_argument('--mask', default=None, metavar='FITS', help='Mask image: non-zero pixels take no part in the fit.')
    parser.add_argument('--sigma_lower', default=3.0, type=float, help='Lower clipping bound of the pixel fit in sigma. Default: 3.0')
    parser.add_argument('--sigma_upper', default=2.0, type=float,
                        help='Upper clipping bound in sigma (tighter: emission only adds). Default: 2.0')
    parser.add_argument('--maxiters', default=10, type=int, help='Most clipping rounds of the pixel fit. Default: 10')
    parser.add_argument('--satlevel', default=None, type=float, help='Stars whose list peak reaches this level are not used. Default: none')
    parser.add_argument('--matched_out', default=None, metavar='PREFIX',
                        help='Also write the PSF-matched images to PREFIX_narrow.fits and PREFIX_continuum.fits.')
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    return parser.parse_args(argv)


def main(args=None):
    p = command_line_opts(args)
    from astrophotography_amd.core.ApContinuumSubtract import ApContinuumSubtract
    cs = ApContinuumSubtract(p.loglevel, method=p.method, psf_match=not p.no_psf_match, sigma_lower=p.sigma_lower,
                             sigma_upper=p.sigma_upper, maxiters=p.maxiters, satlevel=p.satlevel)
    cs.subtract_files(p.narrow, p.continuum, p.output, fwhm=p.fwhm, stars=p.stars, mask_file=p.mask, scale=p.scale, offset=p.offset,
                      matched_out=p.matched_out)
    return 0


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
