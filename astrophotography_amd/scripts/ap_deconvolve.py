#!/usr/bin/env python3
"""ap_deconvolve - sharpens a finished co-add with its own PSF: damped Richardson-Lucy deconvolution on the GPU (ApDeconvolve;
DESIGN 4.3i).

    ap_deconvolve coadd.fits sharp.fits
    ap_deconvolve coadd.fits sharp.fits --psf moffat --beta 3 --fwhm 3.4 --niter 50 --damp 3 --readnoise 4.2

The FWHM is measured from the image's stars and the sky level from its clipped median unless given; pixels without data stay NaN.
The settings are logged and written to the output header (DCONPSF, DCONFWHM, ...); the result goes on to ap_composite."""
import argparse
import logging


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_deconvolve', description='Richardson-Lucy deconvolution of an image with a Gaussian, '
                                     'Moffat or given PSF.')
    parser.add_argument('input', metavar='INPUT.FITS', help='Image to sharpen (float32 co-add, NaN = no data).')
    parser.add_argument('output', metavar='OUTPUT.FITS', help='Output image (float32, overwritten).')
    parser.add_argument('--psf', default='gaussian', metavar='gaussian|moffat|FILE.FITS',
                        help='PSF model, or a FITS file with an odd, square PSF stamp (normalised to sum 1). Default: gaussian')
    parser.add_argument('--fwhm', default=None, type=float, help='FWHM of the PSF in pixels. Default: measured from the stars of the image.')
    parser.add_argument('--beta', default=2.5, type=float, help='Exponent of the Moffat profile. Default: 2.5')
    parser.add_argument('--radius', default=None, type=int,
                        help='Radius of the PSF stamp in pixels, at most 12. Default: ceil(1.7 FWHM) (gaussian), ceil(2.5 FWHM) (moffat)')
    parser.add_argument('--niter', default=30, type=int, help='Number of iterations. Default: 30')
    parser.add_argument('--damp', default=0.0, type=float,
                        help='Damping threshold in sigma: residuals below it are left alone (noise is not sharpened). Default: 0 (none)')
    parser.add_argument('--sky', default=None, type=float, help='Sky level in ADU, held out of the deconvolution. Default: the clipped median')
    parser.add_argument('--gain_keyword', default='EGAIN', metavar='KEYWORD',
                        help='Header keyword with the gain in e-/ADU (used by the damping). Default: EGAIN')
    parser.add_argument('--readnoise', default=0.0, type=float, help='Read noise in ADU (used by the damping). Default: 0')
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    return parser.parse_args(argv)


def main(args=None):
    p = command_line_opts(args)
    from astrophotography_amd.core.ApDeconvolve import ApDeconvolve
    dc = ApDeconvolve(p.loglevel, psf=p.psf, beta=p.beta, radius=p.radius, niter=p.niter, damp=p.damp, readnoise=p.readnoise,
                      gain_keyword=p.gain_keyword)
    dc.deconvolve_files(p.input, p.output, fwhm=p.fwhm, sky=p.sky)
    return 0


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
