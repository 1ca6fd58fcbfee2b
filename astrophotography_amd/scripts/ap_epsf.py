#!/usr/bin/env python3
"""ap_epsf - the empirical PSF of an image from its own stars, PSF-fitting photometry with it, and the image with the stars removed
(ApEmpiricalPsf):

    ap_find_stars image.fits stars.fits
    ap_epsf image.fits stars.fits psf.fits --photometry phot.fits --residual nostars.fits
    ap_deconvolve image.fits sharp.fits --psf psf.fits

PSF.FITS holds the ePSF's stamp at pixel spacing in its primary HDU (odd, square, sum 1) and the oversampled grid in the extension
EPSF.  PHOT.FITS is the star list's AP_L1MAG table plus flux_fit, x_fit, y_fit, sky_fit, chi2 and fit_ok.  The exit status is 0
(done), 1 (bad input) or 2 (fewer than 3 usable stars)."""
import argparse
import logging
import os


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_epsf', description='Build an empirical PSF from the stars of an image; fit and remove the stars with it.')
    parser.add_argument('inp_image', help='Input FITS image.')
    parser.add_argument('source_list', help='Input FITS table of the stars found by ap_find_stars (extension AP_L1MAG).')
    parser.add_argument('psf_file', help='Output FITS file of the PSF: the stamp (primary) and the oversampled grid (extension EPSF).')
    parser.add_argument('--photometry', default=None, metavar='PHOT.FITS', help='Write the PSF-fitting photometry of every star to this table.')
    parser.add_argument('--residual', default=None, metavar='RES.FITS', help='Write the image with the fitted stars removed.')
    parser.add_argument('--model', default=None, metavar='MODEL.FITS', help='Write the image of the fitted stars.')
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    parser.add_argument('--oversampling', default=4, type=int, help='Grid nodes per pixel, 1 .. 4. Default: 4')
    parser.add_argument('--radius', default=12, type=int, metavar='PIXELS', help='Radius of the PSF stamp, 2 .. 32. Default: 12')
    parser.add_argument('--fit_radius', default=None, type=float, metavar='PIXELS', help='Radius of the fits. Default: max(2, the FWHM in the source list)')
    parser.add_argument('--max_stars', default=500, type=int, help='The ePSF is built from at most this many of the brightest isolated stars. Default: 500')
    parser.add_argument('--niter', default=8, type=int, help='Rounds of the build. Default: 8')
    parser.add_argument('--smoothing', default='quartic', choices=['quartic', 'quadratic', 'none'], help='5 x 5 smoothing of every update. Default: quartic')
    parser.add_argument('--fit_sky', default=False, action='store_true', help='Fit the local sky of every star as well.')
    parser.add_argument('--passes', default=1, type=int, choices=[1, 2], help='2: fit every star again with the others removed. Default: 1')
    parser.add_argument('--gain_keyword', default=None, metavar='KEY', help='Header card of the gain (e-/ADU): weigh the fits by the noise model 1 / (readnoise^2 + model / gain). Give --readnoise with it: '
                             'with a read noise of 0 a star with a pixel whose model is <= 0 is refused (fit_ok false).')
    parser.add_argument('--readnoise', default=0.0, type=float, metavar='ADU', help='Read noise of the noise model. Default: 0')
    return parser.parse_args(argv)


def main(args=None):
    p = command_line_opts(args)
    from astrophotography_amd.core.ApEmpiricalPsf import BAD_INPUT, ApEmpiricalPsf
    log = logging.getLogger('ap_epsf')
    for name in (p.inp_image, p.source_list):
        if not os.path.isfile(name):
            log.error('ap_epsf: cannot find %s' % name)
            return BAD_INPUT
    try:
        ep = ApEmpiricalPsf(loglevel=p.loglevel, oversampling=p.oversampling, radius=p.radius, fit_radius=p.fit_radius, max_stars=p.max_stars,
                            niter=p.niter, smoothing=p.smoothing, fit_sky=p.fit_sky, gain_keyword=p.gain_keyword, readnoise=p.readnoise)
        out = ep.run_files(p.inp_image, p.source_list, p.psf_file, phot_file=p.photometry, residual_file=p.residual, model_file=p.model,
                           passes=p.passes)
    except (ValueError, OSError, KeyError) as exc:                          # a bad argument, a missing file, a list without the table
        log.error('ap_epsf: %s' % (exc,))
        return BAD_INPUT
    return out['status']


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
