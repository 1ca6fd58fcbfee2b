#!/usr/bin/env python3
"""ap_find_stars - detect the stars of a FITS image and write their positions and aperture photometry to a FITS table
(reference: scripts/ap_find_stars.py).

By default the script does ONE source search, at --search_fwhm.  With --fit_fwhm (implied by --quality_report) it follows the
reference: Gaussians are fitted to a sample of the stars (ApMeasureStars), the search and the photometry are repeated at the
measured FWHM, and the quality report is written.  The plots are not provided: --plotfile and --fwhm_plot are accepted and a
warning says that nothing is written."""
import argparse
import logging


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_find_stars',
                                     description=('Detects stars within a FITS image and performs aperture photometry on them, '
                                                  'writing the source list to a FITS table. One search is made, at '
                                                  '--search_fwhm, unless --fit_fwhm or --quality_report asks for the FWHM to be '
                                                  'fitted and the search to be repeated at the measured value.'))
    parser.add_argument('fits_image', metavar='IN_IMAGE.FITS', help='Path/name of the FITS image to search for stars.')
    parser.add_argument('source_list', metavar='OUT_SRCLIST.FITS', help='Path/name of the output FITS table of sources.')
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    parser.add_argument('-e', '--fits_extension', default=0, type=int, metavar='EXT_NUM',
                        help='FITS extension number to read from. Default=0 (Primary)')
    parser.add_argument('-m', '--max_sources', default=None, type=int, metavar='NUM_SRCS',
                        help=('Limit output source list the brightest set of NUM_SRCS sources. This also applies to the ds9 '
                              'format region file, if any. Default: Output all the sources.'))
    def_search_fwhm = 3.0
    def_search_nsigma = 7.0
    def_bitdepth = 16
    def_sat_frac = 0.80
    parser.add_argument('--search_fwhm', default=def_search_fwhm, type=float,
                        help=f'Source search FWHM (pixels). Default: {def_search_fwhm}')
    parser.add_argument('--search_nsigma', default=def_search_nsigma, type=float,
                        help=('Source search threshold in numbers of sigma above the background (standard deviations). '
                              f'Default: {def_search_nsigma}'))
    parser.add_argument('--bitdepth', default=def_bitdepth, type=int,
                        help=f'Detector bitdepth used in saturation calculation. Default: {def_bitdepth}')
    parser.add_argument('--sat_frac', default=def_sat_frac, type=float,
                        help=f'Fraction of max ADU used in saturation calculation. Default: {def_sat_frac}')
    parser.add_argument('--retain_saturated', action='store_true',
                        help=('Do not exclude possibly saturated stars from the source list. By default pixels within a box of '
                              'width 8x search_fwhm centered on possibly saturated stars are excluded from source detection '
                              'and fitting.'))
    parser.add_argument('--plotfile', default=None, metavar='IMG_WITH_SRCS.PNG', help='Accepted; no plot is produced.')
    parser.add_argument('--fit_fwhm', action='store_true', default=False,
                        help=('Fit 2-D Gaussians to a sample of the stars, then repeat the search and the photometry at the '
                              'measured FWHM.'))
    parser.add_argument('--quality_report', default=None, metavar='QUALITY_REPORT.TXT',
                        help='Name for the optional YAML image quality report (seeing, PSF circularity). Implies --fit_fwhm.')
    parser.add_argument('--fwhm_plot', default=None, metavar='FWHM_FITS.PNG', help='Accepted; no plot is produced.')
    parser.add_argument('-d', '--ds9', default=None, metavar='ds9.reg', help='Name for optional ds9-format region file.')
    parser.add_argument('-q', '--quiet', action='store_true', default=False,
                        help='Quiet mode suppresses the printing of the detected source lists to STDOUT while running.')
    return parser.parse_args(argv)


def main(args=None):
    p_args = command_line_opts(args)
    import astrophotography_amd as ap
    log = logging.getLogger('ap_find_stars')
    for flag, val in (('--plotfile', p_args.plotfile), ('--fwhm_plot', p_args.fwhm_plot)):
        if val is not None:
            log.warning('%s %s: not produced (plots are not provided).', flag, val)
    find_stars = ap.ApFindStars(p_args.fits_image, p_args.fits_extension, p_args.search_fwhm, p_args.search_nsigma, p_args.bitdepth,
                                p_args.max_sources, p_args.retain_saturated, p_args.sat_frac, p_args.loglevel, None, p_args.quiet)
    if p_args.fit_fwhm or p_args.quality_report is not None:
        new_fwhm, _, num_used = find_stars.measure_fwhm(None)
        if not num_used or not new_fwhm > 0:
            raise RuntimeError('No star could be fitted: the FWHM was not measured.')
        from astrophotography_amd import ops
        radius = ops.daofind_kernel(new_fwhm)['R']
        if radius > ops.DAOFIND_MAX_RADIUS:
            raise RuntimeError(f'The measured FWHM of {new_fwhm:.2f} pixels needs a search kernel of radius {radius}, above the '
                               f'star finder\'s limit of {ops.DAOFIND_MAX_RADIUS}.')
        find_stars.source_search(new_fwhm, p_args.search_nsigma)
        find_stars.aperture_photometry()
    if p_args.ds9 is not None:
        find_stars.write_ds9_region_file(p_args.ds9)
    find_stars.write_source_list(p_args.source_list)
    if p_args.quality_report is not None:
        find_stars.write_quality_report(p_args.quality_report)
    return 0


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
