#!/usr/bin/env python3
"""ap_auto_badcol - statistically bad columns and rows of a FITS image, printed as YAML that can be pasted into a user
bad-pixel file for ap_find_badpix --user_badpix (reference: scripts/ap_auto_badcol.py:35-116).

Deviation: --sigma and --window are parsed as float / int (the reference has no type= and fails on any user value)."""
import argparse
import logging
import sys


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_auto_badcol',
                                     description=('Attempts to automatically detect statistically bad columns and rows in a given '
                                                  'FITS image, reporting the output in a format that can be cut and pasted into a '
                                                  'user badpixel YaML file.'))
    parser.add_argument('fitsimage', metavar='FITSIMAGE.FITS',
                        help=('Path/name of input FITS image to look for bad columns or rows in. The image data is assumed to '
                              'be in the primary extension of the FITS file.'))
    p_sigma = 5.0
    p_window_len = 11
    parser.add_argument('--sigma', metavar='NSIGMA', default=p_sigma, type=float,
                        help=('Columns or rows are identified as being bad if the median pixel value is more than NSIGMA '
                              'standard deviations away from the locally determined average. '
                              f'Default: {p_sigma}'))
    parser.add_argument('--window', metavar='LENGTH', default=p_window_len, type=int,
                        help=('Size of the moving average window function used to generate the local estimate of the column '
                              f'or row value. Default value: {p_window_len}'))
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    return parser.parse_args(argv)


def format_report(fitsimg, sigma, window, badcols, badrows):
    """The script's stdout (:92-116): a comment line, then bad_columns / bad_rows as 1-based YAML lists."""
    lines = [f'# Auto bad columns from {fitsimg}, sigma={sigma}, window_len={window}']
    for key, what, idx in (('bad_columns', 'columns', badcols), ('bad_rows', 'rows', badrows)):
        if idx is None:
            lines.append(f'# No bad {what} detected.')
        elif len(idx) == 0:
            lines.append(key + ': {}')
        else:
            lines.append(key + ':')
            lines.extend(f'- {int(v) + 1:d}' for v in idx)         # FITS-like 1-based indexing
    return '\n'.join(lines) + '\n'


def main(args=None):
    p_args = command_line_opts(args)
    import astrophotography_amd as ap
    auto_badcols = ap.ApAutoBadcols(p_args.loglevel)
    badcols, badrows = auto_badcols.process_fits(p_args.fitsimage, p_args.sigma, p_args.window)
    sys.stdout.write(format_report(p_args.fitsimage, p_args.sigma, p_args.window, badcols, badrows))
    return 0


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
