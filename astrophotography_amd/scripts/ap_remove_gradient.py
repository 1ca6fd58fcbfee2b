#!/usr/bin/env python3
"""ap_remove_gradient - removes the large-scale sky gradient (light pollution, moonlight, residual vignetting) of a finished co-add
on the GPU (ApRemoveGradient).

    ap_remove_gradient coadd.fits flat_sky.fits
    ap_remove_gradient coadd.fits flat_sky.fits --model tps --smoothing 0.3 --exclude 900,700,1500,1300 --background_out sky.fits
    ap_remove_gradient coadd.fits flat_sky.fits --samples my_samples.yml --mode divide

The sky is sampled by the sigma-clipped median of small boxes away from the sources, a polynomial or a thin-plate spline is fitted to
the samples (those on an object are rejected) and subtracted from, or divided into, the image.  The result goes on to
ap_continuum_subtract, ap_deconvolve, ap_multiscale and ap_composite."""
import argparse
import logging


def _rect(text):
    try:
        x0, y0, x1, y1 = (float(v) for v in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('expected x0,y0,x1,y1 (four numbers), got %r' % text) from None
    return x0, y0, x1, y1


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_remove_gradient', description='Fits a smooth surface to the sky background of an image and '
                                     'subtracts it (or divides by it).')
    parser.add_argument('input', metavar='IN.FITS', help='Input image (float32 co-add, NaN = no data).')
    parser.add_argument('output', metavar='OUT.FITS', help='Output image (float32, overwritten).')
    parser.add_argument('--model', default='poly', choices=['poly', 'tps'],
                        help='Surface model: a polynomial in x and y, or a smoothing thin-plate spline through the samples. Default: poly')
    parser.add_argument('--degree', default=3, type=int, help='Total degree of the polynomial, 1 to 6. Default: 3')
    parser.add_argument('--smoothing', default=0.1, type=float,
                        help='Smoothing of the thin-plate spline: 0 interpolates the samples, large values tend to a plane. Default: 0.1')
    parser.add_argument('--samples_per_row', default=16, type=int,
                        help='Columns of the automatic grid of samples; the rows have the same pitch. Default: 16')
    parser.add_argument('--box_radius', default=12, type=int, help='Half-size of a sample box in pixels, 0 to 32. Default: 12')
    parser.add_argument('--samples', default=None, metavar='FILE.YML',
                        help='Use the samples of this file (x, y per sample; what --samples_out writes) instead of the grid.')
    parser.add_argument('--exclude', default=[], type=_rect, action='append', metavar='x0,y0,x1,y1',
                        help='Drop the samples whose centre lies in this rectangle of pixels (repeatable).')
    parser.add_argument('--mode', default='subtract', choices=['subtract', 'divide'],
                        help='subtract: additive gradients (light pollution). divide: multiplicative ones (vignetting). Default: subtract')
    parser.add_argument('--pedestal', default=None, type=float,
                        help='Level added back after the subtraction (the level the image keeps under divide). '
                             'Default: the median of the kept samples')
    parser.add_argument('--k_high', default=2.0, type=float, help='Samples more than this many sigma above the surface are rejected. Default: 2.0')
    parser.add_argument('--k_low', default=3.0, type=float, help='Samples more than this many sigma below the surface are rejected. Default: 3.0')
    parser.add_argument('--step', default=16, type=int, help='Step in pixels of the lattice the surface is evaluated on, 4 to 64. Default: 16')
    parser.add_argument('--background_out', default=None, metavar='FITS', help='Also write the fitted surface as an image.')
    parser.add_argument('--samples_out', default=None, metavar='FILE.YML', help='Also write x, y, value, sigma and kept of every sample.')
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    return parser.parse_args(argv)


def main(args=None):
    p = command_line_opts(args)
    from astrophotography_amd.core.ApRemoveGradient import ApRemoveGradient
    rg = ApRemoveGradient(p.loglevel)
    rg.remove_files(p.input, p.output, background_out=p.background_out, samples_out=p.samples_out, samples_file=p.samples, model=p.model,
                    degree=p.degree, smoothing=p.smoothing, samples_per_row=p.samples_per_row, box_radius=p.box_radius, exclude=p.exclude,
                    mode=p.mode, pedestal=p.pedestal, k_high=p.k_high, k_low=p.k_low, step=p.step)
    return 0


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
