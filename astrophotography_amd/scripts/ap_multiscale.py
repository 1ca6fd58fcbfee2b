#!/usr/bin/env python3
"""ap_multiscale - noise reduction and detail enhancement by scale: the starlet (B3-spline a trous) transform on the GPU
(ApMultiscale).

    ap_multiscale coadd.fits clean.fits
    ap_multiscale sharp.fits clean.fits --scales 5 --threshold 3,3,2,1,0 --gain 1,1.3,1.3,1,1 --mode soft --sigma 4.1

The image noise is measured from the finest plane unless given; pixels without data stay NaN.  The settings are logged and written
to the output header (MSCALES, MSMODE, MSSIGMA, MSK1.., MSG1.., MSGRES); the result goes on to ap_composite."""
import argparse
import logging


def _floats(text):
    try:
        return [float(v) for v in text.split(',')]
    except ValueError:
        raise argparse.ArgumentTypeError('expected a number or a comma-separated list of numbers, got %r' % text)


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_multiscale', description='Starlet denoise and sharpen of an image.')
    parser.add_argument('input', metavar='INPUT.FITS', help='Image to treat (float32 co-add, NaN = no data).')
    parser.add_argument('output', metavar='OUTPUT.FITS', help='Output image (float32, overwritten).')
    parser.add_argument('--scales', default=4, type=int, help='Number of scales, 1 to 6 (spacings 1, 2, 4, ...). Default: 4')
    parser.add_argument('--threshold', default=None, type=_floats, metavar='K1,K2,..',
                        help='Threshold of each plane in units of its noise, one value per scale or one for all; 0 leaves a plane alone. '
                        'Default: 3,3,2,1,1,1 cut to the number of scales')
    parser.add_argument('--gain', default=[1.0], type=_floats, metavar='G1,G2,..',
                        help='Gain of each plane, one value per scale or one for all; above 1 sharpens that scale, 0 drops it. Default: 1')
    parser.add_argument('--residual_gain', default=1.0, type=float, help='Gain of the smooth residual. Default: 1')
    parser.add_argument('--mode', default='hard', choices=['hard', 'soft'], help='Thresholding of the planes. Default: hard')
    parser.add_argument('--sigma', default=None, type=float, help='Image noise in ADU. Default: measured from the finest plane')
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    return parser.parse_args(argv)


def main(args=None):
    p = command_line_opts(args)
    from astrophotography_amd.core.ApMultiscale import ApMultiscale
    ms = ApMultiscale(p.loglevel, scales=p.scales, k=p.threshold, gains=p.gain, residual_gain=p.residual_gain, mode=p.mode, sigma=p.sigma)
    ms.process_file(p.input, p.output)
    return 0


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
