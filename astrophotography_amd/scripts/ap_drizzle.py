#!/usr/bin/env python3
"""ap_drizzle - drizzle co-add of registered, dithered frames onto a finer grid on the GPU (ApDrizzle).

    ap_drizzle out.fits frame-*.fits --transforms transforms.yml --scale 2 --pixfrac 0.5 --reject --weight_image weight.fits
    ap_drizzle out.fits mosaic-*.fits --transforms transforms.yml --cfa --pattern RGGB      # writes out_r.fits, out_g.fits, out_b.fits

The transforms are those of ap_coadd, as ap_register writes them:

    transforms:
      frame-0001.fits: [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]     # xin = a0*x + a1*y + a2 ; yin = a3*x + a4*y + a5
"""
import argparse
import logging
import os


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_drizzle', description='Drizzle dithered frames onto a finer grid and combine them.')
    parser.add_argument('output_image', metavar='OUTPUT_IMAGE.FITS', help='Output drizzled image (overwritten).')
    parser.add_argument('input_images', metavar='INPUT_IMAGE.FITS', nargs='+', help='Calibrated frames to combine.')
    parser.add_argument('--transforms', required=True, metavar='TRANSFORMS.YML', help='Per-file 2x3 affine transforms (ap_register writes them).')
    parser.add_argument('--scale', default=2.0, type=float, metavar='S', help='Output pixels per input pixel and axis. Default: 2')
    parser.add_argument('--pixfrac', default=0.5, type=float, metavar='P', help='Side of a drop in input pixels, (0, 1]. Default: 0.5')
    parser.add_argument('--reject', default=False, action='store_true', help='Flag outliers against a median co-add first.')
    parser.add_argument('--k', default=3.5, type=float, metavar='NSIGMA', help='--reject: noise term of the threshold. Default: 3.5')
    parser.add_argument('--grow', default=1.2, type=float, metavar='G',
                        help='--reject: factor on the local spread of the reference, which protects star cores. Default: 1.2')
    parser.add_argument('--cfa', default=False, action='store_true',
                        help='The inputs are Bayer mosaics: drizzle each colour from its own pixels into OUTPUT_r/_g/_b.fits.')
    parser.add_argument('--pattern', default=None, metavar='RGGB', help='--cfa: the Bayer pattern. Default: BAYERPAT of the first file')
    parser.add_argument('--weight_image', default=None, metavar='WEIGHTS.FITS', help='Optional output weight image.')
    parser.add_argument('--badpix', default=None, metavar='BADPIX.FITS', help='Optional bad pixel mask shared by the inputs.')
    parser.add_argument('--image_size', default=None, metavar='NX,NY', help='Output size (default: the input size times the scale).')
    parser.add_argument('--no_weighting', default=False, action='store_true', help='Equal frame weights instead of inverse background variance.')
    parser.add_argument('--conserve_flux', default=False, action='store_true', help='Keep totals (scale by the pixel-area ratio) instead of surface brightness.')
    parser.add_argument('--ignore_distortion', default=False, action='store_true',
                        help='Use the affines of the transforms file even when it holds a distortion entry (ap_register --model polyN).')
    parser.add_argument('--max_tile_error', default=0.01, type=float, metavar='PIXELS',
                        help='Distortion: refuse maps whose linearisation per 16 x 64 tile costs more than this. Default: 0.01')
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    return parser.parse_args(argv)


def main(args=None):
    p = command_line_opts(args)
    import yaml
    from astrophotography_amd.core.ApDrizzle import ApDrizzle
    with open(p.transforms) as fh:
        doc = yaml.safe_load(fh) or {}
    table = doc.get('transforms') or {}
    affines = []
    for f in p.input_images:
        key = f if f in table else os.path.basename(f)
        if key not in table:
            raise RuntimeError(f'Error, no transform for {f} in {p.transforms}.')
        if len(table[key]) != 6:
            raise RuntimeError(f'Error, transform of {key} must have 6 coefficients.')
        affines.append([float(v) for v in table[key]])
    out_shape = None
    if p.image_size:
        nx, ny = (int(v) for v in p.image_size.split(','))
        out_shape = (ny, nx)
    dz = ApDrizzle(p.loglevel, scale=p.scale, pixfrac=p.pixfrac, reject=p.reject, k=p.k, grow=p.grow,
                   weighting='none' if p.no_weighting else 'background', conserve_flux=p.conserve_flux)
    from astrophotography_amd.scripts.ap_coadd import distortion_maps
    dz.drizzle_files(p.input_images, affines, p.output_image, weight_file=p.weight_image, mask_file=p.badpix, cfa=p.cfa, pattern=p.pattern,
                     out_shape=out_shape, maps=distortion_maps(doc, p.input_images, p.ignore_distortion), max_tile_error=p.max_tile_error)
    return 0


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
