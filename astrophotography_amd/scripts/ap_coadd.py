#!/usr/bin/env python3
"""ap_coadd - Lanczos-3 resample + co-add of registered frames on the GPU (the role SWarp plays in the
reference's scripts/resample_all.sh:330-342).  Transforms come from a YAML file:

    transforms:
      frame-0001.fits: [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]     # xin = a0*x + a1*y + a2 ; yin = a3*x + a4*y + a5
      frame-0002.fits: [0.99999, -0.0035, 1.25, 0.0035, 0.99999, -0.75]

A file written by ``ap_register --model poly3`` also holds ``distortion:`` (a polynomial map per frame, DESIGN 4.3e'), which is used
in place of the affines unless --ignore_distortion is given.  Without --transforms the frames are registered through their headers:
RA---TAN / DEC--TAN, with or without SIP distortion terms.
"""
import argparse
import logging
import os


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_coadd', description='Resample registered frames onto one grid and combine them.')
    parser.add_argument('output_image', metavar='OUTPUT_IMAGE.FITS', help='Output co-added image (overwritten).')
    parser.add_argument('input_images', metavar='INPUT_IMAGE.FITS', nargs='+', help='Calibrated frames to combine.')
    parser.add_argument('--transforms', default=None, metavar='TRANSFORMS.YML',
                        help='Per-file 2x3 affine transforms. Default: register through the TAN WCS of the file headers.')
    parser.add_argument('--center', default=None, metavar='RA,DEC', help='Output tangent point in degrees (WCS mode).')
    parser.add_argument('--pixelscale', default=None, type=float, metavar='ARCSEC', help='Output pixel scale (WCS mode).')
    parser.add_argument('--combine', default='MEDIAN', choices=['MEDIAN', 'AVERAGE', 'WEIGHTED', 'SUM', 'CLIPPED', 'WINSORIZED', 'MINMAX', 'ESD'],
                        help='Combine type (resample_all.sh add modes 0/1/2 = MEDIAN/WEIGHTED/SUM); WINSORIZED and MINMAX reject '
                             'outliers in stacks of few frames, ESD (the generalized ESD test) in stacks of a couple of dozen and more (at most 128). '
                             'Default: MEDIAN')
    parser.add_argument('--weight_image', default=None, metavar='WEIGHTS.FITS', help='Optional output weight image.')
    parser.add_argument('--badpix', default=None, metavar='BADPIX.FITS', help='Optional bad pixel mask shared by the inputs.')
    parser.add_argument('--image_size', default=None, metavar='NX,NY', help='Output size (default: input size).')
    parser.add_argument('--oversampling', default=1, type=int, metavar='N',
                        help='Sub-samples per output pixel and axis (SWarp OVERSAMPLING; resample_all.sh uses 4). Default: 1')
    parser.add_argument('--gain_keyword', default='EGAIN', metavar='KEYWORD',
                        help='Header keyword with the detector gain in e-/ADU (SWarp GAIN_KEYWORD). Default: EGAIN')
    parser.add_argument('--sigma', default=3.0, type=float, metavar='NSIGMA', help='CLIPPED and WINSORIZED.')
    parser.add_argument('--maxiters', default=5, type=int, metavar='N', help='CLIPPED and WINSORIZED; -1 = until convergence.')
    parser.add_argument('--nlow', default=1, type=int, metavar='N', help='MINMAX: lowest values dropped per pixel. Default: 1')
    parser.add_argument('--nhigh', default=1, type=int, metavar='N', help='MINMAX: highest values dropped per pixel. Default: 1')
    parser.add_argument('--esd_outliers', default=0.3, type=float, metavar='FRACTION',
                        help='ESD: the largest fraction of a pixel\'s values that may be outliers, 0 .. 0.5. Default: 0.3')
    parser.add_argument('--esd_significance', default=0.05, type=float, metavar='ALPHA', help='ESD: significance level of the test. Default: 0.05')
    parser.add_argument('--esd_low_relaxation', default=1.5, type=float, metavar='FACTOR',
                        help='ESD: a low value\'s deviation is divided by this before it is tested (>= 1). Default: 1.5')
    parser.add_argument('--normalize', default='none', choices=['none', 'additive', 'multiplicative', 'additive+scaling'],
                        help='Bring the resampled frames to the level of the reference frame before they are combined: by an offset '
                             '(sky level), a factor (transparency) or scale and offset (noise and sky). Default: none')
    parser.add_argument('--reference', default='0', metavar='FILE_OR_INDEX',
                        help='The frame the others are normalised to: one of the input files or its index. Default: 0')
    parser.add_argument('--weighting', default='none', choices=['none', 'noise'],
                        help='WINSORIZED, MINMAX and ESD: average the surviving values with inverse-variance weights of the '
                             'normalised frames. Default: none')
    parser.add_argument('--norm_box', default=None, type=int, metavar='PIXELS',
                        help='WINSORIZED, MINMAX and ESD: normalise LOCALLY - the statistics are taken per box of PIXELS x PIXELS and scale and '
                             'offset are interpolated at every pixel, for frames whose sky differs in shape (moon, light dome, '
                             'meridian flip). Default: one scale and one offset per frame')
    parser.add_argument('--ignore_distortion', default=False, action='store_true',
                        help='Use the affines of the transforms file even when it holds a distortion entry (ap_register --model polyN).')
    parser.add_argument('--max_tile_error', default=0.01, type=float, metavar='PIXELS',
                        help='Distortion: refuse maps whose linearisation per 16 x 64 tile costs more than this. Default: 0.01')
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    return parser.parse_args(argv)


def distortion_maps(doc, input_images, ignore=False):
    """The distortion maps of the input files from a transforms document (its `distortion:` entry, as ap_register --model polyN
    writes it), or None when it has none or `ignore` is set."""
    entry = doc.get('distortion')
    if entry is None or ignore:
        return None
    from astrophotography_amd.distortion import from_document
    try:
        return from_document(entry, input_images)
    except ValueError as err:
        raise RuntimeError(f'Error, {err}.') from err


def main(args=None):
    p = command_line_opts(args)
    import yaml
    from astrophotography_amd.core.ApResample import ApResample
    affines = None
    table = None
    maps = None
    if p.transforms is not None:
        with open(p.transforms) as fh:
            doc = yaml.safe_load(fh) or {}
        table = doc.get('transforms') or {}
        affines = []
        maps = distortion_maps(doc, p.input_images, p.ignore_distortion)
    for f in (p.input_images if table is not None else []):
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
    rs = ApResample(p.loglevel, combine=p.combine, sigma=p.sigma, maxiters=None if p.maxiters < 0 else p.maxiters,
                    oversampling=p.oversampling, gain_keyword=p.gain_keyword, nlow=p.nlow, nhigh=p.nhigh, normalize=p.normalize, reference=p.reference,
                    weighting=None if p.weighting == 'none' else p.weighting, norm_box=p.norm_box,
                    esd_outliers=p.esd_outliers, esd_significance=p.esd_significance, esd_low_relaxation=p.esd_low_relaxation)
    center = None
    if p.center:
        center = tuple(float(v) for v in p.center.split(','))
    rs.coadd_files(p.input_images, affines, p.output_image, weight_file=p.weight_image, mask_file=p.badpix, out_shape=out_shape,
                   center=center, pixscale=p.pixelscale, maps=maps, max_tile_error=p.max_tile_error)
    return 0


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
