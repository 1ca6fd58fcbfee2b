#!/usr/bin/env python3
"""ap_composite - colour composites (RGB TIFF) of three co-added FITS images on the GPU, in place of composite_all.sh + STIFF:

    ap_composite n6888 2560x1920_resamp.fits sho rgb
    ap_composite --red r.fits --green g.fits --blue b.fits -o out.tiff --gamma_fac 1.2 --colour_sat 1.5

The first form is composite_all.sh: for each colour selection (sho: SII, Ha, OIII; rgb: Red, Green, Blue; hgb: Ha, Green, Blue as
red, green, blue) it reads PREFIX_FILTER_SUFFIX and writes PREFIX_FILTERS_SHORTSUFFIX_gfNN_csNN_b8.tiff for gamma_fac 1.0, 1.2,
1.4 times colour_sat 1.0, 1.5, 2.0, with the script's levels (quantiles 0.60 and 0.999) and gamma 2.2.  Missing inputs: their
names are listed and the exit status is 8.  The second form takes any three files; several --gamma_fac / --colour_sat form a
grid, and with more than one variant the label _gfNN_csNN goes in front of the output's extension.  All variants of a selection
come from one kernel launch (ApComposite; DESIGN 4.3f: STIFF is absent, the arithmetic is this project's definition)."""
import argparse
import getpass
import logging
import os

COLOUR_SELECTIONS = {'sho': ('SII', 'Ha', 'OIII'), 'rgb': ('Red', 'Green', 'Blue'), 'hgb': ('Ha', 'Green', 'Blue')}   # composite_all.sh:192-198
SCRIPT_GAMMA_FAC = (1.0, 1.2, 1.4)          # composite_all.sh:150
SCRIPT_COLOUR_SAT = (1.0, 1.5, 2.0)         # composite_all.sh:147
SCRIPT_MIN_LEVEL, SCRIPT_MAX_LEVEL = 0.60, 0.999        # composite_all.sh:179-182 (they override :167-170)
SCRIPT_GAMMA = 2.2
EXIT_BAD_SELECTION, EXIT_MISSING = 4, 8     # composite_all.sh:201, :221


def _levels(text):
    try:
        return [float(v) for v in str(text).split(',')]
    except ValueError:
        raise argparse.ArgumentTypeError('%r is not a number or three numbers separated by commas' % (text,))


def _types(text):
    t = [v.strip().upper() for v in str(text).split(',')]
    if len(t) not in (1, 3) or any(v not in ('QUANTILE', 'MANUAL') for v in t):
        raise argparse.ArgumentTypeError('%r: QUANTILE or MANUAL, one value or three separated by commas' % (text,))
    return t if len(t) == 3 else t * 3


def command_line_opts(argv):
    parser = argparse.ArgumentParser(prog='ap_composite', description='Colour composites (RGB TIFF) of three co-added FITS images.')
    parser.add_argument('names', metavar='PREFIX SUFFIX SELECTION', nargs='*',
                        help='composite_all.sh form: file prefix, file suffix and one or more of sho, rgb, hgb.')
    parser.add_argument('--red', metavar='R.FITS', help='Image shown as red.')
    parser.add_argument('--green', metavar='G.FITS', help='Image shown as green.')
    parser.add_argument('--blue', metavar='B.FITS', help='Image shown as blue.')
    parser.add_argument('-o', '--output', metavar='OUT.TIFF', help='Output TIFF of the --red/--green/--blue form.')
    parser.add_argument('--gamma_fac', action='append', type=float, metavar='FAC',
                        help='Luminance gamma factor; repeatable. Default: 1.0 (composite_all.sh form: 1.0 1.2 1.4)')
    parser.add_argument('--colour_sat', action='append', type=float, metavar='SAT',
                        help='Colour saturation; repeatable. Default: 1.0 (composite_all.sh form: 1.0 1.5 2.0)')
    parser.add_argument('--gamma', default=SCRIPT_GAMMA, type=float, help='Display gamma. Default: 2.2')
    parser.add_argument('--min_level', default=[SCRIPT_MIN_LEVEL], type=_levels, metavar='L[,L,L]', help='Lower level. Default: 0.60')
    parser.add_argument('--max_level', default=[SCRIPT_MAX_LEVEL], type=_levels, metavar='L[,L,L]', help='Upper level. Default: 0.999')
    parser.add_argument('--min_type', default=['QUANTILE'] * 3, type=_types, metavar='QUANTILE|MANUAL', help='Default: QUANTILE')
    parser.add_argument('--max_type', default=['QUANTILE'] * 3, type=_types, metavar='QUANTILE|MANUAL', help='Default: QUANTILE')
    parser.add_argument('--bits', default=8, type=int, choices=[8, 16], help='Bits per channel. Default: 8')
    parser.add_argument('--no_flip', action='store_true', help='Keep the FITS row order (default: first TIFF row = last FITS row, as STIFF).')
    parser.add_argument('--description', default=None, help='ImageDescription tag. Default: the prefix, or the output name.')
    parser.add_argument('--copyright', default=None, help='Copyright tag. Default: the user name.')
    parser.add_argument('-l', '--loglevel', default='INFO', help='Logging message level. Default: INFO')
    p = parser.parse_args(argv)
    explicit = [p.red, p.green, p.blue, p.output]
    if any(v is not None for v in explicit):
        if not all(v is not None for v in explicit) or p.names:
            parser.error('the explicit form takes --red, --green, --blue and -o, and no positional arguments')
        p.form = 'files'
    else:
        if len(p.names) < 3:
            parser.error('expected PREFIX SUFFIX and at least one colour selection (sho, rgb, hgb), or --red/--green/--blue/-o')
        p.form = 'script'
        p.prefix, p.suffix, p.selections = p.names[0], p.names[1], p.names[2:]
    return p


def label(gamma_fac, colour_sat, bits):
    """gf10_cs15_b8: the labels of composite_all.sh:148-155 (the value times ten, two digits)."""
    return 'gf%02d_cs%02d_b%d' % (round(gamma_fac * 10), round(colour_sat * 10), bits)


def input_names(prefix, suffix, selection):
    """The red, green and blue file of a colour selection (composite_all.sh:209)."""
    return ['%s_%s_%s' % (prefix, f, suffix) for f in COLOUR_SELECTIONS[selection]]


def output_name(prefix, suffix, selection, gamma_fac, colour_sat, bits):
    """composite_all.sh:137, :225, :243-246: the suffix loses its last extension, the filter names are run together."""
    short = suffix.rsplit('.', 1)[0] if '.' in suffix else suffix
    return '%s_%s_%s_%s.tiff' % (prefix, ''.join(COLOUR_SELECTIONS[selection]), short, label(gamma_fac, colour_sat, bits))


def variant_outputs(output, grid, bits):
    """The output files of the explicit form: OUT itself for one variant, OUT_gfNN_csNN_bN.EXT for several."""
    if len(grid) == 1:
        return [output]
    stem, ext = os.path.splitext(output)
    return ['%s_%s%s' % (stem, label(g, s, bits), ext) for g, s in grid]


def _user():
    try:
        return getpass.getuser()
    except Exception:                                        # noqa: BLE001 - no user database entry: no copyright holder
        return ''


def main(args=None):
    p = command_line_opts(args)
    copyright = p.copyright if p.copyright is not None else _user()
    common = dict(gamma=p.gamma, bits=p.bits, flip=not p.no_flip, min_level=p.min_level, max_level=p.max_level, min_type=p.min_type,
                  max_type=p.max_type, copyright=copyright)
    from astrophotography_amd.core.ApComposite import ApComposite, variant_grid
    if p.form == 'files':
        grid = variant_grid(p.gamma_fac or [1.0], p.colour_sat or [1.0])
        ApComposite(p.loglevel).composite_files(p.red, p.green, p.blue, variant_outputs(p.output, grid, p.bits),
                                                gamma_fac=p.gamma_fac or [1.0], colour_sat=p.colour_sat or [1.0],
                                                description=p.description if p.description is not None else os.path.basename(p.output),
                                                **common)
        return 0
    gamma_fac, colour_sat = p.gamma_fac or list(SCRIPT_GAMMA_FAC), p.colour_sat or list(SCRIPT_COLOUR_SAT)
    grid = variant_grid(gamma_fac, colour_sat)
    comp = None
    for sel in p.selections:
        if sel not in COLOUR_SELECTIONS:
            print('Error, unexpected 3-color combination %s\n  Allowed values are: %s' % (sel, ' '.join(COLOUR_SELECTIONS)))
            return EXIT_BAD_SELECTION
        files = input_names(p.prefix, p.suffix, sel)
        missing = [f for f in files if not os.path.exists(f)]
        if missing:
            for f in missing:
                print('    Error, cannot find %s' % f)
            print('Error, missing %d required files.\n  Current directory: %s' % (len(missing), os.getcwd()))
            return EXIT_MISSING
        comp = comp or ApComposite(p.loglevel)
        outs = [output_name(p.prefix, p.suffix, sel, g, s, p.bits) for g, s in grid]
        comp.composite_files(files[0], files[1], files[2], outs, gamma_fac=gamma_fac, colour_sat=colour_sat,
                             description=p.description if p.description is not None else p.prefix, **common)
    return 0


if __name__ == '__main__':
    try:
        status = main()
    except Exception:
        logging.getLogger(__name__).critical('Shutting down due to fatal error')
        raise
    else:
        raise SystemExit(status)
