"""ctypes binding of libapgpu.so (C ABI: include/apgpu.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails, an exception is
raised.  The CPU oracle under oracle/ is test infrastructure and is never imported from here.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, 'libapgpu.so')

APGPU_F32, APGPU_U16, APGPU_F64 = 0, 1, 2
OPS = {'ADD': 0, 'SUB': 1, 'MUL': 2, 'DIV': 3}
CENTER = {'median': 0, 'mean': 1}
DEV = {'std': 0, 'mad_std': 1}
MAX_STACK = 512
STACK_EXACT_MOMENTS, STACK_MOMENTS_MEAN, STACK_SINGLE_KERNEL, STACK_NONFINITE_UNCLIPPED = 1, 2, 4, 8    # apgpu_stack_args.flags
STACK_REJECT_WINSORIZED, STACK_REJECT_MINMAX = 16, 32   # apgpu_stack_args.flags: the rejection rules of small stacks (ops.stack_reject)
STACK_FRAME_PARAMS = 64                                 # APGPU_STACK_FRAME_PARAMS: exp_ratio = float32 [3][N] scale, offset, weight (with a rejection rule)
STACK_FRAME_LOCAL = 128                                 # APGPU_STACK_FRAME_LOCAL: workspace = a host StackLocal (scale / offset meshes; with a rejection rule)
STACK_REJECT_ESD = 256                                  # APGPU_STACK_REJECT_ESD: the generalized ESD test; workspace = a host StackEsd
STACK_REJECT_MAX = 128                                # APGPU_STACK_REJECT_MAX: frames a rejection rule takes
CCDPROC_FORM = {'astropy': 0, 'legacy': 1}                                  # APGPU_CCDPROC_*
STACK_WS_STATS_OFFSET = 16384                           # APGPU_STACK_WS_STATS_OFFSET: int64 calls, pixels, pixels listed, 64-pixel blocks given up

E_INVAL, E_UNSUPPORTED, E_LAUNCH, E_WORKSPACE = -1, -2, -3, -4
GAUSS2D_REC, GAUSS2D_MAX_BOX = 20, 76                   # APGPU_GAUSS2D_REC, APGPU_GAUSS2D_MAX_BOX
REGISTER_MAX_K, REGISTER_MAX_STARS = 64, 4096           # APGPU_REGISTER_MAX_K, APGPU_REGISTER_MAX_STARS
COMPOSITE_MAX_VARIANTS, TONE_TABLE_LEN = 16, 10241      # APGPU_COMPOSITE_MAX_VARIANTS, APGPU_TONE_TABLE_LEN
BLUR_MAX_RADIUS, BLUR_TILE_H, BLUR_TILE_W = 32, 32, 64  # APGPU_BLUR_MAX_RADIUS, APGPU_BLUR_TILE_H, APGPU_BLUR_TILE_W
DECONV_MAX_RADIUS, DECONV_TILE_H, DECONV_TILE_W = 12, 32, 64    # APGPU_DECONV_MAX_RADIUS, APGPU_DECONV_TILE_H, APGPU_DECONV_TILE_W
STARLET_MAX_SCALES, STARLET_TILE_H, STARLET_TILE_W, STARLET_CHAIN = 6, 32, 64, 8     # APGPU_STARLET_MAX_SCALES, _TILE_H, _TILE_W, _CHAIN
STARLET_TILE_MAX_SPACING, STARLET_TILE_MAX_AUTO = 8, 0  # APGPU_STARLET_TILE_MAX_SPACING, APGPU_STARLET_TILE_MAX_AUTO
STARLET_MODE = {'hard': 0, 'soft': 1}                   # APGPU_STARLET_HARD, APGPU_STARLET_SOFT
STARLET_FIRST, STARLET_LAST = 1, 2                      # APGPU_STARLET_FIRST, APGPU_STARLET_LAST
STARLET_FORM = {'auto': 0, 'tile': 1, 'direct': 2}      # APGPU_STARLET_FORM_*
DRIZZLE_TILE_H, DRIZZLE_TILE_W = 4, 64                  # APGPU_DRIZZLE_TILE_H, APGPU_DRIZZLE_TILE_W
DEMOSAIC_RCD_TILE_H, DEMOSAIC_RCD_TILE_W, DEMOSAIC_RCD_HALO = 32, 64, 10     # APGPU_DEMOSAIC_RCD_TILE_H, _TILE_W, _HALO
POLY_MAX_DEGREE = 5                                     # APGPU_POLY_MAX_DEGREE
GRADIENT_MAX_SAMPLES, GRADIENT_MAX_RADIUS, GRADIENT_MAX_DEGREE = 4096, 32, 6     # APGPU_GRADIENT_MAX_SAMPLES, _MAX_RADIUS, _MAX_DEGREE
GRADIENT_MIN_STEP, GRADIENT_MAX_STEP, GRADIENT_TILE_H, GRADIENT_TILE_W = 4, 64, 32, 128      # APGPU_GRADIENT_MIN_STEP, _MAX_STEP, _TILE_H, _TILE_W
SURFACE_MODEL = {'poly': 0, 'tps': 1}                   # APGPU_SURFACE_POLY, APGPU_SURFACE_TPS
GRADIENT_MODE = {'subtract': 0, 'divide': 1}            # APGPU_GRADIENT_SUBTRACT, APGPU_GRADIENT_DIVIDE
CELL_MAX_CAPACITY = 65536                               # APGPU_CELL_MAX_CAPACITY
EPSF_MAX_OVERSAMPLING, EPSF_MAX_RADIUS, EPSF_REC, EPSF_TILE = 4, 32, 8, 32      # APGPU_EPSF_MAX_OVERSAMPLING, _MAX_RADIUS, _REC, _TILE
SUBTRACT_MAX_RADIUS, SUBTRACT_MAX_BASIS, SUBTRACT_MAX_DEGREE, SUBTRACT_MAX_HALF = 15, 64, 3, 15     # APGPU_SUBTRACT_MAX_RADIUS, _MAX_BASIS, _MAX_DEGREE, _MAX_HALF
SUBTRACT_TILE_H, SUBTRACT_TILE_W, SUBTRACT_CONVOLVED_IMAGE = 32, 64, 1                             # APGPU_SUBTRACT_TILE_H, _TILE_W, _CONVOLVED_IMAGE


class ApGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('libapgpu error %d: %s' % (code, msg))
        self.code = code


class StackArgs(C.Structure):
    """struct apgpu_stack_args (include/apgpu.h)."""
    _fields_ = [
        ('frames', C.c_void_p), ('dtype', C.c_int32), ('n_frames', C.c_int32), ('n_pixels', C.c_int64),
        ('bias', C.c_void_p), ('dark', C.c_void_p), ('nflat', C.c_void_p), ('exp_ratio', C.c_void_p),
        ('pedestal', C.c_void_p), ('dark_still_biased', C.c_int32), ('center', C.c_int32),
        ('dev', C.c_int32), ('maxiters', C.c_int32), ('sigma_lower', C.c_double), ('sigma_upper', C.c_double),
        ('pixmask', C.c_void_p), ('mean', C.c_void_p), ('median', C.c_void_p), ('std', C.c_void_p),
        ('count', C.c_void_p), ('moments', C.c_void_p), ('frame_stride', C.c_int64),
        ('mean_f64', C.c_void_p), ('std_f64', C.c_void_p), ('moments_f64', C.c_int32), ('flags', C.c_int32),
        ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t),
    ]


class StackLocal(C.Structure):
    """struct apgpu_stack_local (include/apgpu.h): the descriptor APGPU_STACK_FRAME_LOCAL finds in StackArgs.workspace."""
    _fields_ = [
        ('width', C.c_int64), ('row0', C.c_int64), ('box_height', C.c_int32), ('box_width', C.c_int32),
        ('ny', C.c_int32), ('nx', C.c_int32), ('scale', C.c_void_p), ('offset', C.c_void_p), ('weight', C.c_void_p),
    ]


class StackEsd(C.Structure):
    """struct apgpu_stack_esd (include/apgpu.h): the descriptor APGPU_STACK_REJECT_ESD finds in StackArgs.workspace (lambda_ is its
    member `lambda`: the critical values on the device; local: a host StackLocal's address with APGPU_STACK_FRAME_LOCAL)."""
    _fields_ = [('lambda_', C.c_void_p), ('max_outliers', C.c_int32), ('reserved', C.c_int32), ('local', C.c_void_p)]


# name -> (restype, argtypes); every symbol include/apgpu.h declares
SIGNATURES = {
    'apgpu_last_error': (C.c_char_p, []),
    'apgpu_version': (C.c_int, []),
    'apgpu_flat_normalize_ws_bytes': (C.c_size_t, [C.c_int64]),
    'apgpu_flat_normalize_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_calibrate': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'apgpu_flat_normalize_f64_ws_bytes': (C.c_size_t, [C.c_int64]),
    'apgpu_flat_normalize_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_calibrate_mixed': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]),
    'apgpu_stack_ws_bytes': (C.c_size_t, [C.c_int64, C.POINTER(C.c_size_t)]),
    'apgpu_stack_sigclip': (C.c_int, [C.POINTER(StackArgs), C.c_void_p]),
    'apgpu_stack_median': (C.c_int, [C.POINTER(StackArgs), C.c_void_p]),
    'apgpu_stack_kernel_name': (C.c_int, [C.POINTER(StackArgs), C.c_int, C.c_char_p, C.c_size_t]),
    'apgpu_moments_finalize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'apgpu_moments_finalize_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_void_p]),
    'apgpu_moments_finalize_f64p': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int64, C.c_void_p]),
    'apgpu_resample_stack_ws_bytes': (C.c_size_t, [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32]),
    'apgpu_resample_stack_sigclip': (C.c_int, [C.POINTER(StackArgs), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_combine_ccdproc_f64_ws_bytes': (C.c_size_t, [C.c_int32, C.c_int64]),
    'apgpu_combine_ccdproc_f64': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_sigclip_global_ws_bytes': (C.c_size_t, [C.c_int64]),
    'apgpu_sigclip_global_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_sigclip_global_f64_ws_bytes': (C.c_size_t, [C.c_int64]),
    'apgpu_sigclip_global_f64': (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_axis_nanmedian': (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    'apgpu_sliding_clipped_stats_ws_bytes': (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int64]),
    'apgpu_sliding_clipped_stats': (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int, C.c_double,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_image_difference_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_void_p]),
    'apgpu_threshold_mask_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    'apgpu_mask_add_rects_u8': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    'apgpu_fix_badpix_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    'apgpu_fix_badpix_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    'apgpu_imarith': (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    'apgpu_source_mask_ws_bytes': (C.c_size_t, [C.c_int64, C.c_int64]),
    'apgpu_source_mask_u8': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    'apgpu_box_clipped_stats_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                                              C.c_int32, C.c_void_p, C.c_void_p]),
    'apgpu_spline_zoom_f64': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_double,
                                        C.c_double, C.c_void_p, C.c_void_p]),
    'apgpu_lacosmic_ws_bytes': (C.c_size_t, [C.c_int64, C.c_int64]),
    'apgpu_sepmedfilt_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_lacosmic_satmask': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    'apgpu_lacosmic_iterate': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_float,
                                         C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_imarith_f64': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    'apgpu_fits_decode': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    'apgpu_fits_encode_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'apgpu_fits_encode_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'apgpu_bayer_split_u16': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_resample_affine_f32': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_int64, C.c_void_p]),
    'apgpu_resample_oversampled_f32': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                 C.c_int64, C.c_int64, C.c_void_p]),
    'apgpu_block_mean_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    'apgpu_weighted_mean_f32': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_daofind_convolve_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    'apgpu_local_peaks_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'apgpu_daofind_measure': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_aperture_phot_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double,
                                          C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_gauss2d_fit_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_triangle_build': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_triangle_vote': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                      C.c_void_p, C.c_void_p]),
    'apgpu_nearest_match': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_quantile_levels_ws_bytes': (C.c_size_t, [C.c_int64, C.c_int64]),
    'apgpu_quantile_levels_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_composite_rgb': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int32,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'apgpu_bayer_demosaic': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                       C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'apgpu_bayer_channel_sums': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                           C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_gauss_blur_norm_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_double), C.c_int32, C.c_double, C.c_void_p,
                                            C.c_void_p]),
    'apgpu_pair_moments_ws_bytes': (C.c_size_t, [C.c_int64]),
    'apgpu_pair_moments_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_linear_combine_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p]),
    'apgpu_deconv_ws_bytes': (C.c_size_t, [C.c_int64, C.c_int64]),
    'apgpu_deconv_norm_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    'apgpu_deconv_ratio_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_float,
                                         C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'apgpu_deconv_update_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_float), C.c_int32, C.c_void_p,
                                          C.c_void_p]),
    'apgpu_richardson_lucy_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_float, C.c_float,
                                            C.c_float, C.c_int32, C.c_float, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p]),
    'apgpu_starlet_step_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                         C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    'apgpu_starlet_plane1_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    'apgpu_starlet_ws_bytes': (C.c_size_t, [C.c_int64, C.c_int64]),
    'apgpu_starlet_planes_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_multiscale_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'apgpu_drizzle_f32': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                    C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'apgpu_drizzle_reject_u8': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                          C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'apgpu_nearest_match_poly': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32,
                                           C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_poly_tile_affines': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int64,
                                          C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]),
    'apgpu_drizzle_tiles_f32': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                          C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'apgpu_drizzle_reject_tiles_u8': (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'apgpu_sample_clipped_stats_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_double,
                                                 C.c_int32, C.c_void_p, C.c_void_p]),
    'apgpu_surface_lattice_f64': (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'apgpu_surface_apply_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_sky_project': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    'apgpu_cell_select': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    'apgpu_epsf_accumulate_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_epsf_update_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                        C.c_void_p, C.c_void_p]),
    'apgpu_epsf_shift_f32': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    'apgpu_epsf_fit_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_double, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]),
    'apgpu_epsf_render_f32': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_subtract_basis_f64': (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'apgpu_subtract_stamps_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int32, C.c_double, C.c_double, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    'apgpu_subtract_apply_f32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                           C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib = None


def load():
    """Loads libapgpu.so; raises ImportError (no CPU fallback) if it has not been built."""
    global _lib
    if _lib is None:
        path = os.environ.get('APGPU_LIBRARY', LIB_PATH)      # development: a variant build (tools/variant_lib.sh)
        if not os.path.exists(path):
            raise ImportError('%s is missing: build it with `python -m astrophotography_amd._build` '
                              '(hipcc --offload-arch=gfx950). There is no CPU fallback.' % path)
        # PyTorch-ROCm bundles its own libamdhip64.so; it must be in the process BEFORE libapgpu.so so
        # that both resolve to ONE HIP runtime (stream handles are only valid inside the runtime that
        # created them).
        try:
            import torch  # noqa: F401
        except ImportError:      # symbol-only use without torch (no device work possible then)
            pass
        lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise ApGpuError(rc, load().apgpu_last_error().decode('utf-8', 'replace'))
