/*
 * apgpu.h - C ABI of libapgpu.so: the MI355X (gfx950) implementation of AstroPhotography's per-pixel
 * calibrate -> mask -> arithmetic -> stack-reduce hot path.
 *
 * The reference (DaveStrickland/AstroPhotography v0.5.1) is pure Python and has no FFI of its own;
 * its boundary for this path is the Ap* class API.  Each entry point below replaces
 * the NumPy/astropy/ccdproc arithmetic of one reference method (cited as file:line relative to
 * AstroPhotography/ in the reference tree); the Python Ap* shells in astrophotography_amd/ bind them
 * with ctypes (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless its name ends in _host;
 *  - the caller owns every buffer; the library allocates nothing and keeps no state (one exception, stated at
 *    apgpu_stack_args.workspace: a stack call WITHOUT a workspace makes a stream-ordered temporary allocation);
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is asynchronous
 *    with respect to the host, no call synchronises;
 *  - functions return 0 on success or a negative APGPU_E* code; apgpu_last_error() returns a
 *    thread-local message for the last failing call;
 *  - images are row-major [H][W]; frame stacks are contiguous slabs [N][H][W] (P = H*W pixels);
 *  - workspace sizes are returned by the matching *_ws_bytes function; workspaces need 16-byte
 *    alignment (any hipMalloc / torch allocation has it).
 */
#ifndef APGPU_H
#define APGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APGPU_VERSION 130           /* 0.1.3: apgpu_resample_stack_sigclip, APGPU_STACK_NONFINITE_UNCLIPPED, apgpu_combine_ccdproc_f64(form);
                                       additive since: apgpu_axis_nanmedian, apgpu_sliding_clipped_stats(_ws_bytes);
                                       apgpu_daofind_convolve_f32, apgpu_local_peaks_f32, apgpu_daofind_measure, apgpu_aperture_phot_f32;
                                       apgpu_gauss2d_fit_f32; apgpu_triangle_build, apgpu_triangle_vote, apgpu_nearest_match;
                                       apgpu_quantile_levels_f32(_ws_bytes), apgpu_composite_rgb;
                                       apgpu_bayer_demosaic, apgpu_bayer_channel_sums;
                                       apgpu_drizzle_f32, apgpu_drizzle_reject_u8;
                                       apgpu_nearest_match_poly, apgpu_poly_tile_affines, apgpu_drizzle_tiles_f32,
                                       apgpu_drizzle_reject_tiles_u8;
                                       apgpu_sky_project, apgpu_cell_select */

/* error codes */
#define APGPU_OK            0
#define APGPU_EINVAL       -1       /* bad argument (NULL pointer, bad enum, size <= 0 ...) */
#define APGPU_EUNSUPPORTED -2       /* valid request this build cannot serve (e.g. N > APGPU_MAX_STACK) */
#define APGPU_ELAUNCH      -3       /* HIP runtime error at launch */
#define APGPU_EWORKSPACE   -4       /* workspace too small */

/* element types of pixel data */
#define APGPU_F32 0
#define APGPU_U16 1
#define APGPU_F64 2                 /* float64 masters / frames (apgpu_calibrate_mixed, *_f64 entry points) */

/* ApImArith._allowed_ops (core/ApImArith.py:34) */
#define APGPU_OP_ADD 0
#define APGPU_OP_SUB 1
#define APGPU_OP_MUL 2
#define APGPU_OP_DIV 3

/* clip centre / deviation estimators (astropy SigmaClip cenfunc / stdfunc) */
#define APGPU_CENTER_MEDIAN 0
#define APGPU_CENTER_MEAN   1
#define APGPU_DEV_STD       0
#define APGPU_DEV_MAD_STD   1

/* largest N one stack call reduces: up to 128 frames the per-pixel column lives in registers; 129 .. 512 frames are reduced chunk by
 * chunk (64 frames in registers at a time: clipped mean with its median / std planes, plain median, the median / mad_std configuration
 * on raw frames) with an LDS-resident exact kernel behind them for the pixels they are not sure of and for every other option */
#define APGPU_MAX_STACK 512

const char *apgpu_last_error(void);
int apgpu_version(void);

/* ---------------------------------------------------------------------------------------------
 * A1  ApCalibrate._generate_flat (core/ApCalibrate.py:166-190)
 *     norm = np.nanmean(flat) [float32 pairwise sum in 8192-element pieces, / count of non-NaN],
 *     nflat = flat / norm.  Bit-exact with numpy.  norm is written to norm_out[0] (device).
 * ------------------------------------------------------------------------------------------- */
size_t apgpu_flat_normalize_ws_bytes(int64_t n_pixels);
int apgpu_flat_normalize_f32(const float *flat, float *nflat, float *norm_out, int64_t n_pixels,
                             void *ws, size_t ws_bytes, void *stream);
/* The same for a float64 flat (a master written by ccdproc is float64 and _read_fits keeps float data as it is,
 * core/ApCalibrate.py:301-305): float64 pairwise sum in the same 8192-element pieces, float64 division. */
size_t apgpu_flat_normalize_f64_ws_bytes(int64_t n_pixels);
int apgpu_flat_normalize_f64(const double *flat, double *nflat, double *norm_out, int64_t n_pixels,
                             void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A2  ApCalibrate.calibrate arithmetic block (core/ApCalibrate.py:439-464) incl. the read-time
 *     conversions of _read_fits (core/ApCalibrate.py:304-326), over a slab of N frames:
 *       x = (f32(raw) [+ pedestal[f]]) - bias;  D = dark_still_biased ? dark - bias : dark;
 *       x = x - exp_ratio[f] * D;  out = nflat ? (nflat != 0 ? x / nflat : x) : x
 *     every operation separately rounded to float32 (no FMA contraction, IEEE division).
 *     exp_ratio[N] (float32(EXPTIME_img / EXPTIME_dark)) and pedestal[N] are device arrays;
 *     pedestal may be NULL; a zero pedestal entry adds nothing.  nflat may be NULL (no flat).
 * ------------------------------------------------------------------------------------------- */
int apgpu_calibrate(const void *raw, int raw_dtype, const float *bias, const float *dark,
                    const float *nflat, const float *exp_ratio, const float *pedestal,
                    int dark_still_biased, float *out, int64_t n_frames, int64_t n_pixels, void *stream);

/* A2 with float64 inputs: any mix of raw APGPU_U16 / APGPU_F32 / APGPU_F64 and masters APGPU_F32 / APGPU_F64, evaluated with
 * NumPy's per-operation type promotion exactly as the reference's expressions do (core/ApCalibrate.py:301-305: only
 * non-float FITS data is converted to float32; scripts/ap_combine_darks.py:437: ApMasterCal writes float64 masters):
 *   x = raw - bias in T1 = f64 if raw or bias is f64;  D = dark - bias in T2 = f64 if dark or bias is f64 (or D = dark,
 *   T2 = dark's type);  ds = T2(exp_ratio) * D;  y = x - ds in T3 = T1 | T2;  out = y / nflat in T4 = T3 | nflat's type.
 * exp_ratio[N] and pedestal[N] (may be NULL) are float64 device arrays (python floats; the pedestal is added in the raw
 * frame's own type).  out_dtype must be T4 (APGPU_F64 if any participating array is float64, else APGPU_F32). */
int apgpu_calibrate_mixed(const void *raw, int raw_dtype, const void *bias, int bias_dtype, const void *dark, int dark_dtype,
                          const void *nflat, int nflat_dtype, const double *exp_ratio, const double *pedestal,
                          int dark_still_biased, void *out, int out_dtype, int64_t n_frames, int64_t n_pixels, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A6/A7 + the fused north-star kernel: per-pixel sigma-clipped reduction along N of a slab
 *     [N][P], optionally calibrating each value on the fly (A2) so the raw slab is read once.
 *     Semantics = astropy.stats.sigma_clipped_stats(cube, axis=0, sigma_lower, sigma_upper,
 *     maxiters, cenfunc, stdfunc) (astropy/stats/sigma_clipping.py:298-383, 924-937): non-finite
 *     values dropped; <= maxiters passes of { centre, dev, keep lo <= x <= hi }; final bounds
 *     applied to all values; outputs are the float64 statistics rounded once to float32.
 *     maxiters < 0 iterates to convergence.  With maxiters = 1, centre = median, dev = mad_std and
 *     sigma_lower = sigma_upper = 5 this is the ccdproc.combine configuration of
 *     scripts/ap_combine_darks.py:394-420.
 *     Outputs (each may be NULL): mean/median/std [P] float32, count [P] int32 survivors,
 *     mean_f64/std_f64 [P] float64 (the unrounded statistics: ccdproc.combine and CCDData.write keep float64,
 *     scripts/ap_combine_darks.py:411-439), and the N-shard partial moments of the survivors
 *     (all-reduced over ranks, then apgpu_moments_finalize[_f64]) in one of two layouts:
 *       moments_f64 == 0: float32 moments[3][P] = sum, count, sum of squares (a mean-only exchange all-reduces
 *                         the contiguous [2][P] prefix, 8 bytes per pixel; the float32 sums round per rank);
 *       moments_f64 != 0: double sum[P], double sumsq[P], int32 count[P] laid out back to back in `moments`
 *                         (20 P bytes, 8-byte aligned): ranks add float64 sums and int32 counts, the combined
 *                         mean is the float64 combine rounded once to float32 (12 bytes per pixel mean-only);
 *       moments_f64 == 2: the same layout, but the call ADDS its moments to what the buffer already holds: a stack
 *                         of more than APGPU_MAX_STACK frames is reduced chunk by chunk into one buffer (hierarchical
 *                         clipping: every chunk is clipped against its own statistics);
 *       moments_f64 == 3: packed float64 planes double moments[3][P] = sum, count, sum of squares: the count rides as a
 *                         float64 (exact to 2^53), so ONE all-reduce of the contiguous [2][P] prefix (16 bytes per pixel,
 *                         24 with the third plane for a std) combines the ranks (apgpu_moments_finalize_f64p);
 *       moments_f64 == 4: layout 3, ADDING to what the buffer holds (a rank's share reduced in several chunks).
 * ------------------------------------------------------------------------------------------- */
typedef struct apgpu_stack_args {
    const void *frames;          /* [N][P] APGPU_F32 or APGPU_U16 */
    int32_t dtype;
    int32_t n_frames;            /* 1 .. APGPU_MAX_STACK */
    int64_t n_pixels;
    /* fused calibration: bias == NULL -> frames are reduced as they are */
    const float *bias;           /* [P] */
    const float *dark;           /* [P] */
    const float *nflat;          /* [P] or NULL */
    const float *exp_ratio;      /* [N]; with APGPU_STACK_FRAME_PARAMS: [3][N] scale, offset, weight (below) */
    const float *pedestal;       /* [N] or NULL */
    int32_t dark_still_biased;
    int32_t center;              /* APGPU_CENTER_* */
    int32_t dev;                 /* APGPU_DEV_* */
    int32_t maxiters;            /* >= 1, or < 0 = until convergence */
    double sigma_lower;
    double sigma_upper;
    const uint8_t *pixmask;      /* [P] or NULL; non-zero = pixel excluded (outputs NaN / 0) */
    float *mean;                 /* [P] or NULL */
    float *median;               /* [P] or NULL */
    float *std;                  /* [P] or NULL */
    int32_t *count;              /* [P] or NULL */
    void *moments;               /* NULL, or the partial moments of the survivors in the layout moments_f64 selects */
    int64_t frame_stride;        /* elements between the starts of consecutive frames; 0 = n_pixels.
                                    > n_pixels lets a call reduce a row stripe of a larger slab */
    double *mean_f64;            /* [P] or NULL */
    double *std_f64;             /* [P] or NULL */
    int32_t moments_f64;         /* layout of `moments`, see above */
    int32_t flags;               /* APGPU_STACK_* bits below; 0 = defaults (was reserved0) */
    void *workspace;             /* NULL, or apgpu_stack_ws_bytes(n_pixels, ..) bytes for the two-kernel scheme (below) */
    size_t workspace_bytes;
} apgpu_stack_args;

/* apgpu_stack_args.flags.  The lean kernels (mean / count / moments outputs, median centre, std deviation, full slot
 * counts) clip on a float32 fast path: moments and bound tests in float32 with an error margin, and every wavefront in
 * which a comparison falls inside the margin is redone on the float64 path - the survivor sets are ALWAYS those of the
 * float64 evaluation; the mean carries the float32 rounding of its sum (a few 1e-3 ulp(float32); still the float64 mean
 * rounded once for > 90 % of the pixels, within 1 ulp otherwise).
 *   APGPU_STACK_EXACT_MOMENTS   force the float64 path: the mean is the float64 mean of the survivors rounded once.
 *   APGPU_STACK_MOMENTS_MEAN    the float64-layout moments will only be used for a mean (sum, count): lets the fast path
 *                               fill them; their sum of squares then has float32 accuracy (not good for a std).
 *                               Without it float64-layout moments always come from the float64 path. */
#define APGPU_STACK_EXACT_MOMENTS 1
#define APGPU_STACK_MOMENTS_MEAN 2
#define APGPU_STACK_SINGLE_KERNEL 4   /* never the fast kernel + redo pass pair described below: one complete kernel, no workspace used */
/*   APGPU_STACK_NONFINITE_UNCLIPPED  (dev == APGPU_DEV_MAD_STD only) a column that holds a non-finite value is not clipped: mean /
 *                               count / std of its finite values.  This is what ccdproc >= 2.2's Combiner.sigma_clipping does
 *                               for scripts/ap_combine_darks.py:394-420: it delegates to astropy.stats.sigma_clip, whose general
 *                               path hands the callables np.ma.median / mad_std a plain array in which invalid values are NaN
 *                               - NaN bounds, nothing rejected (golden group G12, arrays c*_b_*, run for real).  Without the
 *                               flag non-finite values are masked and the rest is clipped (ccdproc <= 2.1's own loop). */
#define APGPU_STACK_NONFINITE_UNCLIPPED 8

/* The rejection rules of SMALL stacks (5 .. 30 registered light frames, where an outlier inflates the very standard deviation
 * a sigma clip judges it by): Winsorized sigma clipping and min/max rejection, through apgpu_stack_sigclip.  The two bits are
 * mutually exclusive.  With either: one launch, float64 arithmetic, `workspace` is never read or written (APGPU_STACK_FRAME_LOCAL
 * below reads a descriptor there, on the host);
 * APGPU_STACK_EXACT_MOMENTS, APGPU_STACK_MOMENTS_MEAN and APGPU_STACK_SINGLE_KERNEL are accepted and have no effect;
 * center must be APGPU_CENTER_MEDIAN and dev APGPU_DEV_STD, APGPU_STACK_NONFINITE_UNCLIPPED is APGPU_EINVAL; outputs are
 * mean, std, count, mean_f64, std_f64 (`moments` or `median` != NULL: APGPU_EUNSUPPORTED); n_frames <= APGPU_STACK_REJECT_MAX
 * (the column lives in registers; more: APGPU_EUNSUPPORTED).  Both dtypes, the fused calibration, pixmask and frame_stride
 * work as without the bits.  apgpu_resample_stack_sigclip does not serve them (APGPU_EUNSUPPORTED).
 *
 * Per pixel: S = the finite values of the column after the optional calibration (float32 values), widened to float64, in frame
 * order.  A masked pixel or an empty S gives NaN (0x7fc00000) and count 0.  No contraction: every multiply and add rounds.
 *   APGPU_STACK_REJECT_WINSORIZED (kl = sigma_lower, kh = sigma_upper, both >= 0; maxiters rounds, < 0 = until a round removes
 *   nothing):
 *     round:  n = len(S); if n < 3: stop
 *             med = np.median(S); sig = np.std(S)                      (ddof 0, numpy's summation order)
 *             repeat at most APGPU_STACK_WINSOR_MAX_INNER times:
 *                 W   = min(max(S, med - 1.5*sig), med + 1.5*sig)      (clamped from S each time, never from the previous W)
 *                 s0  = sig; sig = 1.134 * np.std(W)
 *                 if |sig - s0| <= 0.0005 * s0: break
 *             keep x with  med - kl*sig <= x <= med + kh*sig           (inclusive)
 *             if nothing was removed: stop;  S = the kept values, still in frame order
 *     np.median of an even count: the two middle values summed from +0 and halved.
 *   APGPU_STACK_REJECT_MINMAX (nlow = sigma_lower, nhigh = sigma_upper: whole numbers 0 .. 127 held as doubles, else
 *   APGPU_EINVAL; maxiters unused): order S by (order-preserving key of the value: -0 below +0, then frame index), drop the first
 *     nlow and the last nhigh; n <= nlow + nhigh: nothing survives.
 *   Outputs over the survivors in frame order: count = m, mean_f64 = np.add.reduce(surv) / m, std_f64 = np.std(surv); mean and
 *   std are those values rounded once to float32. */
#define APGPU_STACK_REJECT_WINSORIZED 16
#define APGPU_STACK_REJECT_MINMAX 32
#define APGPU_STACK_REJECT_MAX 128
#define APGPU_STACK_WINSOR_MAX_INNER 16

/* APGPU_STACK_FRAME_PARAMS: per-frame normalisation and weights inside the two rejection rules - frames of one night do not
 * share a sky level or a scale, and a rule that compares the values of a pixel with each other needs them on one.  Valid only
 * together with exactly one of APGPU_STACK_REJECT_WINSORIZED / APGPU_STACK_REJECT_MINMAX (without: APGPU_EUNSUPPORTED, the other
 * stack kernels, apgpu_stack_median and apgpu_resample_stack_sigclip do not serve it).  With the bit:
 *   bias, dark, nflat and pedestal must be NULL (APGPU_EINVAL): light frames are calibrated already, the fused calibration and
 *   the frame parameters exclude each other;
 *   exp_ratio must be non-NULL (APGPU_EINVAL) and points to float32 [3][n_frames] on the device: row 0 the scale a_i, row 1 the
 *   offset b_i, row 2 the weight w_i.  The CALLER guarantees a_i and b_i finite and w_i finite and > 0 (the library cannot look);
 *   pixmask, frame_stride, both dtypes, the outputs and APGPU_STACK_REJECT_MAX are as without the bit.
 * Definition (no contraction: every multiply and add rounds):
 *   x = the raw value as float32 (uint16 is exact);  v = float32(float32(a_i * x) + b_i)
 *   S = the finite v of the column in frame order (a raw NaN or inf is not finite after the map either); the rule runs on S
 *   exactly as defined above, the min/max tie rule by frame index included.
 *   count = m; std_f64 = np.std(surv) as above - it is UNWEIGHTED; std = std_f64 rounded once.
 *   mean_f64 = num / den, both sums over the survivors in frame order, sequentially from +0.0 in float64:
 *       num += double(w_k) * double(v_k)       (the product of two widened float32 values is exact)
 *       den += double(w_k)
 *   which is np.cumsum(...)[-1] of the terms; mean = mean_f64 rounded once.  No survivor or a masked pixel: NaN and count 0. */
#define APGPU_STACK_FRAME_PARAMS 64

/* APGPU_STACK_FRAME_LOCAL: LOCAL normalisation inside the two rejection rules - one scale and one offset per frame level the
 * sky, but not its shape: a rising moon, a light dome or a meridian flip leave a gradient of tens of ADU between the frames of a
 * pixel, which the rule takes for the column's sigma.  With the bit, scale and offset of a frame are MESHES (one value per
 * box_height x box_width box, the geometry of apgpu_box_clipped_stats_f32) interpolated bilinearly at every pixel.  Valid only
 * together with exactly one of APGPU_STACK_REJECT_WINSORIZED / APGPU_STACK_REJECT_MINMAX (without: APGPU_EUNSUPPORTED;
 * apgpu_stack_median and apgpu_resample_stack_sigclip: APGPU_EUNSUPPORTED); not together with APGPU_STACK_FRAME_PARAMS
 * (APGPU_EINVAL); bias, dark, nflat, pedestal and exp_ratio must be NULL (APGPU_EINVAL).
 *   `workspace` - which the rejection rules otherwise never look at - is a HOST pointer to an apgpu_stack_local, and
 *   workspace_bytes must be sizeof(apgpu_stack_local).  The library reads it on the host during the call and checks what it
 *   can see (APGPU_EINVAL: width < 1 or not a divisor of n_pixels, row0 < 0, a box side outside 1 .. 32768, ny or nx < 1,
 *   ny * nx >= 2^31, offset NULL, image rows or columns beyond 2^30).  The CALLER guarantees finite meshes and finite weights
 *   > 0.  The mesh need not cover the image: beyond the outer box centres the outer values hold.
 *   pixmask, frame_stride (row stripes: row0), both dtypes, the outputs and APGPU_STACK_REJECT_MAX are as without the bit.
 * Definition (no contraction; every operation rounds once in float32).  Box centres lie at (j + 0.5) box - 0.5.  Per axis, with
 * c the pixel coordinate, b the box size and m the mesh extent (whole-number arithmetic, exact; one IEEE division):
 *     u = 2c + 1 - b;  j0 = clamp(floor(u / 2b), 0, max(m - 2, 0));  j1 = min(j0 + 1, m - 1)
 *     t = float32(clamp(u - 2 b j0, 0, 2b)) / float32(2b)
 * (j0, j1, ty) from the image row y = row0 + p / width, (k0, k1, tx) from the column x = p % width.  For a mesh M of frame i:
 *     top = M[j0][k0] + tx * (M[j0][k1] - M[j0][k0]);  bot = the same on row j1;  m(y, x) = top + ty * (bot - top)
 *   x_raw = the raw value as float32;  v = float32(float32(a(y, x) * x_raw) + b(y, x));  scale == NULL: v = float32(x_raw + b),
 *   the bits a mesh of ones gives.  From here on the definition of APGPU_STACK_FRAME_PARAMS holds word for word: S = the finite
 *   v in frame order, the rule unchanged, count and std_f64 unweighted, mean_f64 = num / den over the survivors with weight[i]
 *   (NULL: 1).  A mesh that is constant per frame gives the bits of APGPU_STACK_FRAME_PARAMS with those scalars. */
#define APGPU_STACK_FRAME_LOCAL 128
typedef struct apgpu_stack_local {
    int64_t width;                  /* pixel p of the call is image row row0 + p / width, column p % width; n_pixels % width == 0 */
    int64_t row0;                   /* image row of the call's first pixel (row stripes); >= 0 */
    int32_t box_height, box_width;  /* 1 .. 32768 */
    int32_t ny, nx;                 /* mesh shape, >= 1 */
    const float *scale;             /* device float32 [n_frames][ny][nx], or NULL = 1 everywhere */
    const float *offset;            /* device float32 [n_frames][ny][nx], not NULL */
    const float *weight;            /* device float32 [n_frames], or NULL = 1 */
} apgpu_stack_local;

/* APGPU_STACK_REJECT_ESD: the generalized extreme Studentized deviate test (Rosner 1983) as a third rejection rule, for stacks of a
 * couple of dozen frames and more.  The caller states the largest fraction of a column that may be outliers; candidates are taken
 * one at a time from the column's two ends, and the largest prefix of removals that is significant is what goes - two equal
 * outliers cannot mask each other, and a clean column loses a value with probability about alpha, not alpha per value.
 * Mutually exclusive with APGPU_STACK_REJECT_WINSORIZED and APGPU_STACK_REJECT_MINMAX (APGPU_EINVAL); everything said for those
 * bits holds: one launch, float64 arithmetic, n_frames <= APGPU_STACK_REJECT_MAX, outputs mean / std / count / mean_f64 / std_f64
 * (`moments` or `median`: APGPU_EUNSUPPORTED), center APGPU_CENTER_MEDIAN and dev APGPU_DEV_STD, APGPU_STACK_NONFINITE_UNCLIPPED is
 * APGPU_EINVAL, the no-effect bits are accepted, both dtypes, the fused calibration, pixmask and frame_stride work,
 * APGPU_STACK_FRAME_PARAMS and APGPU_STACK_FRAME_LOCAL combine with it; the median entry point and the fused resample + clip do
 * not serve it (APGPU_EUNSUPPORTED).
 *   sigma_lower = frac, the largest fraction of outliers, 0 .. 0.5; sigma_upper = relax, the low relaxation (a low candidate's
 *   deviation is divided by it: dark outliers are rarer than bright ones), >= 1 and finite; else APGPU_EINVAL.  maxiters unused.
 *   `workspace` is a HOST pointer to an apgpu_stack_esd and workspace_bytes its size; the library reads it on the host during the
 *   call.  lambda: the critical values on the DEVICE, float64 [n_frames + 1][max_outliers], lambda[n * max_outliers + i] for step
 *   i of a column of n finite values (the caller guarantees: no NaN; +inf = never significant).  With APGPU_STACK_FRAME_LOCAL the
 *   mesh descriptor is `local` (checked as described there).  APGPU_EINVAL: lambda NULL, max_outliers outside 1 .. 64,
 *   reserved != 0, local non-NULL without the bit or NULL with it.
 * Definition (no contraction: every operation rounds on its own).  Per pixel, S = the finite values of the column after the
 * calibration or the frame map, in float64, n = len(S); a masked pixel or an empty S gives NaN (0x7fc00000) and count 0.
 *     K = min(floor(frac * n), n - 3, max_outliers)        (frac * n: one float64 product; K <= 0: nothing is removed)
 *     y = S ordered by (order-preserving key of the value: -0 below +0, then frame index);  lo, hi = 0, n;  L = H = 0
 *     for i in 0 .. K-1:
 *         w = y[lo:hi];  m = hi - lo
 *         mean = np.add.reduce(w) / m;  d = w - mean;  sd = np.sqrt(np.add.reduce(d * d) / (m - 1))
 *         if not (sd > 0): break
 *         dl = (mean - w[0]) / relax;  dh = w[m-1] - mean
 *         if dh >= dl: R = dh / sd; hi -= 1     else: R = dl / sd; lo += 1
 *         if R > lambda[n][i]: L, H = lo, n - hi
 *     survivors = the APGPU_STACK_REJECT_MINMAX rule with nlow = L, nhigh = H on S (same ties)
 *   count, mean_f64, std_f64 and the weighted mean under APGPU_STACK_FRAME_PARAMS / APGPU_STACK_FRAME_LOCAL are formed word for word
 *   as for APGPU_STACK_REJECT_MINMAX.
 * The table (ops.esd_lambda computes it on the host): with m = n - i values left, p = 1 - alpha / (2 m) and t the p-quantile of
 * Student's t with m - 2 degrees of freedom, lambda = (m - 1) t / sqrt((m - 2 + t^2) m); entries with i >= K_n and rows n < 4
 * hold +inf. */
#define APGPU_STACK_REJECT_ESD 256
typedef struct apgpu_stack_esd {
    const double *lambda;            /* device float64 [n_frames + 1][max_outliers]: lambda[n * max_outliers + i] */
    int32_t max_outliers;            /* 1 .. 64 */
    int32_t reserved;                /* 0 */
    const apgpu_stack_local *local;  /* host; non-NULL iff APGPU_STACK_FRAME_LOCAL is set */
} apgpu_stack_esd;

/* The two-kernel scheme and its workspace.  A clipped stack of up to 128 frames (and the chunked kernel for 129 .. 512) with
 * lean outputs runs as a FAST kernel - the float32 fast path alone, four wavefronts per SIMD - followed by a REDO PASS of the
 * complete kernel over what the fast kernel could not finish: single pixels (unsure comparisons, non-finite values, masked
 * pixels, operands outside the guards of the fast division) gathered from per-segment lists, and whole 256-pixel tiles that
 * (in 64-pixel blocks) the fast kernel gave up without trying once more than an eighth of the pixels it had seen were failing - so that a stack
 * whose pixels mostly fail costs about one pass of the complete kernel, not both kernels in full.  The lists, counters and
 * tile flags live in `workspace`:
 *   - size: apgpu_stack_ws_bytes(n_pixels, &zero_bytes) bytes (about 4 bytes per pixel), 16-byte aligned;
 *   - its first zero_bytes bytes must be ZERO at the first call (hipMemsetAsync once; zeroing all of it is fine); every call
 *     leaves them zero again (the statistics and one mode word excepted, below).  After a call that returned an error, zero
 *     them again;
 *   - the layout depends on n_pixels: a workspace serves calls of ONE n_pixels (re-zero the prefix before using it for
 *     another image size) and must not be shared by calls that may run concurrently (two streams);
 *   - the 32 bytes at APGPU_STACK_WS_STATS_OFFSET hold four int64 counters, cumulative over the calls that used this
 *     workspace and never reset by the library: calls, pixels, pixels listed, 64-pixel blocks given up (apgpu_stack_ws_stats) -
 *     the caller may copy them out (after the stream has been synchronised) to see which fraction of its data leaves the fast
 *     path: (pixels_listed + 64 * blocks_given_up) / pixels;
 *   - the workspace also remembers, from one call to the next, whether the guard is needed: a call that sent under an eighth
 *     of its pixels to the redo pass (listed, or in blocks given up) lets the next call on the same workspace skip the fast
 *     kernel's look at the counters (it costs 1.5 % of the benchmark, 6 % of a 16-frame stack); the first call after the data has turned bad therefore runs unguarded - both
 *     kernels in full, measured 1.20 - 1.25 x the complete kernel's time when every column fails (profiles/r05/redo_sweep.txt)
 *     - and sets the guard for the calls after it.
 *     The ccdproc.combine configuration (one pass of median / mad_std) keeps a mode word of its own in the same line: after a call
 *     that gave up more than an eighth of its sampled 64-pixel blocks, the next call tries only every 16th tile on the fast kernel.
 * workspace == NULL: the call allocates and frees a stream-ordered temporary of the same size itself (hipMallocAsync /
 * hipMemsetAsync / hipFreeAsync on `stream` - three more runtime calls per stack; the only place where the library
 * allocates); if that fails too, or with APGPU_STACK_SINGLE_KERNEL, the complete kernel reduces the whole stack in one launch. */
#define APGPU_STACK_WS_STATS_OFFSET 16384
typedef struct apgpu_stack_ws_stats {
    int64_t calls, pixels, pixels_listed, blocks_given_up;
} apgpu_stack_ws_stats;
size_t apgpu_stack_ws_bytes(int64_t n_pixels, size_t *zero_bytes);

int apgpu_stack_sigclip(const apgpu_stack_args *args, void *stream);

/* A6 on FLOAT64 frames (BITPIX -64 inputs of ApMasterCal: ccdproc's Combiner is float64 throughout, so such frames must
 * not pass through the float32 stack kernels): base = median, dev = mad_std, ONE strict pass, float64 mean in frame order, std
 * of the kept values, survivor count.  `form` selects which published Combiner.sigma_clipping is followed, operation for
 * operation (oracle/apref.c apref_combine_ccdproc_form, golden group G12 - both forms run for real):
 *   APGPU_CCDPROC_ASTROPY (ccdproc >= 2.2, what requirements.txt:18 resolves to today): astropy.stats.sigma_clip - rejected
 *       where x < base - dev * low or x > base + dev * high; a column holding a non-finite value is not clipped at all;
 *   APGPU_CCDPROC_LEGACY  (ccdproc <= 2.1): rejected where x - base < -low * dev or x - base > high * dev; non-finite values
 *       are masked and the rest is clipped.
 * frames: double [N][P] with frame_stride elements between frames (0 = n_pixels); outputs may be NULL; workspace:
 * double[2][N][P] (apgpu_combine_ccdproc_f64_ws_bytes).  A correctness path (insertion sort per pixel). */
#define APGPU_CCDPROC_ASTROPY 0
#define APGPU_CCDPROC_LEGACY 1
size_t apgpu_combine_ccdproc_f64_ws_bytes(int32_t n_frames, int64_t n_pixels);
int apgpu_combine_ccdproc_f64(const double *frames, int32_t n_frames, int64_t n_pixels, int64_t frame_stride, double low,
                              double high, int32_t form, double *mean, int32_t *count, double *std, void *workspace,
                              size_t workspace_bytes, void *stream);

/* Plain median along N (np.nanmedian(axis=0)); config 4.  Optional fused calibration as above. */
int apgpu_stack_median(const apgpu_stack_args *args, void *stream);

/* Name of the kernel variant apgpu_stack_sigclip (median_only == 0) / apgpu_stack_median (!= 0) dispatches for `args`
 * (slot count, raw type, fused calibration, rich / lean, full / padded), as rocprofv3 prints it without the namespace,
 * e.g. "stack_sigclip_kernel<64, float, true, false, true>".  Launches nothing; name_host is a HOST buffer. */
int apgpu_stack_kernel_name(const apgpu_stack_args *args, int median_only, char *name_host, size_t name_bytes);

/* mean = sum / cnt from all-reduced float32 moments (planes sum, cnt; cnt == 0 -> NaN).  `std` must be NULL:
 * sumsq / cnt - mean^2 from float32 sums about zero cancels catastrophically for CCD-range data (APGPU_EUNSUPPORTED);
 * use the float64 layout for a standard deviation. */
int apgpu_moments_finalize(const float *moments, float *mean, float *std, int64_t n_pixels, void *stream);

/* The float64 layout: mean = sum / cnt and std = sqrt(max(sumsq / cnt - mean^2, 0)) evaluated in float64, stored as
 * float32 (mean, std) and/or float64 (mean_f64, std_f64); every output may be NULL; sumsq may be NULL if no std is
 * wanted; cnt == 0 -> NaN. */
int apgpu_moments_finalize_f64(const double *sum, const double *sumsq, const int32_t *count, float *mean, float *std,
                               double *mean_f64, double *std_f64, int64_t n_pixels, void *stream);

/* The packed float64 layout (moments_f64 == 3 / 4): the three planes as pointers (buffer, buffer + P, buffer + 2 P);
 * sumsq may be NULL if no std is wanted; count == 0 -> NaN. */
int apgpu_moments_finalize_f64p(const double *sum, const double *count, const double *sumsq, float *mean, float *std,
                                double *mean_f64, double *std_f64, int64_t n_pixels, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A3  astropy.stats.sigma_clipped_stats(data, sigma) with axis=None as called at
 *     core/ApFindBadPixels.py:191 (astropy/stats/sigma_clipping.py:385-433, numpy nan-functions):
 *     global iterative clip of an image with numpy's arithmetic reproduced exactly (exact median by
 *     radix select, numpy-ordered pairwise sums):
 *       _f32: float32 data, float32 statistics (float32 masters);
 *       _f64: float64 data and statistics - what numpy computes for integer images (the caller widens
 *             uint16/int16 pixels exactly) and for float64 data.
 *     Results stay on the device: stats_out[10] float64 =
 *       { mean, median, std, lo, hi, iterations, survivors, min, max, reserved }
 *     (lo/hi = bounds of the last pass; min/max of the survivors).  maxiters < 0 = until convergence.
 * ------------------------------------------------------------------------------------------- */
size_t apgpu_sigclip_global_ws_bytes(int64_t n_pixels);
int apgpu_sigclip_global_f32(const float *data, int64_t n_pixels, double sigma_lower, double sigma_upper,
                             int maxiters, double *stats_out, void *ws, size_t ws_bytes, void *stream);
size_t apgpu_sigclip_global_f64_ws_bytes(int64_t n_pixels);
int apgpu_sigclip_global_f64(const double *data, int64_t n_pixels, double sigma_lower, double sigma_upper,
                             int maxiters, double *stats_out, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F5  ApAutoBadcols.process (core/ApAutoBadcols.py:180-258), the bad column / row finder of
 *     scripts/ap_auto_badcol.py:76-116.  dtype: APGPU_F32 or APGPU_F64; numpy takes the median of integers in
 *     float64, so uint16 images are APGPU_U16 below and other integer images are widened exactly by the caller.
 *     apgpu_axis_nanmedian: np.nanmedian(data, axis) of every frame of a slab [N][H][W] (:196, :200); axis 0 ->
 *       out [N][W] (per column), axis 1 -> out [N][H] (per row), in the data's dtype (APGPU_U16: float64 out, the
 *       pixels widened as they are read).  Exact order statistic of the non-NaN values; numpy 1.26's two paths are
 *       both reproduced: lines shorter than 600 go through np.ma.median (the middle value of an odd count is
 *       T(x + x) / 2), longer ones through np.median (the value itself); an even count gives T(a + b) / 2; an
 *       all-NaN line gives NaN.  n_frames <= 65535.
 *     apgpu_sliding_clipped_stats: _sliding_stats_1d (:143-167) and the flag of _process (:225-227) for n_lines
 *       lines of `length` values each: for every index i the window values[max(0, i - hw) : min(L, i + hw + 1)],
 *       hw = (window_len - 1) / 2, is clipped exactly as by the A3 entry points (astropy's noaxis clip,
 *       sigma_lower = sigma_upper = sigma; maxiters < 0 = until convergence) and
 *         mean[i], std[i]  = the clipped mean and std (float64 holding values of the dtype),
 *         nsig[i]          = |float64(values[i]) - mean[i]| / std[i]   (float64; std == 0 gives inf or NaN),
 *         flag[i]          = nsig[i] >= nsigma                         (uint8 0 / 1; NaN is not bad).
 *       window_len >= 1 (a window longer than the line is cut at both ends); ws >= the _ws_bytes value.
 * ------------------------------------------------------------------------------------------- */
int apgpu_axis_nanmedian(const void *data, int dtype, int64_t n_frames, int64_t height, int64_t width, int axis, void *out,
                         void *stream);
size_t apgpu_sliding_clipped_stats_ws_bytes(int dtype, int64_t n_lines, int64_t length, int64_t window_len);
int apgpu_sliding_clipped_stats(const void *values, int dtype, int64_t n_lines, int64_t length, int64_t window_len, double sigma,
                                int maxiters, double nsigma, double *mean, double *std, double *nsig, uint8_t *flag, void *ws,
                                size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F2  ApImageDifference (scripts/ap_calc_read_noise.py:122): out = float64(a) - float64(b) where neither
 *     bad1 nor bad2 (uint8, non-zero = bad, either may be NULL) flags the pixel, NaN elsewhere; feed
 *     `out` to apgpu_sigclip_global_f64 (maxiters 1, huge sigma) for np.std/mean/median/min/max of
 *     diff[good] in numpy's order.  a, b: APGPU_F32 or APGPU_U16.
 * ------------------------------------------------------------------------------------------- */
int apgpu_image_difference_f64(const void *a, const void *b, int dtype, const uint8_t *bad1, const uint8_t *bad2,
                               double *out, int64_t n_pixels, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A4  ApFindBadPixels._generate_sigmaclip_mask (core/ApFindBadPixels.py:194-216):
 *     mask = (data < f32(lo)) | (data > f32(hi)) as uint8; nbad_out[0] (device int64) = sum(mask).
 *     If thresholds_dev != NULL the two float64 thresholds are read from the device
 *     (thresholds_dev[0], [1]) instead of the by-value arguments, so A3 -> A4 chains without a sync.
 * ------------------------------------------------------------------------------------------- */
int apgpu_threshold_mask_f32(const float *data, int64_t n_pixels, double lothresh, double hithresh,
                             const double *thresholds_dev, uint8_t *mask, int64_t *nbad_out, void *stream);

/* A4 user overlays (core/ApFindBadPixels.py:70-158): mask[r0:r1, c0:c1] += value for n_rects
 * 0-based half-open rectangles rects[n][4] = {r0, r1, c0, c1} (device int32). uint8 wrap-around. */
int apgpu_mask_add_rects_u8(uint8_t *mask, int64_t height, int64_t width, const int32_t *rects,
                            int32_t n_rects, int32_t value, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A5  ApFixBadPixels.fix_bad_pixels (core/ApFixBadPixels.py:292-445): every pixel with mask != 0
 *     becomes the median of the good pixels of the ORIGINAL image inside the (2*deltapix+1)^2 window
 *     clipped to the image, if at least min_valid of them exist; otherwise it is left unchanged.
 *     out may not alias data.  stats_out[3] (device int64) = { nbad, nfixed, nremaining }.
 *     Any deltapix >= 0 (register-resident sorting networks for 1..3, rank counting beyond); any alignment of
 *     data/out (a frame cut out of a slab).  _f64: the same on a float64 image, medians in float64 - what the
 *     reference computes after a float64 calibration (np.median in the input's dtype).
 * ------------------------------------------------------------------------------------------- */
int apgpu_fix_badpix_f32(const float *data, const uint8_t *mask, int64_t height, int64_t width,
                         int32_t deltapix, int32_t min_valid, float *out, int64_t *stats_out, void *stream);
int apgpu_fix_badpix_f64(const double *data, const uint8_t *mask, int64_t height, int64_t width,
                         int32_t deltapix, int32_t min_valid, double *out, int64_t *stats_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A8  ApImArith.process_files op block (core/ApImArith.py:320-333): out = a (op) b, with b an image
 *     (b != NULL) or the scalar float32(scalar).  APGPU_F32: IEEE float32.  APGPU_U16: image (op)
 *     image only, ADD/SUB/MUL wrap modulo 2^16 (numpy); DIV and scalar operands are rejected with
 *     APGPU_EUNSUPPORTED just as numpy raises UFuncTypeError.
 * ------------------------------------------------------------------------------------------- */
int apgpu_imarith(const void *a, const void *b, double scalar, int op, int dtype, void *out,
                  int64_t n_pixels, void *stream);
/* The float64 cases of the same block: a float64 image (op) image / scalar, and float32 (op) float64 image pairs -
 * NumPy computes in float64 as soon as one operand ARRAY is float64 and stores in the dtype of `a`
 * (np.add(data1, data2, out=zeros_like(data1)), same_kind casting).  a_dtype / b_dtype: APGPU_F32 | APGPU_F64. */
int apgpu_imarith_f64(const void *a, int a_dtype, const void *b, int b_dtype, double scalar, int op, void *out,
                      int64_t n_pixels, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A9  RawConv split geometry (core/RawConv.py:111-128, 163-190): planes[k] = where(colour == k,
 *     max(raw - black[k], 0), 0) for k = R0 G1 B2 G2 3, full-size planes [4][H][W].
 *     pattern_host[4] = colour of cell positions (0,0),(0,1),(1,0),(1,1); black_host may be NULL.
 * ------------------------------------------------------------------------------------------- */
int apgpu_bayer_split_u16(const uint16_t *raw, int64_t height, int64_t width, const int32_t *pattern_host,
                          const int32_t *black_host, uint16_t *planes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F1  FITS payload <-> device arrays: what astropy.io.fits does at core/ApCalibrate.py:270-277 (read,
 *     uint=True) and :392-399 (write).  `payload` is the big-endian data unit exactly as in the file
 *     (device copy of the raw bytes).
 *     decode: BITPIX 16 with unsigned16 != 0 (BSCALE 1, BZERO 32768) -> uint16[n];
 *             BITPIX 16 with unsigned16 == 0 -> float32[n] (integers are converted to float32 at read
 *             time, core/ApCalibrate.py:304-307); BITPIX -32 -> float32[n]; BITPIX 32 -> int32[n];
 *             BITPIX -64 -> float64[n]; BITPIX 64 -> int64[n].
 *     encode: float32[n] -> big-endian BITPIX -32 payload; float64[n] -> BITPIX -64 payload.
 * ------------------------------------------------------------------------------------------- */
int apgpu_fits_decode(const void *payload, int bitpix, int unsigned16, void *out, int64_t n_pixels, void *stream);
int apgpu_fits_encode_f32(const float *data, void *payload, int64_t n_pixels, void *stream);
int apgpu_fits_encode_f64(const double *data, void *payload, int64_t n_pixels, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F3  Affine Lanczos-3 resample of registered frames - the step the reference hands to SWarp
 *     (scripts/resample_all.sh:123-131 RESAMPLING_TYPE LANCZOS3; :298 FSCALE = 1/EXPTIME; :330-342 the call).
 *     frames [n_frames, h_in, w_in] float32; mask [h_in, w_in] uint8 shared by all frames, or NULL;
 *     affines [n_frames][6] float64 (device): xin = A0*x + A1*y + A2, yin = A3*x + A4*y + A5 maps OUTPUT
 *     pixel (x = column, y = row, 0-based) to INPUT coordinates.  With affines_per_tile != 0 the array is
 *     [n_frames][tiles_y][tiles_x][6], one transform per APGPU_RESAMPLE_TILE_H x APGPU_RESAMPLE_TILE_W tile of the
 *     output (tiles_y = ceil(h_out / TILE_H), tiles_x = ceil(w_out / TILE_W); x, y stay absolute): a piecewise-
 *     affine form of a smooth non-linear registration such as TAN -> TAN through the sky (wcs.tile_affines).
 *     conserve_flux != 0 multiplies every pixel by |A0*A4 - A1*A3|, the area of an output pixel in input pixels
 *     (SWarp's FSCALASTRO_TYPE VARIABLE, resample_all.sh:129: total flux, not surface brightness, is preserved); fscale [n_frames] float32 or NULL (= 1);
 *     lut [n_phases + 1][6] float32 (device, 8-byte aligned): row p = normalised Lanczos-3 weights of the
 *     taps floor(xin)-2 .. floor(xin)+3 for the fractional offset p / n_phases (ops.lanczos3_table).
 *     out [n_frames, h_out, w_out] float32 = NaN where any of the 36 taps is outside the frame, masked or
 *     non-finite; weight_out (uint8, same shape, or NULL) = 1 where out is defined.  The co-add itself
 *     (COMBINE_TYPE MEDIAN / AVERAGE / SUM / CLIPPED) is apgpu_stack_median / apgpu_stack_sigclip on `out`:
 *     both skip the NaN pixels.  Exact definition: oracle/apref.c apref_resample_affine_f32.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_RESAMPLE_TILE_H 16
#define APGPU_RESAMPLE_TILE_W 64
int apgpu_resample_affine_f32(const float *frames, int32_t n_frames, int64_t h_in, int64_t w_in, const uint8_t *mask,
                              const double *affines, int32_t affines_per_tile, int32_t conserve_flux, const float *fscale,
                              const float *lut, int32_t n_phases, float *out, uint8_t *weight_out, int64_t h_out,
                              int64_t w_out, void *stream);

/* F3 (continued)  SWarp's OVERSAMPLING n (resample_all.sh:112, 339: 4) in one pass: every output pixel is the mean of n x n
 *     interpolations at the centres of its sub-pixels.  fine_affines maps pixel (u, v) of the n-times FINER grid - output
 *     pixel (x, y) owns u = n x .. n x + n - 1, v = n y .. n y + n - 1 - to input coordinates (ops.oversampled_affines, or
 *     wcs.tile_affines of the n-times finer WCS); with affines_per_tile != 0 there is one transform per TILE_H x TILE_W tile
 *     of the OUTPUT grid, [n_frames][tiles_y][tiles_x][6].  Each sub-sample is apgpu_resample_affine_f32's value at (u, v)
 *     (flux scale, conserve_flux = |det| of the fine transform, NaN rules included); out = (float)(sum * (1.0 / n^2)) with the
 *     sum accumulated in float64 in row-major order (v outer, u inner) - bit-identical to apgpu_block_mean_f32 of the fine
 *     resample, without the n^2-times larger image ever existing.  oversampling 1..16 (1 = apgpu_resample_affine_f32).
 *     Exact definition: oracle/apref.c apref_resample_oversampled_f32. */
int apgpu_resample_oversampled_f32(const float *frames, int32_t n_frames, int64_t h_in, int64_t w_in, const uint8_t *mask,
                                   const double *fine_affines, int32_t affines_per_tile, int32_t conserve_flux, const float *fscale,
                                   const float *lut, int32_t n_phases, int32_t oversampling, float *out, uint8_t *weight_out,
                                   int64_t h_out, int64_t w_out, void *stream);

/* F3 (continued)  The two-step form of OVERSAMPLING, and COMBINE_TYPE WEIGHTED.
 *     apgpu_block_mean_f32: OVERSAMPLING n (resample_all.sh:112, 339: 4) - the frame is resampled onto a grid n times finer
 *     (apgpu_resample_affine_f32 with the transform of the sub-pixel centres) and every output pixel is the mean of its
 *     n x n sub-samples: fine [n*h_out, n*w_out] float32 -> out [h_out, w_out] float32, float64 accumulation in row-major
 *     order inside the block, NaN if any sub-sample is NaN.
 *     apgpu_weighted_mean_f32: COMBINE_TYPE WEIGHTED (resample_all.sh:65-68) with one weight per frame (SWarp with
 *     WEIGHT_TYPE NONE weighs a frame by the inverse variance of its scaled background noise): per pixel
 *     mean = sum_i w_i x_i / sum_i w_i over the frames whose resampled value is finite (float64 accumulation in frame
 *     order), wsum_out = that sum of weights = the -WEIGHTOUT_NAME image (resample_all.sh:342); NaN / 0 where no frame
 *     contributes.  weights [n_frames] float32 on the device, all finite and > 0. */
int apgpu_block_mean_f32(const float *fine, int64_t h_out, int64_t w_out, int32_t oversampling, float *out, void *stream);

/* F3 + A7 in one launch: the co-add of scripts/resample_all.sh:330-342 (one SWarp call: resample every frame, combine) without
 * the resampled slab.  Every output pixel's N values are apgpu_resample_affine_f32's values for it (same tile records, same window
 * arithmetic, bit for bit; oversampling 1) and their reduction is apgpu_stack_sigclip's lean one (mean / count / moments, centre
 * median or mean, deviation std): NaN ("frame absent": a window off the frame, on a bad pixel or on a non-finite value) is
 * skipped as there.  `args` is the stack's argument block with: frames = the INPUT frames [n_frames][h_in * w_in] float32
 * (frame_stride 0 = h_in * w_in), n_frames <= 16 per call, n_pixels = h_out * w_out, no fused calibration, no pixmask, outputs
 * among mean / count / moments, flags among APGPU_STACK_EXACT_MOMENTS / APGPU_STACK_MOMENTS_MEAN; its workspace fields are not
 * used.  The other arguments are apgpu_resample_affine_f32's.  workspace: apgpu_resample_stack_ws_bytes(..) bytes, 64-byte
 * aligned, caller-owned, need not be initialised: tile records, and with a mask the bad-pixel list and one uint32 per output
 * pixel (which frames' windows hold a bad pixel).  HBM traffic 4 n_frames P + 4 P instead of 12 n_frames P + 4 P. */
size_t apgpu_resample_stack_ws_bytes(int32_t n_frames, int64_t h_in, int64_t w_in, int64_t h_out, int64_t w_out, int32_t has_mask);
int apgpu_resample_stack_sigclip(const apgpu_stack_args *args, int64_t h_in, int64_t w_in, const uint8_t *mask,
                                 const double *affines, int32_t affines_per_tile, int32_t conserve_flux, const float *fscale,
                                 const float *lut, int32_t n_phases, int64_t h_out, int64_t w_out, void *workspace,
                                 size_t workspace_bytes, void *stream);
int apgpu_weighted_mean_f32(const float *slab, int32_t n_frames, int64_t n_pixels, const float *weights, float *mean_out,
                            float *wsum_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F4  Sky-background mesh of ApMeasureBackground (core/ApMeasureBackground.py:142-175, 382-415).  The reference calls
 *     photutils (detect_threshold / detect_sources / make_source_mask, Background2D with MedianBackground + SigmaClip,
 *     BkgZoomInterpolator); photutils is not in the build container, so these entry points implement its published
 *     algorithms as restated in oracle/background_ref.py (parity with photutils itself is unpinned).
 *
 *     apgpu_source_mask_u8: `above` [H][W] uint8 (non-zero = pixel above the detection threshold, e.g. from
 *       apgpu_threshold_mask_f32) -> 8-connected components, components with fewer than min_pixels pixels dropped
 *       (detect_sources(npixels)), the rest dilated with a dilate_size x dilate_size square
 *       (SegmentationImage.make_source_mask(size)); mask_out [H][W] uint8 0/1; nsources_out[0] (device int64, may be
 *       NULL) = surviving components.
 *     apgpu_box_clipped_stats_f32: the image is cut into box_height x box_width boxes (the last row / column of boxes
 *       may stick out of the image: those pixels count as masked, Background2D's edge_method 'pad'); per box astropy's
 *       SigmaClip(sigma, maxiters, median / std) over the unmasked finite pixels; stats_out[ny][nx][4] (device float64)
 *       = { median, std, count of the final survivors, pixels masked before clipping }.
 *     apgpu_spline_zoom_f64: scipy.ndimage.zoom(mesh, (zoom_y, zoom_x), order=3, mode='reflect', grid_mode=True)[:H, :W]
 *       from the prefiltered cubic B-spline coefficients coef[ny][nx] (device float64), clipped to [vmin, vmax].
 * ------------------------------------------------------------------------------------------- */
size_t apgpu_source_mask_ws_bytes(int64_t height, int64_t width);
int apgpu_source_mask_u8(const uint8_t *above, int64_t height, int64_t width, int32_t min_pixels, int32_t dilate_size,
                         uint8_t *mask_out, int64_t *nsources_out, void *ws, size_t ws_bytes, void *stream);
int apgpu_box_clipped_stats_f32(const float *data, const uint8_t *mask, int64_t height, int64_t width, int32_t box_height,
                                int32_t box_width, double sigma, int32_t maxiters, double *stats_out, void *stream);
int apgpu_spline_zoom_f64(const double *coef, int32_t ny, int32_t nx, int32_t zoom_y, int32_t zoom_x, int64_t height,
                          int64_t width, double vmin, double vmax, double *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F4  L.A.Cosmic, the step ApFixCosmicRays.process hands to ccdproc.cosmicray_lacosmic -> astroscrappy.detect_cosmics
 *     (core/ApFixCosmicRays.py:267-295).  Neither package is in the build container: the entry points implement the
 *     algorithm as restated in oracle/lacosmic_ref.py (parity with astroscrappy itself is unpinned).  Images are float32 in
 *     ELECTRONS (the caller multiplies by the gain, as ccdproc does with gain_apply = True).
 *     apgpu_sepmedfilt_f32: median of `size` (5, 7 or 9) along rows, then along columns, borders copied (astroscrappy's
 *       separable median filters); ws >= 4 * H * W bytes.
 *     apgpu_lacosmic_satmask: astroscrappy's update_mask - cores of saturated stars (data >= satlevel where the 7-median
 *       exceeds satlevel / 10) dilated twice with the 5 x 5 kernel, OR inmask (may be NULL) grown by one pixel.
 *     apgpu_lacosmic_iterate: ONE detect_cosmics iteration, in place on clean / crmask: Laplacian of the 2x subsampled
 *       image, noise model sqrt(max(sepmed7, 1e-5) + readnoise^2), fine-structure image from the 7 x 7 kernel psfk (device,
 *       49 floats; NULL = fsmode 'median'), sp > sigclip and sp / f > objlim, two 3 x 3 growth steps (sp > sigclip, then
 *       sp > sigfrac * sigclip), 'meanmask' cleaning over 5 x 5 with background_level where no good neighbour exists;
 *       ncr_out[0] (device int64) = cosmic-ray pixels found in this iteration (the caller stops at 0).
 *     ws >= apgpu_lacosmic_ws_bytes(H, W) for the last two.
 * ------------------------------------------------------------------------------------------- */
size_t apgpu_lacosmic_ws_bytes(int64_t height, int64_t width);
int apgpu_sepmedfilt_f32(const float *data, int64_t height, int64_t width, int32_t size, float *out, void *ws, size_t ws_bytes,
                         void *stream);
int apgpu_lacosmic_satmask(const float *data, const uint8_t *inmask, int64_t height, int64_t width, float satlevel,
                           uint8_t *mask_out, void *ws, size_t ws_bytes, void *stream);
int apgpu_lacosmic_iterate(float *clean, const uint8_t *mask, uint8_t *crmask, int64_t height, int64_t width, float sigclip,
                           float sigfrac, float objlim, float readnoise, const float *psfk, float background_level,
                           int64_t *ncr_out, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F6  ApFindStars (core/ApFindStars.py:87-201 the constructor, :299-340 source_search, :363-446 aperture_photometry).
 *     The reference calls photutils (DAOStarFinder, find_peaks, aperture_photometry), which is not in the build container: the
 *     entry points implement the published DAOFIND algorithm (Stetson 1987) as restated in tests/findstars_model.py (parity
 *     with photutils itself is unpinned); the annulus statistic is astropy's sigma_clipped_stats (golden group G16).
 *     These entry points need no workspace.
 *
 *     apgpu_daofind_convolve_f32: out[i][j] = float32( sum_{a,b} kernel[a][b] * d[i + R - a][j + R - b] ), d = data - bg_median
 *       (one float32 subtraction) inside the image and 0 outside it; kernel [(2R+1)][(2R+1)] float64 on the device (the zero-sum
 *       DAOFIND kernel, ops.daofind_kernel); all taps in row-major (a, b) order, float64, multiply and add separately
 *       rounded.  1 <= radius <= 12 (APGPU_EUNSUPPORTED beyond: fwhm too large).
 *     apgpu_local_peaks_f32: pixel p is a peak when no pixel under the footprint (uint8 [fp_height][fp_width], non-zero = member,
 *       centred at index size / 2 per axis; a member outside the image holds 0) exceeds values[p], float64(values[p]) >
 *       threshold (strict), mask[p] == 0 (mask may be NULL) and p lies at least `border` pixels from every image edge.  Peaks go
 *       into list[capacity] (int32 flat indices, in no particular order: sort them) through a counter: count_out[0] (device
 *       int32) is ALWAYS the true number of peaks, the list is written only below `capacity` - count_out[0] > capacity tells
 *       the caller to call again with a larger list.  height * width < 2^31; the footprint is at most 64 x 64.
 *     apgpu_daofind_measure: per candidate (flat index of a peak at least `radius` from every edge) the DAOFIND quantities from
 *       the (2R+1)^2 cut-outs of d and of the convolved image: records[n][16] float64 = x_peak, y_peak, npix, peak, conv_peak,
 *       sharpness, roundness1, roundness2, dx, dy, hx, hy, xcentroid, ycentroid, flux, mag; keep[n] uint8 = 1 where the candidate
 *       passes the rejection rules (positive fit amplitudes, sharpness / roundness strictly inside their limits, centroid shift
 *       <= radius, finite values).  tables [6][(2R+1)^2], quad [(2R+1)^2] and consts [18] float64 on the device are the per-tap
 *       weights and fit constants ops.daofind_kernel builds (consts: npixels - 1, threshold_eff, sharplo, sharphi, roundlo,
 *       roundhi, sigma^2, p, then sumg, sumgsq, sdgd, sdgds, sgdgd for x and for y).
 *     apgpu_aperture_phot_f32: per source (xc, yc: float64, x = column) sum_raw = sum overlap * data over the pixels the circle
 *       of r_aperture touches (exact circle / pixel-square overlap areas, pixel (i, j) covers [j - 0.5, j + 0.5] x [i - 0.5,
 *       i + 0.5], pixels outside the image contribute nothing), area = the sum of those overlaps, n_annulus = pixels of the
 *       image whose centre has r_in^2 <= d^2 <= r_out^2, bkg_median = median of astropy's sigma_clipped_stats(annulus values,
 *       sigma, maxiters) - non-finite values dropped, numpy's float32 arithmetic as apgpu_sigclip_global_f32 - or NaN if none
 *       is left.  An annulus is held on chip: pi ((r_out + sqrt(1/2))^2 - (r_in - sqrt(1/2))^2) <= 4096 (APGPU_EUNSUPPORTED
 *       beyond; r_in = 30, r_out = 45 fits).
 * ------------------------------------------------------------------------------------------- */
int apgpu_daofind_convolve_f32(const float *data, int64_t height, int64_t width, const double *kernel, int32_t radius,
                               float bg_median, float *out, void *stream);
int apgpu_local_peaks_f32(const float *values, int64_t height, int64_t width, const uint8_t *footprint, int32_t fp_height,
                          int32_t fp_width, double threshold, const uint8_t *mask, int32_t border, int32_t *list,
                          int32_t capacity, int32_t *count_out, void *stream);
int apgpu_daofind_measure(const float *data, const float *conv, int64_t height, int64_t width, const int32_t *candidates,
                          int32_t n_candidates, int32_t radius, float bg_median, const double *tables, const double *quad,
                          const double *consts, double *records, uint8_t *keep, void *stream);
int apgpu_aperture_phot_f32(const float *data, int64_t height, int64_t width, const double *xc, const double *yc,
                            int32_t n_sources, double r_aperture, double r_in, double r_out, double sigma, int32_t maxiters,
                            double *sum_raw, float *bkg_median, int32_t *n_annulus, double *area, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F7  ApMeasureStars (core/ApMeasureStars.py:223-430): weighted least-squares fits of A exp(-(a du^2 + b du dv + c dv^2)) + B
 *     (astropy's Gaussian2D + Const2D; a, b, c from x_stddev, y_stddev, theta) to n square cut-outs of a float32 image, one
 *     wavefront per star, float64.  The cut-out of star s is img[box_y[s] .. + box_width)[box_x[s] .. + box_width); u is the
 *     ROW index and v the column index inside it (np.mgrid: the reference's axes, kept).  Weights 1 / sd with v = d > 0 ? d : 1,
 *     sd = v != 1 ? sqrt(v) : sqrt(mean of the v != 1), in the reference's float32 arithmetic; no v != 1 at all: not fitted.
 *     init [n][7] and the first 7 entries of a record are A, x_stddev, y_stddev, theta, B, x_mean, y_mean (APGPU_GAUSS2D_*).
 *     Levenberg-Marquardt with the analytic Jacobian in the reference's three stages (4, 5, 7 leading parameters free; a stage
 *     runs if the one before converged; at most max_iter iterations each; a stage ends when every step is <= 1e-10 of its
 *     parameter, or of the parameter's unit-weight error if that is larger).
 *     out_rec [n][APGPU_GAUSS2D_REC] float64: the parameters [0..7), their standard errors [7..14) (sqrt(diag((J^T W J)^-1)
 *     chi^2 / (box_width - n_free)): astropy's scaling, whose degrees of freedom count the ROWS of the 2-D grid; 0 for
 *     parameters not free in the last converged stage and when the fit is not ok), [14] chi^2 / (box_width^2 - n_free),
 *     [15] chi^2, [16..19) iterations per stage, [19] n_free of the last stage run.  out_ok [n] int32: 1 all three stages
 *     converged with a positive-definite matrix, 0 not, -1 the box does not lie inside the image (nothing read).
 *     box_width even, 12 .. APGPU_GAUSS2D_MAX_BOX (APGPU_EUNSUPPORTED above: the cut-out is held in LDS).
 *     All pointers but img's shape arguments are device pointers.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_GAUSS2D_REC 20
#define APGPU_GAUSS2D_MAX_BOX 76
#define APGPU_GAUSS2D_AMPL 0
#define APGPU_GAUSS2D_XSTD 1
#define APGPU_GAUSS2D_YSTD 2
#define APGPU_GAUSS2D_THETA 3
#define APGPU_GAUSS2D_BG 4
#define APGPU_GAUSS2D_XMEAN 5
#define APGPU_GAUSS2D_YMEAN 6
int apgpu_gauss2d_fit_f32(const float *img, int64_t height, int64_t width, const int32_t *box_y, const int32_t *box_x,
                          const double *init, int32_t n, int32_t box_width, int32_t max_iter, double *out_rec, int32_t *out_ok,
                          void *stream);

/* ---------------------------------------------------------------------------------------------
 * F8  ApRegister: relative registration of frames from their star lists by triangle similarity (Groth 1986, Valdes et al.
 *     1995).  The reference has no such step (it sends the list to astrometry.net); the rule is this project's own and is
 *     restated in tests/register_model.py (parity unpinned, the truth is a known synthetic transform).
 *     xy [n_frames][max_stars][2] float64 (x = column, y = row, 0-based, integer = pixel centre), count [n_frames] int32 the
 *     valid leading entries of each list, brightest first; frame 0 is the reference.  One launch covers all frames.  No
 *     workspace.
 *
 *     apgpu_triangle_build: every i < j < k among the first min(count[f], k) stars of frame f.  Squared sides dx*dx + dy*dy;
 *       sorted a2 >= b2 >= c2 by a stable sort of (side opposite i, side opposite j, side opposite k); x = sqrt(b2 / a2),
 *       y = sqrt(c2 / a2); v0, v1, v2 the vertices opposite the shortest, middle and longest side; orientation the sign (-1, 0,
 *       1) of (v1 - v0) x (v2 - v0).  Kept iff c2 >= min_side^2, y >= 0.1, x <= 0.98 and y <= 0.98 x.  Kept triangles of frame
 *       f go to tri_xy [f][tri_capacity][2] (x, y) and tri_v [f][tri_capacity] (v0 | v1 << 8 | v2 << 16 | (orientation + 1) <<
 *       24) in no particular order, their number to tri_count [f].  3 <= k <= APGPU_REGISTER_MAX_K and tri_capacity >=
 *       k (k-1) (k-2) / 6 (APGPU_EINVAL otherwise).
 *     apgpu_triangle_vote: for every frame f >= 1 and every (triangle r of frame 0, triangle t of frame f) with |x_r - x_t| <=
 *       eps and |y_r - y_t| <= eps (inclusive) and, unless allow_mirror, equal orientation: votes [f][v_r][v_t] += 1 for the
 *       three canonical vertex pairs.  votes [n_frames][k][k] int32 is zeroed by the call; votes [0] stays zero.  Integer
 *       sums: the result does not depend on how the work is split, and is the same on every run.
 *     apgpu_nearest_match: transforms [n_frames][6] float64, p = T_f(r) = ((a0 x + a1 y) + a2, (a3 x + a4 y) + a5) for a
 *       reference star r.  fwd_idx [f][i] = the star j of frame f nearest to T_f(r_i) with d2 = dx*dx + dy*dy <= radius^2
 *       (inclusive), fwd_d2 [f][i] that d2; bwd_idx [f][j] = the reference star i whose T_f(r_i) is nearest to star j of frame
 *       f, bwd_d2 [f][j] its d2.  Ties go to the lower index.  No star inside the radius, or an entry at or beyond the list's
 *       count: -1 and +inf.  All four outputs are [n_frames][max_stars]; max_stars <= APGPU_REGISTER_MAX_STARS.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_REGISTER_MAX_K 64
#define APGPU_REGISTER_MAX_STARS 4096
int apgpu_triangle_build(const double *xy, const int32_t *count, int32_t n_frames, int32_t max_stars, int32_t k, double min_side,
                         int32_t tri_capacity, double *tri_xy, int32_t *tri_v, int32_t *tri_count, void *stream);
int apgpu_triangle_vote(const double *tri_xy, const int32_t *tri_v, const int32_t *tri_count, int32_t n_frames,
                        int32_t tri_capacity, int32_t k, double eps, int32_t allow_mirror, int32_t *votes, void *stream);
int apgpu_nearest_match(const double *xy, const int32_t *count, const double *transforms, int32_t n_frames, int32_t max_stars,
                        double radius, int32_t *fwd_idx, double *fwd_d2, int32_t *bwd_idx, double *bwd_d2, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F9  ApComposite: the colour composite of three co-added planes, the step scripts/composite_all.sh hands to the external
 *     program STIFF.  STIFF is not in the reference tree, so the arithmetic below is this project's own definition, restated in
 *     tests/composite_model.py (parity unpinned).  planes [3][height][width] float32 (red, green, blue), all
 *     float32 arithmetic in the stated order, no contraction.
 *
 *     apgpu_quantile_levels_f32: q [3][2] float64 (min and max quantile of each channel, 0 .. 1), manual [3][2] float32 or NULL
 *       (an entry that is not NaN replaces that level).  With v[0 .. n) the finite values of a channel in ascending order of
 *       their order-preserving keys (-0.0 below +0.0), the level of q is v[floor(q (n - 1))], the product in float64
 *       (np.quantile, method 'lower'): an exact order statistic by radix select, all six in the same four reads of the planes,
 *       no host synchronisation.  n = 0: NaN.  levels [3][2] float32 (lo, hi per channel) and n_finite [3] int64 are written on
 *       the device.  The workspace is small and does not depend on the image size.
 *     apgpu_composite_rgb: n_variants (1 .. APGPU_COMPOSITE_MAX_VARIANTS) images from one read of the planes.  Variant v has a
 *       tone table tables [v][APGPU_TONE_TABLE_LEN] float32 and a saturation colour_sat_host [v] (HOST array).  Per pixel, with
 *       pos(a) = a > 0 ? a : 0 (NaN gives 0):
 *           scale_c = hi_c > lo_c ? 1 / (hi_c - lo_c) : 0         (IEEE division; NaN levels give 0)
 *           s_c = pos((x_c - lo_c) scale_c);   Y = ((s_0 + s_1) + s_2) float32(1/3)
 *           c_c = pos(Y + sat (s_c - Y));      o_c = c_c G(Y) < 1 ? c_c G(Y) : 1
 *           pixel_c = (unsigned)(o_c (2^bits - 1) + 0.5f);        any x_c not finite: the pixel is black in every variant
 *       G(Y) = T(Y) / Y of the luminance curve T comes from the table, indexed by the bits b of min(Y, 1): cell i = (b >> 15) -
 *       ((127 - 40) << 8) (256 knots per octave from 2^-40, entry 10240 = Y = 1), t = float32(b & 0x7fff) 2^-15, G = G[i] + t
 *       (G[i + 1] - G[i]) (subtract, multiply, add; at the closing knot t = 0 and G[i + 1] is not read); Y < 2^-40: G = 0.
 *       out [n_variants][height][width][3] uint8 (bits 8) or uint16 (bits 16), interleaved RGB; flip != 0: output row r is
 *       plane row height - 1 - r (FITS rows run bottom to top).  planes and out 4-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_COMPOSITE_MAX_VARIANTS 16
#define APGPU_TONE_TABLE_LEN 10241
size_t apgpu_quantile_levels_ws_bytes(int64_t height, int64_t width);
int apgpu_quantile_levels_f32(const float *planes, int64_t height, int64_t width, const double *q, const float *manual,
                              float *levels, int64_t *n_finite, void *ws, size_t ws_bytes, void *stream);
int apgpu_composite_rgb(const float *planes, int64_t height, int64_t width, const float *levels, const float *tables,
                        const float *colour_sat_host, int32_t n_variants, int32_t bits, int32_t flip, void *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F10 ApDebayer: Bayer demosaic, white-balance scaling and the sums behind the white balance (core/RawConv.py:291-366 white
 *     balance from the image, :401-486 rgb, :488-587 grey).  The reference leaves the interpolation to LibRaw, which is not in
 *     its tree, so the arithmetic below is this project's own definition, restated in tests/demosaic_model.py.
 *     All float32, one rounding per operation in the stated order, no contraction; NaN and inf propagate by IEEE rules.
 *
 *     pattern_host [4]: the colour (R 0, G1 1, B 2, G2 3) of cell position (r & 1) 2 + (c & 1), as in A9, here a Bayer arrangement
 *       (a permutation of 0 .. 3 with red and blue on one diagonal; APGPU_EINVAL otherwise).  black_host, gain_host: [4] float32
 *       HOST arrays by colour, NULL = zeros / ones; the black levels of uint16 data must be integers 0 .. 65535.
 *     sample   s(r, c) = float32(max(raw - black[k], 0)) gain[k] with k the colour of the site.  uint16: integer subtraction
 *       (RawConv._safe_subtract); float32: d = raw - black[k], d < 0 gives 0, NaN stays NaN.
 *     borders  an index is reflected about the edge sample (-1 -> 1, -2 -> 2, H -> H - 2), folded with period 2 (H - 1), so every
 *       tap keeps its colour.  height, width >= 2, odd sizes included.
 *     taps     C the site; N S W E its edge neighbours; NW NE SW SE the diagonals; N2 S2 W2 E2 at distance 2 on the axes;
 *       ns = N + S, we = W + E, d4 = (NW + NE) + (SW + SE), ns2 = N2 + S2, we2 = W2 + E2, e4 = ns + we, a4 = ns2 + we2.
 *     BILINEAR    own colour C.  At R/B: G = e4 0.25f, the other of R/B = d4 0.25f.  At G: the colour that shares the row =
 *       we 0.5f, the colour that shares the column = ns 0.5f.
 *     MHC         Malvar-He-Cutler 2004 in sixteenths.  Own colour C.  At R/B: G = ((8 C + 4 e4) - 2 a4) 2^-4, the other of R/B =
 *       ((12 C + 4 d4) - 3 a4) 2^-4.  At G: the colour of the row = (((10 C + 8 we) + ns2) - 2 (d4 + we2)) 2^-4, the colour of
 *       the column = (((10 C + 8 ns) + we2) - 2 (d4 + ns2)) 2^-4.
 *     SUPERPIXEL  height and width even; one output pixel per cell: R = s_R, G = (s_G1 + s_G2) 0.5f, B = s_B.
 *     RCD         ratio-corrected, edge-directed: modelled on RCD 2.x (L. Sanz Rodriguez), without its refinement passes; PARITY
 *       UNPINNED (LibRaw and librtprocess are absent), restated in tests/demosaic_rcd_model.py.  IEEE division.  s is extended to
 *       all integer positions by the folded reflection above; every intermediate plane outside the image is what the same
 *       formulas give on that extended mosaic (NOT a reflection of the intermediate plane).  eps = 2^-10, epssq = 2^-20, in
 *       sample units (powers of two: constant mosaics come back exactly); a float mosaic normalised to 0 .. 1 should be brought
 *       to ADU scale with gain.  s >= 0 or NaN, so every denominator is >= eps.  t(n): the plane n steps along the direction in
 *       question; d4(a) = (a(NW) + a(NE)) + (a(SW) + a(SE)); pair(g1, e1, g2, e2) = (g2 e1 + g1 e2) / (g1 + g2).
 *       1 statistics, all sites, along V and H:  h = (((t(-3) + t(3)) - (t(-1) + t(1))) - 3 (t(-2) + t(2))) + 6 s, q = h h,
 *         stat = (q(-1) + q(+1)) + q(0), stat < epssq gives epssq (a NaN stays);  VH = V / (V + H).
 *         vd = |0.5 - VH| < |0.5 - vn| ? vn : VH with vn = 0.25 d4(VH).
 *       2 low pass, R/B sites:  lpf = (s + 0.5 ((N + S) + (W + E))) + 0.25 d4(s).
 *       3 green at R/B sites.  Towards each of N, S, W, E (t steps that way):
 *           grad = (((eps + |t(1) - t(-1)|) + |s - t(2)|) + |t(1) - t(3)|) + |t(2) - t(4)|
 *           est  = t(1) (1 + (lpf - lpf(2)) / ((eps + lpf) + lpf(2)))
 *         V_est = pair(gN, eN, gS, eS), H_est = pair(gW, eW, gE, eE), G = vd H_est + (1 - vd) V_est.  At green sites G = s.
 *       4 diagonal statistics, R/B sites: stat of step 1 along NW-SE (P) and NE-SW (Q);  D = (P - Q) / (P + Q).
 *         (RCD's PQ = P / (P + Q) is (1 + D) / 2.  D changes its sign bit for bit when P and Q change places, which a mirrored
 *         mosaic makes them do; 1 - P / (P + Q) and Q / (P + Q) differ in the last bit, so PQ would not give mirrored planes.)
 *       5 the other of R/B at R/B sites:  dd = |D| < |dn| ? dn : D with dn = 0.25 d4(D).  Towards each diagonal d:
 *           grad = ((eps + |s(d) - s(-d)|) + |s(d) - s(3d)|) + |G - G(2d)|,  est = s(d) - G(d)
 *         P_est = pair(gNW, eNW, gSE, eSE), Q_est = pair(gNE, eNE, gSW, eSW),
 *         O = G + ((0.5 (1 - dd)) P_est + (0.5 (1 + dd)) Q_est).
 *       6 R and B at green sites, for each colour c: X = colour c at the R/B sites (s where native, O elsewhere), vd of step 1
 *         at this site.  Towards each of N, S, W, E:
 *           grad = ((eps + |G - G(2)|) + |X(1) - X(-1)|) + |X(1) - X(3)|,  est = X(1) - G(1)
 *         V_est, H_est as in step 3;  value = G + ((1 - vd) V_est + vd H_est).
 *       Nothing is clamped.  An output pixel depends on the samples within Chebyshev distance APGPU_DEMOSAIC_RCD_HALO (6 reads O
 *       at 3, O reads G at 2 diagonally, G reads vn at 1, whose V reads s at 4).  One launch, no workspace: a workgroup keeps the
 *       planes of a tile of APGPU_DEMOSAIC_RCD_TILE_H x APGPU_DEMOSAIC_RCD_TILE_W pixels and its halo in LDS.
 *     output      RGB_F32: out [n_frames][3][h][w] float32.  RGB_U16: the same as (uint16)(v > 0 ? (v < 65535 ? v : 65535) : 0),
 *       truncating, NaN gives 0 (np.clip + astype, RawConv.py:484-486).  GREY_F32: out [n_frames][h][w] = (0.299f R + 0.587f G) +
 *       0.114f B (CCIR 601, :550).  DIRECT_F32: out [n_frames][height][width] = s, the 'direct' luminance (:533-547); method is
 *       ignored.  (h, w) = (height, width), halved for SUPERPIXEL.  mosaic and out aligned to their element size; no workspace.
 *
 *     The channel sums are the device half of RawConv._get_whitebalance_from_region: rect_host [4] int64 = rowmin, rowmax, colmin,
 *     colmax, inclusive, clamped to the image.  For each colour, the sum of max(raw - black[k], 0) over its sites inside the
 *     rectangle and their number: uint16 data gives exact uint64 sums [4]; float32 data gives float64 sums [4] of the finite
 *     samples (in no fixed order) and counts them.  sums (8 bytes each) and counts [4] int64 are written on the device.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_DEMOSAIC_BILINEAR   0
#define APGPU_DEMOSAIC_MHC        1
#define APGPU_DEMOSAIC_SUPERPIXEL 2
#define APGPU_DEMOSAIC_RCD        4   /* 3 is no method and stays APGPU_EINVAL, as version 130 has refused it all along */
#define APGPU_DEMOSAIC_RCD_TILE_H 32
#define APGPU_DEMOSAIC_RCD_TILE_W 64
#define APGPU_DEMOSAIC_RCD_HALO   10
#define APGPU_DEMOSAIC_RGB_F32    0
#define APGPU_DEMOSAIC_RGB_U16    1
#define APGPU_DEMOSAIC_GREY_F32   2
#define APGPU_DEMOSAIC_DIRECT_F32 3
int apgpu_bayer_demosaic(const void *mosaic, int32_t dtype, int64_t n_frames, int64_t height, int64_t width, const int32_t *pattern_host,
                         const float *black_host, const float *gain_host, int32_t method, int32_t output, void *out, void *stream);
int apgpu_bayer_channel_sums(const void *mosaic, int32_t dtype, int64_t height, int64_t width, const int32_t *pattern_host,
                             const float *black_host, const int64_t *rect_host, void *sums, int64_t *counts, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F11 ApContinuumSubtract: narrow-band continuum subtraction L = N' - s C' - b (the reference's stage table lists "Continuum
 *     Subtract" as not yet built, doc/iTelescope_processing.md:8-29, so the arithmetic is this project's own definition, DESIGN
 *     4.3h, restated in tests/continuum_model.py).  No contraction: every multiply and add below rounds on its own.
 *
 *     apgpu_gauss_blur_norm_f32: the normalised, separable blur that matches the sharper image's PSF to the broader one.
 *       data, out [height][width] float32, 4-byte aligned, distinct; taps_host [2 radius + 1] float64 on the HOST (normally
 *       exp(-(k - R)^2 / (2 sigma^2)) normalised to sum 1; any weights are taken as they are); 0 <= radius <=
 *       APGPU_BLUR_MAX_RADIUS (larger: APGPU_EUNSUPPORTED); min_weight >= 0.  valid(y, x) = inside the image and finite.
 *       row pass     a(y, x) = sum_k w[k] double(v(y, x + k - R)), m(y, x) = sum_k w[k], both over the valid taps only, k
 *                    ascending, float64 accumulators that start at +0, the product rounded before the sum.
 *       column pass  A(y, x) = sum_k w[k] a(y + k - R, x), M(y, x) = sum_k w[k] m(y + k - R, x) over the rows inside the image,
 *                    in the same way.
 *       out(y, x) = float32(A / M) (IEEE division, then one rounding to float32) where valid(y, x) and M >= min_weight; NaN
 *       (0x7fc00000) elsewhere: holes keep their footprint and a pixel whose neighbourhood is mostly missing is not
 *       extrapolated.  radius 0 with taps {1} is the identity with that rule (+-inf become NaN).  One launch, no workspace: a
 *       workgroup owns a tile of APGPU_BLUR_TILE_H x APGPU_BLUR_TILE_W pixels and stages it with a halo of `radius` in LDS;
 *       image edges and tile edges take the same path (out-of-image taps are staged as NaN).
 *
 *     apgpu_pair_moments_f64: the six moments of the straight-line fit n = s c + b.  n_img, c_img [n_pixels] float32; mask
 *       [n_pixels] uint8 or NULL (non-zero excludes).  A pixel counts when n and c are finite, mask == 0 and lo <= r <= hi
 *       (inclusive) with r = double(n) - (s double(c) + b), the product, the sum and the difference each rounded; lo = -inf,
 *       hi = +inf keeps every finite unmasked pair.  out6 [6] float64 on the device = count, sum c, sum n, sum c c, sum c n,
 *       sum n n (terms formed in float64).  The count is an exact 64-bit integer, written as a double.  The sums are formed per
 *       lane, per workgroup and over the workgroups in an order that depends on n_pixels alone (no floating-point atomics): the
 *       same input gives the same bits on every run and for every alignment.  s, b, lo, hi must not be NaN.  ws: a workspace of
 *       apgpu_pair_moments_ws_bytes(n_pixels) bytes, 8-byte aligned, owned by the caller; one launch.
 *
 *     apgpu_linear_combine_f32: out = (float32(ca x) + float32(cb y)) + c0, every operation in float32, NaN (0x7fc00000) where x
 *       or y is not finite; y NULL: out = float32(ca x) + c0, NaN where x is not finite.  out may be x or y.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_BLUR_MAX_RADIUS 32
#define APGPU_BLUR_TILE_H 32
#define APGPU_BLUR_TILE_W 64
int apgpu_gauss_blur_norm_f32(const float *data, int64_t height, int64_t width, const double *taps_host, int32_t radius,
                              double min_weight, float *out, void *stream);
size_t apgpu_pair_moments_ws_bytes(int64_t n_pixels);
int apgpu_pair_moments_f64(const float *n_img, const float *c_img, const uint8_t *mask, int64_t n_pixels, double s, double b,
                           double lo, double hi, double *out6, void *ws, size_t ws_bytes, void *stream);
int apgpu_linear_combine_f32(const float *x, const float *y, float ca, float cb, float c0, float *out, int64_t n_pixels, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F12 ApDeconvolve: damped Richardson-Lucy deconvolution of a co-add with its own PSF.  The reference has no such stage, so the
 *     arithmetic is this project's own definition, restated in tests/deconvolve_model.py.
 *
 *     Inputs.  d [height][width] float32; a non-finite value means "no data"; valid(y, x) = inside the image and finite.
 *       p [K][K] float32 on the HOST, K = 2 R + 1, 0 <= R <= APGPU_DECONV_MAX_RADIUS (larger: APGPU_EUNSUPPORTED); every weight
 *       finite and >= 0, the sum > 0; the weights are used as given (the host normalises them).  Sky level b >= 0; gain > 0
 *       (e-/ADU); read noise rn >= 0 (ADU); damping threshold T >= 0; niter >= 0; min_weight >= 0 (0.1 by default in ops).
 *     Rounding and order.  Every operation is float32 and every multiply and add rounds on its own (no contraction, no fmaf).
 *       Accumulators start at +0.  The 2-D tap order is row-major: j (PSF row) ascending outside, i ascending inside.
 *       min(x, 1) means x where x < 1, else 1, and max(x, 0) means x where x > 0, else 0 (a NaN gives the constant).
 *     1 Norm plane (once): n(y, x) = sum_{j,i} p[j][i] W(y + j - R, x + i - R), W = 1 where valid and 0 elsewhere, outside the
 *       image included.  inv(y, x) = 1 / n where n >= min_weight, else 0.
 *     2 Start: u(y, x) = start_level everywhere (a positive float32), or the caller's start plane.
 *     3 Forward + ratio, per iteration: c = (sum_{j,i} p[j][i] u(clampy(y + R - j), clampx(x + R - i))) + b: a true convolution
 *       (the PSF flipped), u edge-replicated outside the image.  At an invalid pixel r = 0.  At a valid pixel with !(c > 0), r = 1.
 *       Otherwise, with T == 0: r = d / c (IEEE division).  Otherwise, with T > 0: e = d - c; var = max(c, 0) / gain + rn rn;
 *       U = min((e e) / ((T T) var), 1); U2 = U U; U4 = U2 U2; U8 = U4 U4; U9 = U8 U; w = U9 (10 - 9 U); r = 1 + (w e) / c.
 *       In both cases r = max(r, 0).  (White's damped RL with the Gaussian form of the likelihood ratio: no log.)
 *     4 Back-projection + update: q = sum_{j,i} p[j][i] r(y + j - R, x + i - R), a correlation; taps outside the image are +0.
 *       u' = (u q) inv where inv != 0, else u' = u.
 *     5 Output: out = u + b at the valid pixels, NaN (0x7fc00000) at the others: holes keep their footprint.
 *
 *     apgpu_deconv_norm_f32 (step 1), apgpu_deconv_ratio_f32 (step 3) and apgpu_deconv_update_f32 (step 4) are the steps alone, one
 *       launch each; all planes [height][width] float32 on the device, 4-byte aligned; the output plane must not be the plane the
 *       taps read (data, u and ratio respectively).
 *     apgpu_richardson_lucy_f32 enqueues 1 + 2 niter launches and nothing else (no allocation, no host synchronisation):
 *       the norm launch also writes the start into the first u plane (or, with niter = 0, the output), u ping-pongs between two
 *       planes, and the last update writes out = u + b / NaN directly.  start_plane NULL: u = start_level (finite, > 0).  ws: a
 *       workspace of apgpu_deconv_ws_bytes(height, width) bytes (the ratio, inv and two u planes, 16 bytes per pixel), 16-byte
 *       aligned, owned by the caller.  out must be neither data nor the start plane.
 *     APGPU_EINVAL: a NULL plane, a negative or non-finite weight, a PSF sum <= 0, sky, gain, read noise or damp out of range, a
 *       workspace that is too small.
 *     A workgroup owns a tile of APGPU_DECONV_TILE_H x APGPU_DECONV_TILE_W outputs and stages it with a halo of R in LDS by the
 *       rule of its pass, so image edges and tile edges take one path (csrc/deconvolve.hip).
 * ------------------------------------------------------------------------------------------- */
#define APGPU_DECONV_MAX_RADIUS 12
#define APGPU_DECONV_TILE_H 32
#define APGPU_DECONV_TILE_W 64
size_t apgpu_deconv_ws_bytes(int64_t height, int64_t width);
int apgpu_deconv_norm_f32(const float *data, int64_t height, int64_t width, const float *psf_host, int32_t radius, float min_weight,
                          float *inv, void *stream);
int apgpu_deconv_ratio_f32(const float *u, const float *data, int64_t height, int64_t width, const float *psf_host, int32_t radius,
                           float sky, float gain, float readnoise, float damp, float *ratio, void *stream);
int apgpu_deconv_update_f32(const float *u, const float *ratio, const float *inv, int64_t height, int64_t width, const float *psf_host,
                            int32_t radius, float *u_out, void *stream);
int apgpu_richardson_lucy_f32(const float *data, int64_t height, int64_t width, const float *psf_host, int32_t radius, float sky, float gain,
                              float readnoise, float damp, int32_t niter, float start_level, const float *start_plane, float min_weight,
                              float *out, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F13 ApMultiscale: noise reduction and detail enhancement by scale with the B3-spline a trous ("starlet") transform.  The
 *     reference has no such stage, so the arithmetic is this project's own definition, restated in
 *     tests/multiscale_model.py.
 *
 *     Input.  d [height][width] float32; a NaN or +-inf pixel is a hole; valid(y, x) = inside the image and finite in the input.
 *       Holes are NaN (0x7fc00000) in every plane and in the output.  1 <= J <= APGPU_STARLET_MAX_SCALES scales.
 *     Taps.  h = {1, 4, 6, 4, 1} / 16 at offsets (k - 2) s, k = 0 .. 4, spacing s = 2^j for step j = 0 .. J - 1.
 *     One step, c_j -> c_{j+1} (c_0 = d): normalised convolution; every multiply and add rounds on its own (no contraction).
 *       Row pass: a(y, x) = sum_k h[k] double(c_j(y, x + (k - 2) s)) and m(y, x) = sum_k h[k], both over the valid taps, k ascending,
 *       float64, accumulators starting at +0.  Column pass: A(y, x) = sum_k h[k] a(y + (k - 2) s, x) and M(y, x) = sum_k h[k] m(y +
 *       (k - 2) s, x) over the rows inside the image, k ascending, float64.  c_{j+1}(y, x) = float32(A / M) where valid(y, x), NaN
 *       elsewhere.  The centre tap of a valid pixel is valid, so M >= 36 / 256: there is no minimum weight.
 *     Planes.  w_{j+1} = c_j - c_{j+1} in float32.
 *     Treatment of plane j with the threshold t_j >= 0 (float32): APGPU_STARLET_HARD T(w) = w where |w| >= t, else +0;
 *       APGPU_STARLET_SOFT T(w) = w - t where w > t, w + t where w < -t, else +0.
 *     Reconstruction, float32: acc_0 = +0, acc_j = acc_{j-1} + g_j T(w_j), out = acc_J + g_res c_J.
 *
 *     The step entry point is one launch: it reads c_in and writes any of c_out = c_{j+1}, w_out = w_{j+1} and acc (NULL: not
 *       wanted).  With APGPU_STARLET_FIRST acc is written as +0 + gain T(w), otherwise read and added to; with APGPU_STARLET_LAST
 *       g_res c_{j+1} is added after that.  All planes [height][width] float32 on the device, 4-byte aligned and distinct.  spacing:
 *       a power of two, 1 .. 32.  form: APGPU_STARLET_FORM_AUTO takes the tile form (a 32 x 64 tile plus a halo of 2 s in LDS) up
 *       to a spacing of APGPU_STARLET_TILE_MAX_AUTO (0: never, as measured) and the direct form (a lane slides along
 *       APGPU_STARLET_CHAIN outputs s rows apart, the row sums in registers) above; the other two values force a form, APGPU_EUNSUPPORTED for the tile form above a
 *       spacing of APGPU_STARLET_TILE_MAX_SPACING.  Both forms give the same bits (csrc/multiscale.hip).
 *     The plane-1 entry point writes w_1 alone, for the noise estimate (8 bytes per pixel).
 *     The planes entry point writes w_1 .. w_J and c_J into planes [scales + 1][height][width], J launches.
 *     The whole-call entry point enqueues J launches and nothing else (no allocation, no host synchronisation): out is the
 *       accumulator, c_j ping-pongs between the two planes of the workspace, c_J is not stored.  12 bytes per pixel for the first
 *       step (8 when it is also the last), 16 for the others, 12 for the last.  thresholds_host, gains_host: float32 [scales].
 *     ws: a workspace of the ws_bytes entry point's size (8 bytes per pixel), 16-byte aligned, owned by the caller; data, out (or
 *       planes) and ws must not overlap.  APGPU_EINVAL: a NULL plane, planes that are not distinct, a threshold that is negative or
 *       not finite, a gain that is not finite, scales, spacing, mode, flags or form out of range.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_STARLET_MAX_SCALES 6
#define APGPU_STARLET_TILE_H 32
#define APGPU_STARLET_TILE_W 64
#define APGPU_STARLET_CHAIN 8
#define APGPU_STARLET_TILE_MAX_SPACING 8   /* the tile form is built for spacings 1, 2, 4, 8 */
#define APGPU_STARLET_TILE_MAX_AUTO 0      /* the measured switch point: the direct form is faster at every spacing */
#define APGPU_STARLET_HARD 0
#define APGPU_STARLET_SOFT 1
#define APGPU_STARLET_FIRST 1
#define APGPU_STARLET_LAST 2
#define APGPU_STARLET_FORM_AUTO 0
#define APGPU_STARLET_FORM_TILE 1
#define APGPU_STARLET_FORM_DIRECT 2
int apgpu_starlet_step_f32(const float *c_in, int64_t height, int64_t width, int32_t spacing, float *c_out, float *w_out, float *acc,
                           float threshold, float gain, float g_res, int32_t mode, int32_t flags, int32_t form, void *stream);
int apgpu_starlet_plane1_f32(const float *data, int64_t height, int64_t width, float *w1, void *stream);
size_t apgpu_starlet_ws_bytes(int64_t height, int64_t width);
int apgpu_starlet_planes_f32(const float *data, int64_t height, int64_t width, int32_t scales, float *planes, void *ws, size_t ws_bytes,
                             void *stream);
int apgpu_multiscale_f32(const float *data, int64_t height, int64_t width, int32_t scales, const float *thresholds_host,
                         const float *gains_host, float g_res, int32_t mode, float *out, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F14 ApDrizzle: variable-pixel linear reconstruction ("drizzle", Fruchter & Hook 2002) of N dithered frames onto a finer grid, and
 *     the blot-and-compare outlier flags in front of it.  The reference has no such stage, so the arithmetic is this project's own
 *     definition, restated in tests/drizzle_model.py and written once in csrc/drizzle_core.h.  Every multiply and add
 *     rounds on its own (no contraction).
 *
 *     Gather form: per output pixel (u = column, v = row, 0-based, integer = pixel centre), over the frames in order.
 *     params [n_frames][10] float64 on the device, per frame: A0 .. A5, hx, hy, w, g.
 *       A maps an OUTPUT pixel to INPUT coordinates, xin = A0 u + A1 v + A2, yin = A3 u + A4 v + A5: the frame's transform composed on
 *       the host, in float64, with the output grid (output pixel (u, v) at reference coordinate ((u + 0.5) / s - 0.5, (v + 0.5) / s -
 *       0.5) for `scale` = s output pixels per reference pixel).  hx = 0.5 hypot(A0, A3), hy = 0.5 hypot(A1, A4): the half-widths of
 *       the "turbo" footprint, the axis-aligned rectangle about (xc, yc) = A(u, v).  The caller keeps lx = 2 hx and ly = 2 hy in
 *       (0, 2]: with pixfrac <= 1 no overlapping pixel then lies outside the window below (a wider footprint is cut to the window;
 *       nothing is read out of bounds).  w: the frame's weight, g: its flux factor (fscale, times |det A| when flux is conserved),
 *       both float32 values, w finite and > 0.
 *     Float64: xc = (A0 u + A1 v) + A2, yc likewise; x0 = xc - hx, x1 = xc + hx; the window origin i0 = ceil(x0 - p/2), j0 likewise.
 *       A frame whose window has no pixel on it (i0 outside -3 .. width - 1 or j0 outside -3 .. height - 1, NaN included) adds nothing.
 *     Float32, in window coordinates: l0 = float(x0 - i0), l1 = float(x1 - i0); the drop of input pixel i0 + t is the square of side
 *       p = pixfrac about it: ox[t] = max(0, min(l1, t + p/2) - max(l0, t - p/2)), t = 0 .. 3, oy likewise; the cover of tap (ti, tj)
 *       is a = (ox[ti] oy[tj]) q with q = float32(1 / (double(p) double(p))).
 *     Taps: rows j0 .. j0 + 3 outer, columns i0 .. i0 + 3 inner.  A tap is skipped when a == 0, the pixel is off the frame, flagged
 *       in mask [height][width] or in frame_masks [n_frames][height][width] (uint8, non-zero = bad, either may be NULL), not finite, or -
 *       with a pattern - of another colour: pattern_host [4] holds the colour (R 0, G1 1, B 2, G2 3) of cell position (j & 1) 2 +
 *       (i & 1) and channel is 0 (R), 1 (G: both greens) or 2 (B); pattern_host NULL: every pixel counts.
 *     Sums, float64 from +0: aw = a w and gv = g value in float32; den += double(aw); num += double(aw) double(gv) (an exact product).
 *     image = float32(num / den), NaN (0x7fc00000) where den == 0; weight = float32(den).  Both [out_height][out_width] float32.
 *     One launch for all frames; a workgroup is APGPU_DRIZZLE_TILE_H rows of APGPU_DRIZZLE_TILE_W output pixels.
 *
 *     Rejection, per pixel (c = column, r = row) of frame i with value v.  params [n_frames][8] float64 on the device, per frame:
 *       B0 .. B5, g, sigma.  B maps an INPUT pixel to the pixel coordinates of ref [ref_height][ref_width] (float32): the inverse of the
 *       frame's transform composed with the reference image's grid, on the host, in float64.  g as above; sigma: the frame's noise
 *       in scaled units (float32 values).
 *     Float64: xr = (B0 c + B1 r) + B2, yr likewise; X = floor(xr), Y = floor(yr).  Float32 from here: fx = float(xr - X), fy likewise;
 *       p00 = ref[Y][X], p01 = ref[Y][X + 1], p10 = ref[Y + 1][X], p11 = ref[Y + 1][X + 1]; top = p00 + fx (p01 - p00), bot = p10 + fx
 *       (p11 - p10), b = top + fy (bot - top); d = max of the four - min of the four.
 *     mask_out[i][r][c] = 1 iff 0 <= X <= ref_width - 2, 0 <= Y <= ref_height - 2, the four and v are finite, and
 *       |g v - b| > k sigma + grow d (strictly); 0 otherwise.  [n_frames][height][width] uint8.
 *     APGPU_EINVAL: a NULL plane, a size below 1, pixfrac outside (0, 1], a pattern that is no permutation of 0 .. 3, channel outside
 *       0 .. 2, image == weight, k or grow negative or not finite.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_DRIZZLE_TILE_H 4
#define APGPU_DRIZZLE_TILE_W 64
int apgpu_drizzle_f32(const float *frames, int32_t n_frames, int64_t height, int64_t width, const uint8_t *mask, const uint8_t *frame_masks,
                      const double *params, float pixfrac, const int32_t *pattern_host, int32_t channel, float *image, float *weight,
                      int64_t out_height, int64_t out_width, void *stream);
int apgpu_drizzle_reject_u8(const float *frames, int32_t n_frames, int64_t height, int64_t width, const double *params, const float *ref,
                            int64_t ref_height, int64_t ref_width, float k, float grow, uint8_t *mask_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F19 Lens distortion: a polynomial map reference pixel -> input pixel per frame, carried through registration, co-add and drizzle
 *     (DESIGN 4.3e'; this project's own definition, written once in csrc/distortion_core.h, on the host in
 *     astrophotography_amd/distortion.py, restated in tests/distortion_model.py).  All float64, every operation rounds on its own.
 *
 *     The map: X = Px(u, v), Y = Py(u, v) with u = (x - x0) / L, v = (y - y0) / L, total degree d in 1 .. APGPU_POLY_MAX_DEGREE.
 *       coef [n_frames][2][ncoef] (x axis, then y axis), ncoef = (d + 1)(d + 2) / 2: coefficient k belongs to u^i v^j, the monomials
 *       running by total degree t = 0 .. d and within t by j = 0 .. t, i = t - j.  One d, x0, y0 and L per call.
 *       Powers by repeated multiplication, up[0] = 1, up[i] = up[i-1] u; the sum from +0 in coefficient order, s = s + c[k] (up[i]
 *       vp[j]).  dX/du likewise from (i c[k]) (up[i-1] vp[j]) over the terms with i >= 1, dX/dv from (j c[k]) (up[i] vp[j-1]) over j >=
 *       1; a derivative with respect to a pixel coordinate is that sum divided by L.
 *
 *     apgpu_nearest_match_poly: apgpu_nearest_match (F8) with T_f the map of frame f in place of the affine; everything else - both
 *       directions, the tie rule, the inclusive radius, the outputs - as there.
 *     apgpu_poly_tile_affines: affines [n_frames][tiles_y][tiles_x][6], tiles of 16 tile_scale rows x 64 tile_scale columns of an
 *       out_height x out_width grid with `scale` = s pixels per reference pixel (tile_scale 1 .. 16): what apgpu_resample_affine_f32
 *       (per_tile), apgpu_resample_oversampled_f32 and ops.drizzle take.  Tile (ty, tx) has its centre at xc = 64 tile_scale tx + (64
 *       tile_scale - 1) / 2, yc = 16 tile_scale ty + (16 tile_scale - 1) / 2, at reference coordinates xr = (xc + 0.5) / s - 0.5, yr
 *       likewise.  With (X, Y) and the derivatives at (xr, yr): a0 = (dX/dx) / s, a1 = (dX/dy) / s, a2 = (X - a0 xc) - a1 yc; a3 =
 *       (dY/dx) / s, a4 = (dY/dy) / s, a5 = (Y - a3 xc) - a4 yc: an affine of OUTPUT pixels (composed != 0).  composed == 0: an
 *       affine of REFERENCE pixels about the same point, a0 = dX/dx, a1 = dX/dy, a2 = (X - a0 xr) - a1 yr and a3 .. a5 likewise (what
 *       ops.drizzle takes and composes with its grid itself).
 *     apgpu_drizzle_tiles_f32: apgpu_drizzle_f32 (F14) with params [n_frames][tiles_y][tiles_x][10], one record per 16 x 64 OUTPUT
 *       pixels, tiles_y = ceil(out_height / 16), tiles_x = ceil(out_width / 64); output pixel (u, v) uses record (v / 16, u / 64).
 *       hx, hy, w and g are the tile's own.
 *     apgpu_drizzle_reject_tiles_u8: apgpu_drizzle_reject_u8 with params [n_frames][tiles_y][tiles_x][8], one record per 16 x 64
 *       INPUT pixels, tiles_y = ceil(height / 16), tiles_x = ceil(width / 64); pixel (c, r) uses record (r / 16, c / 64).
 *     APGPU_EINVAL: as the per-frame entry points, and a degree outside 1 .. 5, an origin or L that is not finite, L <= 0, scale <= 0,
 *       tile_scale outside 1 .. 16.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_POLY_MAX_DEGREE 5
int apgpu_nearest_match_poly(const double *xy, const int32_t *count, const double *coef, int32_t degree, double x0, double y0,
                             double scale_l, int32_t n_frames, int32_t max_stars, double radius, int32_t *fwd_idx, double *fwd_d2,
                             int32_t *bwd_idx, double *bwd_d2, void *stream);
int apgpu_poly_tile_affines(const double *coef, int32_t n_frames, int32_t degree, double x0, double y0, double scale_l, int64_t out_height,
                            int64_t out_width, int32_t tile_scale, double scale, int32_t composed, double *affines, void *stream);
int apgpu_drizzle_tiles_f32(const float *frames, int32_t n_frames, int64_t height, int64_t width, const uint8_t *mask,
                            const uint8_t *frame_masks, const double *params, float pixfrac, const int32_t *pattern_host, int32_t channel,
                            float *image, float *weight, int64_t out_height, int64_t out_width, void *stream);
int apgpu_drizzle_reject_tiles_u8(const float *frames, int32_t n_frames, int64_t height, int64_t width, const double *params,
                                  const float *ref, int64_t ref_height, int64_t ref_width, float k, float grow, uint8_t *mask_out,
                                  void *stream);

/* ---------------------------------------------------------------------------------------------
 * F20 Removal of the large-scale sky gradient of a co-add.  The reference has no such stage: this project's own
 *     definition, restated in tests/gradient_model.py (PARITY UNPINNED).  Host side (ops.fit_surface): the robust fit of a surface
 *     to a few hundred samples.  Device side: the samples, the surface on a lattice, and the pass over the image.  All surface
 *     arithmetic is float64 and every operation rounds on its own.
 *
 *     Coordinates: pixel centre (x, y) = (column, row), 0-based; u = (x - x0) / L, v = (y - y0) / L; for an image of H x W the
 *       callers pass x0 = (W - 1) / 2, y0 = (H - 1) / 2, L = max(W, H) / 2 (the convention of F19).
 *
 *     apgpu_sample_clipped_stats_f32: n_samples <= APGPU_GRADIENT_MAX_SAMPLES square boxes of half-size radius <= APGPU_GRADIENT_
 *       MAX_RADIUS about centres [n_samples][2] (device int32: x, y; a centre may lie anywhere, outside the image too).  Per box
 *       what apgpu_box_clipped_stats_f32 (F4) computes per mesh box - the same kernel, its origin taken from the list: SigmaClip(sigma,
 *       maxiters, median / std) over the pixels that are inside the image, unmasked (mask NULL or mask == 0) and finite;
 *       stats_out [n_samples][4] (device float64) = { median, std, count of the final survivors, pixels of the (2 radius + 1)^2
 *       that were outside, masked or not finite }.  No survivor: NaN, NaN, 0.  n_samples == 0 launches nothing.  Unlike the mesh
 *       entry point, whose std adds in a tree, the std here is np.nanstd of the final survivors with numpy's roundings: the sum from +0
 *       in the box's row-major order, mean = sum / n, the squares of x - mean added in the same order, sqrt(q / n).
 *     apgpu_surface_lattice_f64: the surface at the ny x nx nodes of a lattice of `step` pixels, node (iy, ix) at pixel ((ix - 1)
 *       step, (iy - 1) step); lattice_out [ny][nx] device float64.
 *         APGPU_SURFACE_POLY: n_terms = the degree d in 1 .. APGPU_GRADIENT_MAX_DEGREE; params [(d + 1)(d + 2) / 2] device float64,
 *           coefficient k of u^i v^j in the order of F19 (t = 0 .. d, within t j = 0 .. t, i = t - j); powers by repeated
 *           multiplication; S = the sum from +0 in coefficient order of c[k] (up[i] vp[j]).  centres_uv is not read.
 *         APGPU_SURFACE_TPS: n_terms = K centres (0 .. APGPU_GRADIENT_MAX_SAMPLES); params [3 + K] = a0, a1, a2, w_0 .. w_{K-1};
 *           centres_uv [K][2] = u_k, v_k.  q_k = (u - u_k)^2 + (v - v_k)^2 (the two squares, then their sum), phi(q) = 0 for q == 0,
 *           else (0.5 q) log(q); S = ((A + a0) + a1 u) + a2 v with A the sum from +0 in index order of w_k phi(q_k).  The order is
 *           fixed, so the same input gives the same bits; against another log the result differs by the roundings of K terms.
 *     apgpu_surface_apply_f32: one pass over the image with S(x, y) the cubic-convolution interpolant (Keys, a = -1/2) of the lattice:
 *         ix = x / step (integer), t = double(x - ix step) / double(step), the four nodes ix .. ix + 3 with the weights
 *           w0 = ((-0.5 t + 1) t - 0.5) t, w1 = (1.5 t - 2.5) t t + 1, w2 = ((-1.5 t + 2) t + 0.5) t, w3 = (0.5 t - 0.5) t t;
 *         per lattice row R_a = ((w0 n[a][0] + w1 n[a][1]) + w2 n[a][2]) + w3 n[a][3], then S the same expression of the row weights
 *           and R_0 .. R_3.  ny = (height - 1) / step + 4 and nx likewise (anything else: APGPU_EINVAL): every pixel has its 4 x 4 nodes.
 *         APGPU_GRADIENT_SUBTRACT: out = float32((double(d) - S) + pedestal).
 *         APGPU_GRADIENT_DIVIDE:   out = float32((double(d) / S) pedestal), NaN where S is not finite or S <= 0.
 *         A non-finite d gives NaN in both modes.  surface_out (may be NULL): float32(S) at every pixel.  out may be data;
 *         surface_out must be a plane of its own.  16-byte loads and stores when the planes are 16-byte aligned and width % 4 == 0.
 *     APGPU_EINVAL: NULL or misaligned pointers, a step outside APGPU_GRADIENT_MIN_STEP .. APGPU_GRADIENT_MAX_STEP, more samples or
 *       a larger radius or degree than the limits, sigma < 0 or NaN, an unknown model or mode, a NaN pedestal.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_GRADIENT_MAX_SAMPLES 4096
#define APGPU_GRADIENT_MAX_RADIUS 32
#define APGPU_GRADIENT_MAX_DEGREE 6
#define APGPU_GRADIENT_MIN_STEP 4
#define APGPU_GRADIENT_MAX_STEP 64
#define APGPU_GRADIENT_TILE_H 32
#define APGPU_GRADIENT_TILE_W 128
#define APGPU_SURFACE_POLY 0
#define APGPU_SURFACE_TPS 1
#define APGPU_GRADIENT_SUBTRACT 0
#define APGPU_GRADIENT_DIVIDE 1
int apgpu_sample_clipped_stats_f32(const float *data, const uint8_t *mask, int64_t height, int64_t width, const int32_t *centres,
                                   int32_t n_samples, int32_t radius, double sigma, int32_t maxiters, double *stats_out, void *stream);
int apgpu_surface_lattice_f64(int32_t model, const double *params, const double *centres_uv, int32_t n_terms, double x0, double y0,
                              double half_size, int32_t step, int32_t ny, int32_t nx, double *lattice_out, void *stream);
int apgpu_surface_apply_f32(const float *data, const double *lattice, int64_t height, int64_t width, int32_t ny, int32_t nx,
                            int32_t step, int32_t mode, double pedestal, float *out, float *surface_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F21 Offline plate solving against a catalogue.  The reference sends its source list to astrometry.net; this is the
 *     project's own definition, restated in tests/astrometry_model.py (PARITY UNPINNED).  Device side: the catalogue's projection
 *     about the hint and its search cells.  The triangle votes and neighbour searches are F8's; the fits are host float64.
 *     All arithmetic float64, every operation rounds on its own.
 *
 *     apgpu_sky_project: standard coordinates of n stars (ra, dec: device float64, degrees) about (ra0, dec0), the expressions of
 *       the gnomonic projection in this order, with r = pi / 180 and a = ra r, d = dec r, a0 = ra0 r, d0 = dec0 r:
 *         cosc = sin d0 sin d + (cos d0 cos d) cos(a - a0)
 *         xi   = ((cos d sin(a - a0)) / cosc) / r
 *         eta  = ((cos d0 sin d - (sin d0 cos d) cos(a - a0)) / cosc) / r
 *       xi, eta (device float64 [n], degrees) are NaN where cosc > 0 does not hold (behind the tangent plane, or a non-finite
 *       input); keep (device uint8 [n]) = 1 iff ra and dec are finite, cosc > 0 and cosc >= cos_rc.  keep may be NULL.  One lane
 *       per star; n == 0 launches nothing.
 *     apgpu_cell_select: for each of n_cells closed squares (cells: device float64 [n_cells][3] = centre x, centre y, half side)
 *       the indices of the first `capacity` of the n stars (x, y: device float64 [n], in the caller's order - brightest first) with
 *       |x - cx| <= half and |y - cy| <= half (NaN coordinates are in no cell).  idx [n_cells][capacity] int32: those indices in
 *       ascending order, the unused slots -1; inside [n_cells]: the number of stars in the square when that is <= capacity, else
 *       some value > capacity (the scan stops once the list is full and one more star was seen); count [n_cells] = min(capacity,
 *       inside).  An ordered compaction - a workgroup per cell, wave ballots and prefix counts, no atomics: the same bytes on
 *       every run.  n_cells == 0 launches nothing; n == 0 writes empty lists (x and y are then not read and may be NULL).
 *     APGPU_EINVAL: NULL or misaligned pointers, n or n_cells outside 0 .. 2^31 - 1, capacity outside 1 .. APGPU_CELL_MAX_CAPACITY,
 *       n_cells * capacity >= 2^31, a non-finite (ra0, dec0) or |dec0| > 90, cos_rc outside -1 .. 1.  A cell with a non-finite
 *       member holds no star.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_CELL_MAX_CAPACITY 65536
int apgpu_sky_project(const double *ra, const double *dec, int64_t n, double ra0, double dec0, double cos_rc, double *xi, double *eta,
                      uint8_t *keep, void *stream);
int apgpu_cell_select(const double *x, const double *y, int64_t n, const double *cells, int64_t n_cells, int32_t capacity, int32_t *idx,
                      int32_t *count, int32_t *inside, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F22 Empirical PSF, PSF-fitting photometry and star removal.  The reference has no such stage (photutils is absent);
 *     this is the project's own definition after Anderson & King (2000), restated in tests/epsf_model.py (PARITY UNPINNED).
 *     All arithmetic float64, every operation rounds on its own.
 *
 *     The grid E: device float32 [G][G], G = 2 o R + 1, o = oversampling in 1 .. APGPU_EPSF_MAX_OVERSAMPLING, R = radius in
 *       2 .. APGPU_EPSF_MAX_RADIUS; node (j, i) is the offset ((i - oR) / o, (j - oR) / o) pixels (x = column) from a star's centre.
 *       E(dx, dy) is the separable Keys cubic convolution (a = -0.5) of the grid at u = dx o + oR, v = dy o + oR: with iu = floor(u),
 *       t = u - iu the nodes iu - 1 .. iu + 2 (clamped to 0 .. G - 1) carry the weights w0 .. w3 of apgpu_surface_apply_f32, a row
 *       is ((w0 e0 + w1 e1) + w2 e2) + w3 e3 and the value the same expression of the row weights and the four rows.  It is 0 where
 *       |dx| <= R and |dy| <= R do not both hold.  (csrc/epsf_core.h)
 *     apgpu_epsf_accumulate_f32: stars = device float64 [n][4] (flux f, x, y, sky).  A star takes part if 0 < f < inf, sky is finite
 *       and |x|, |y| <= 1e9.  Pixel p of an axis belongs to node k = floor((p - x) o + 0.5) + oR (at most one pixel per node, axis
 *       and star); the sample of star s at node (j, i) is r = (d - sky) / f - E(px - x, py - y) for that pixel if it lies in the
 *       image and d and r are finite.  Per node: bounds (-inf, inf); a round counts and sums the r inside the closed bounds, ends
 *       the clip if the count is that of the round before, else takes mean = sum / count, std = sqrt(sum (r - mean)^2 / count) and
 *       the new bounds mean -+ sigma std; at most maxiters rounds clip.  mean_out [G][G] float64 (0 where count is 0), count_out
 *       [G][G] int32.  One wavefront per node, lanes stride the stars, butterfly sums: the same bytes on every run.
 *     apgpu_epsf_update_f32: out (j, i) = float32(sum_a sum_b taps[a][b] T(clamp(j + a - 2), clamp(i + b - 2))) in row-major order of
 *       (a, b), T = double(E) + mean where count >= min_count, else double(E).  taps: HOST float64 [5][5].  out must not be grid.
 *     apgpu_epsf_shift_f32: out (j, i) = float32(E((i - oR) / o + dx, (j - oR) / o + dy) scale).  out must not be grid.
 *     apgpu_epsf_fit_f32: init = device float64 [n][4] (f, x, y, sky); damped Gauss-Newton for (f, x, y), and sky with fit_sky, of
 *       f E(px - x, py - y) + sky to the pixels with (px - cx)^2 + (py - cy)^2 <= r_fit^2 about (cx, cy) = rint of the initial
 *       centre, inside the image, with a finite datum.  The datum is the pixel, or with prev (device float64 [n][3] = f0, x0, y0; may
 *       be NULL) pixel + f0 E(px - x0, py - y0): `image` is then a residual image.  Weights 1, or with gain > 0
 *       1 / (readnoise^2 + max(model, 0) / gain), the model being that of the point a step starts from.  It stops when a step has |dx|, |dy| < 1e-7 and |df| <= 1e-9 |f|, or after max_iter
 *       iterations.  rec_out: float64 [n][APGPU_EPSF_REC] = f, x, y, sky, chi^2, pixels used, iterations, ok; a star with fewer than
 *       6 usable pixels, a non-finite input, a system that is not positive definite or a non-finite result has ok = 0, chi^2 = NaN
 *       and its input values.  One wavefront per star.
 *     apgpu_epsf_render_f32: stars = device float64 [n][3] (f, x, y); tile_offsets int32 [tiles + 1], tile_stars int32 [n_entries]: the
 *       stars of every APGPU_EPSF_TILE-pixel square tile (row-major tiles, ceil(width / TILE) per row) in CSR form.  Per pixel the
 *       sum of f E(px - x, py - y) over its tile's list in list order (entries outside 0 .. n - 1 and stars with a non-finite flux
 *       are skipped); model_out = float32(sum), residual_out = float32(double(image) - sum); either may be NULL, image too if
 *       residual_out is.  model_out and residual_out must be planes of their own (neither the other nor image).
 *     APGPU_EINVAL: NULL or misaligned pointers, oversampling, radius or r_fit (1 .. APGPU_EPSF_MAX_RADIUS) out of range, negative
 *       counts, sigma <= 0, maxiters < 0, max_iter < 1, a non-finite tap, offset or scale, a negative gain or read noise.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_EPSF_MAX_OVERSAMPLING 4
#define APGPU_EPSF_MAX_RADIUS 32
#define APGPU_EPSF_REC 8
#define APGPU_EPSF_TILE 32
int apgpu_epsf_accumulate_f32(const float *image, int64_t height, int64_t width, const double *stars, int32_t n_stars,
                              const float *grid, int32_t oversampling, int32_t radius, double sigma, int32_t maxiters,
                              double *mean_out, int32_t *count_out, void *stream);
int apgpu_epsf_update_f32(const float *grid, const double *mean, const int32_t *count, int32_t oversampling, int32_t radius,
                          int32_t min_count, const double *taps, float *out, void *stream);
int apgpu_epsf_shift_f32(const float *grid, int32_t oversampling, int32_t radius, double dx, double dy, double scale, float *out,
                         void *stream);
int apgpu_epsf_fit_f32(const float *image, int64_t height, int64_t width, const double *init, const double *prev, int32_t n_stars,
                       const float *grid, int32_t oversampling, int32_t radius, double r_fit, int32_t fit_sky, double gain,
                       double readnoise, int32_t max_iter, double *rec_out, void *stream);
int apgpu_epsf_render_f32(const float *image, int64_t height, int64_t width, const double *stars, int32_t n_stars,
                          const int32_t *tile_offsets, const int32_t *tile_stars, int32_t n_entries, const float *grid,
                          int32_t oversampling, int32_t radius, float *model_out, float *residual_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * F23 Optimal image subtraction: the kernel fit of Alard & Lupton (1998) with the spatial variation of Alard (2000).
 *     The reference has no such stage; this is the project's own definition, restated in tests/subtract_model.py (PARITY UNPINNED).
 *     Every operation rounds on its own, no contraction.  x = column, y = row; (T (x) K)(x, y) = sum_{u, v} K(u, v) T(x - u, y - v),
 *     a kernel of radius r is stored [2 r + 1][2 r + 1] with K(u, v) at [v + r][u + r].
 *
 *     apgpu_subtract_basis_f64 (host only, no device work): the basis of n_gauss Gaussians (sigmas_host > 0) times polynomials of
 *       the degrees degrees_host in its separable form (csrc/subtract_core.h).  Functions are ordered g, then i, then j ascending
 *       (i + j <= degree g); the 1-D filters g, then power p ascending: filters[f][u + r] = exp(-u^2 / (2 sigma_g^2)) u^p (u^p by
 *       repeated multiplication).  Function n = (g, i, j): b_n(u, v) = filters[row[n]][u + r] filters[col[n]][v + r], row[n] the filter
 *       of (g, i), col[n] that of (g, j); even[n] = 1 where i and j are both even, and then scale[n] = 1 / sum b_n (over v ascending of
 *       the sums over u ascending), else 1.  B_n = scale[n] b_n, minus B_0 where even[n] and n > 0: every function but the first sums
 *       to 0.  The output arrays hold APGPU_SUBTRACT_MAX_BASIS entries (filters: APGPU_SUBTRACT_MAX_BASIS rows of 2 r + 1).
 *       APGPU_EUNSUPPORTED: radius above APGPU_SUBTRACT_MAX_RADIUS, more than APGPU_SUBTRACT_MAX_BASIS functions.
 *     apgpu_subtract_stamps_f32: per stamp s of half-size `half` (n = 2 half + 1 pixels a side) about the integer pixel centers[s] =
 *       (x, y) (device int32 [S][2]), in float64 with every accumulator starting at +0:
 *         R_f(x, y') = sum_u filters[f][u + r] T(x - u, y'), u ascending;  c_n(x, y) = sum_v filters[col[n]][v + r] R_row[n](x, y - v),
 *         v ascending;  V_n = scale[n] c_n, minus V_0 where even[n] and n > 0 (= T (x) B_n);  V_Nb = 1;  V_Nb+1 = I;
 *         gram_out[s][a][b] = gram_out[s][b][a] = sum over the stamp's pixels in row-major order of (w V_a) V_b for a <= b
 *       (float64 [S][Nb + 2][Nb + 2]: the Gram matrix of the Nb + 1 fit vectors, their products with I, and sum w I^2), w = 1 or, with
 *       gain > 0 (then readnoise > 0), 1 / (readnoise^2 / gain^2 + max(I, 0) / gain).  filters: DEVICE float64 [n_filters][2 r + 1]; row,
 *       col, scale, even: HOST arrays of n_basis entries.  status_out[s] (int32): 0, or the bits 1 (the footprint half + r leaves the
 *       image; the other bits are then not looked for), 2 (a non-finite template pixel in the footprint), 4 (a non-finite image
 *       pixel in the stamp), 8 (a non-zero mask pixel in the stamp; mask uint8 [H][W], may be NULL); count_out[s] = n^2 or, with a
 *       status, 0 and a gram of zeros.  One workgroup per stamp, no atomics: the same bytes on every run.
 *     apgpu_subtract_apply_f32: kernels = device float32 [nt][2 r + 1][2 r + 1], nt = (kernel_degree + 1)(kernel_degree + 2) / 2 composite
 *       kernels A_t, one per spatial term phi_t = X^i Y^j (i + j <= degree, i then j ascending; X = (2 x - (W - 1)) / max(W - 1, 1),
 *       Y likewise, powers by repeated multiplication, in float64).  S = `convolved` with non-finite and out-of-image pixels as NaN,
 *       O = `other`.  In float32: conv_t = sum_u sum_v A_t(u, v) S(x - u, y - v), u ascending outside, v ascending inside, from +0;
 *       conv = sum_t float32(phi_t) conv_t, t ascending from +0; B = float32(sum_t bg_host[t] phi_t) (float64, t ascending from +0, the
 *       terms of bg_degree); matched_out (may be NULL) = conv + B; diff_out = (O - conv) - B, or with APGPU_SUBTRACT_CONVOLVED_IMAGE
 *       ((conv + B) - O) / a0 (`convolved` is then the image, `other` the template; a0 finite, not 0); diff_out = NaN where O is not
 *       finite (and, by propagation, where a pixel of the footprint of S is NaN); every NaN written is the quiet NaN 0x7fc00000.
 *       The outputs are planes of their own.
 *     APGPU_EINVAL: NULL or misaligned pointers, shapes <= 0, a radius or half-size below 1, degrees outside 0 .. 3, filter indices
 *       out of range, a non-finite scale, coefficient or a0, gain or readnoise negative, unknown flags.
 * ------------------------------------------------------------------------------------------- */
#define APGPU_SUBTRACT_MAX_RADIUS 15
#define APGPU_SUBTRACT_MAX_BASIS 64
#define APGPU_SUBTRACT_MAX_DEGREE 3
#define APGPU_SUBTRACT_MAX_HALF 15
#define APGPU_SUBTRACT_TILE_H 32
#define APGPU_SUBTRACT_TILE_W 64
#define APGPU_SUBTRACT_CONVOLVED_IMAGE 1
int apgpu_subtract_basis_f64(const double *sigmas_host, const int32_t *degrees_host, int32_t n_gauss, int32_t radius, double *filters_host,
                             int32_t *row_host, int32_t *col_host, double *scale_host, int32_t *even_host, int32_t *n_filters_host,
                             int32_t *n_basis_host);
int apgpu_subtract_stamps_f32(const float *tmpl, const float *image, const uint8_t *mask, int64_t height, int64_t width,
                              const int32_t *centers, int32_t n_stamps, int32_t half, int32_t radius, const double *filters,
                              int32_t n_filters, const int32_t *row_host, const int32_t *col_host, const double *scale_host,
                              const int32_t *even_host, int32_t n_basis, double gain, double readnoise, double *gram_out,
                              int32_t *status_out, int32_t *count_out, void *stream);
int apgpu_subtract_apply_f32(const float *convolved, const float *other, int64_t height, int64_t width, const float *kernels,
                             int32_t radius, int32_t kernel_degree, const double *bg_host, int32_t bg_degree, int32_t flags, float a0,
                             float *diff_out, float *matched_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* APGPU_H */
