// drizzle.hip - F14: variable-pixel linear reconstruction ("drizzle", Fruchter & Hook 2002) of N dithered frames onto a finer grid,
// gather form with the axis-aligned "turbo" footprint, and the blot-and-compare outlier flags that go in front of it.
//
// The reference has no such stage, so the arithmetic is this project's own definition (include/apgpu.h F14), restated in
// tests/drizzle_model.py; it is written once, for one pixel, in drizzle_core.h.  No contraction anywhere.
//
//   drizzle  a lane owns one output pixel (u, v) and walks the N frames in order with (num, den) in float64 registers: no atomics,
//            one launch, the sums in a fixed order.  A workgroup is kTileH rows of kTileW pixels, a wavefront per row, so the stores
//            are whole 256-byte rows.  The ten parameters of a frame are read at a wave-uniform address (scalar loads into SGPRs).
//            The input window is read through L1: at scale s a wavefront's 64 pixels fall on about 64 / s consecutive input pixels
//            per tap, one or two cache lines, and the rows and the halo a neighbouring workgroup reads again come from L2.  The
//            window is 4 x 4 by definition; only the ceil(l + p) + 1 taps per axis that can overlap are visited (2 x 2 at s = 2,
//            p = 0.5), a wave-uniform count, the others having a == 0.
//   reject   elementwise over [N][H][W], a lane per input pixel, four gathered reads of the reference image.
// Every offset is 64-bit: N H W and the output may pass 2^31 elements.
#include "common.h"
#include "drizzle_core.h"

namespace apgpu {
namespace {

constexpr int kTileW = APGPU_DRIZZLE_TILE_W, kTileH = APGPU_DRIZZLE_TILE_H;
static_assert(kTileW == kWave, "a wavefront owns one tile row");

// kTiles: params is [N][tiles_y][tiles_x][10], one record per kParamTileH x kTileW OUTPUT pixels (apgpu_drizzle_tiles_f32).  A workgroup
// lies inside one such tile, so the record's address is built from blockIdx alone and stays wave-uniform.
constexpr int kParamTileH = 16;
static_assert(kParamTileH % kTileH == 0, "a workgroup lies inside one parameter tile");

template <bool kTiles>
__global__ __launch_bounds__(kTileW *kTileH) void drizzle_kernel(const DrizzleImage im, int n_frames, const double *__restrict__ params,
                                                                  int tiles_y, int tiles_x, float *__restrict__ image,
                                                                  float *__restrict__ weight, long long h, long long w)
{
    const long long u = (long long)blockIdx.x * kTileW + threadIdx.x;
    const long long v = (long long)blockIdx.y * kTileH + threadIdx.y;
    if (u >= w || v >= h) return;
    const double ud = (double)u, vd = (double)v;
    double num = 0.0, den = 0.0;
    if (kTiles) {
        const size_t tile = (size_t)(blockIdx.y / (kParamTileH / kTileH)) * (size_t)tiles_x + blockIdx.x, per_frame = (size_t)tiles_y * (size_t)tiles_x;
        for (int f = 0; f < n_frames; f++)
            drizzle_frame(im, f, params + ((size_t)f * per_frame + tile) * kDrizzleFrameDoubles, ud, vd, num, den);
    } else {
        for (int f = 0; f < n_frames; f++) drizzle_frame(im, f, params + (size_t)f * kDrizzleFrameDoubles, ud, vd, num, den);
    }
    const size_t idx = (size_t)v * (size_t)w + (size_t)u;
    float iv, wv;
    drizzle_finish(num, den, iv, wv);
    image[idx] = iv;
    weight[idx] = wv;
}

constexpr int kRejectBlock = 256;

// kTiles: params is [N][tiles_y][tiles_x][8], one record per kParamTileH x kTileW INPUT pixels (apgpu_drizzle_reject_tiles_u8).  A
// wavefront's 64 pixels lie in one tile (the block starts at a multiple of 256 columns); the tile column is taken from the first
// active lane so that the record is read by scalar loads.
template <bool kTiles>
__global__ __launch_bounds__(kRejectBlock) void drizzle_reject_kernel(const float *__restrict__ frames, long long H, long long W,
                                                                       const double *__restrict__ params, int tiles_y, int tiles_x,
                                                                       const float *__restrict__ ref, long long hr, long long wr, float k,
                                                                       float grow, uint8_t *__restrict__ mask_out)
{
    const long long c = (long long)blockIdx.x * kRejectBlock + threadIdx.x;
    const long long r = blockIdx.y;
    const long long f = blockIdx.z;
    if (c >= W) return;
    const size_t idx = ((size_t)f * (size_t)H + (size_t)r) * (size_t)W + (size_t)c;
    size_t rec = (size_t)f;
    if (kTiles) {
        const int tx = __builtin_amdgcn_readfirstlane((int)(c / kTileW));
        rec = ((size_t)f * (size_t)tiles_y + (size_t)(r / kParamTileH)) * (size_t)tiles_x + (size_t)tx;
    }
    mask_out[idx] = drizzle_reject_pixel(ref, hr, wr, params + rec * kRejectFrameDoubles, (double)c, (double)r, frames[idx], k, grow);
}

// The entry points' shared halves.  kTiles: the per-tile records of the *_tiles_* entry points; the tile counts follow from the shapes.
template <bool kTiles>
int drizzle_launch(const char *what, const float *frames, int32_t n_frames, int64_t height, int64_t width, const uint8_t *mask,
                   const uint8_t *frame_masks, const double *params, float pixfrac, const int32_t *pattern_host, int32_t channel, float *image,
                   float *weight, int64_t out_height, int64_t out_width, void *stream)
{
    if (!frames || !params || !image || !weight) return fail(APGPU_EINVAL, "%s: NULL frames, params, image or weight", what);
    if (n_frames < 1 || height < 1 || width < 1 || out_height < 1 || out_width < 1)
        return fail(APGPU_EINVAL, "%s: n_frames %d, input %lld x %lld, output %lld x %lld", what, n_frames, (long long)height,
                    (long long)width, (long long)out_height, (long long)out_width);
    if (!(pixfrac > 0.0f && pixfrac <= 1.0f)) return fail(APGPU_EINVAL, "%s: pixfrac %g is not in (0, 1]", what, (double)pixfrac);
    if (image == weight) return fail(APGPU_EINVAL, "%s: image and weight are one plane", what);
    unsigned cfa = 0xfu;
    if (pattern_host) {
        if (channel < 0 || channel > 2) return fail(APGPU_EINVAL, "%s: channel %d is not 0 (R), 1 (G) or 2 (B)", what, channel);
        unsigned seen = 0;
        cfa = 0;
        for (int p = 0; p < 4; p++) {
            const int32_t col = pattern_host[p];
            if (col < 0 || col > 3) return fail(APGPU_EINVAL, "%s: pattern[%d] = %d is not a colour index 0 .. 3", what, p, col);
            seen |= 1u << col;
            if ((col == 3 ? 1 : col) == channel) cfa |= 1u << p;
        }
        if (seen != 0xfu) return fail(APGPU_EINVAL, "%s: the pattern is not a permutation of 0 .. 3", what);
    }
    dim3 grid;
    if (int rc = tile_grid(what, out_height, out_width, kTileH, kTileW, &grid)) return rc;
    DrizzleImage im;
    im.frames = frames;
    im.mask = mask;
    im.frame_masks = frame_masks;
    im.H = height;
    im.W = width;
    im.hp = 0.5f * pixfrac;
    im.q = (float)(1.0 / ((double)pixfrac * (double)pixfrac));
    im.cfa = cfa;
    const int tiles_y = (int)((out_height + kParamTileH - 1) / kParamTileH), tiles_x = (int)grid.x;
    hipLaunchKernelGGL(drizzle_kernel<kTiles>, grid, dim3(kTileW, kTileH), 0, as_stream(stream), im, n_frames, params, tiles_y, tiles_x, image,
                       weight, (long long)out_height, (long long)out_width);
    return check_launch("drizzle_kernel");
}

template <bool kTiles>
int drizzle_reject_launch(const char *what, const float *frames, int32_t n_frames, int64_t height, int64_t width, const double *params,
                          const float *ref, int64_t ref_height, int64_t ref_width, float k, float grow, uint8_t *mask_out, void *stream)
{
    if (!frames || !params || !ref || !mask_out) return fail(APGPU_EINVAL, "%s: NULL frames, params, ref or mask_out", what);
    if (n_frames < 1 || height < 1 || width < 1 || ref_height < 1 || ref_width < 1)
        return fail(APGPU_EINVAL, "%s: n_frames %d, input %lld x %lld, reference %lld x %lld", what, n_frames, (long long)height,
                    (long long)width, (long long)ref_height, (long long)ref_width);
    if (!(k >= 0.0f) || !(grow >= 0.0f) || !is_finite(k) || !is_finite(grow))
        return fail(APGPU_EINVAL, "%s: k %g and grow %g must be finite and >= 0", what, (double)k, (double)grow);
    if (height > 65535 || n_frames > 65535) return fail(APGPU_EUNSUPPORTED, "%s: more than 65535 rows or frames", what);
    const long long gx = (width + kRejectBlock - 1) / kRejectBlock;
    if (gx > 0x7fffffffLL) return fail(APGPU_EUNSUPPORTED, "%s: rows of %lld pixels", what, (long long)width);
    const int tiles_y = (int)((height + kParamTileH - 1) / kParamTileH), tiles_x = (int)((width + kTileW - 1) / kTileW);
    hipLaunchKernelGGL(drizzle_reject_kernel<kTiles>, dim3((unsigned)gx, (unsigned)height, (unsigned)n_frames), dim3(kRejectBlock), 0,
                       as_stream(stream), frames, (long long)height, (long long)width, params, tiles_y, tiles_x, ref, (long long)ref_height,
                       (long long)ref_width, k, grow, mask_out);
    return check_launch("drizzle_reject_kernel");
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_drizzle_f32(const float *frames, int32_t n_frames, int64_t height, int64_t width, const uint8_t *mask,
                                 const uint8_t *frame_masks, const double *params, float pixfrac, const int32_t *pattern_host, int32_t channel,
                                 float *image, float *weight, int64_t out_height, int64_t out_width, void *stream)
{
    return drizzle_launch<false>("apgpu_drizzle_f32", frames, n_frames, height, width, mask, frame_masks, params, pixfrac, pattern_host, channel,
                                 image, weight, out_height, out_width, stream);
}

extern "C" int apgpu_drizzle_reject_u8(const float *frames, int32_t n_frames, int64_t height, int64_t width, const double *params,
                                       const float *ref, int64_t ref_height, int64_t ref_width, float k, float grow, uint8_t *mask_out,
                                       void *stream)
{
    return drizzle_reject_launch<false>("apgpu_drizzle_reject_u8", frames, n_frames, height, width, params, ref, ref_height, ref_width, k, grow,
                                        mask_out, stream);
}

extern "C" int apgpu_drizzle_tiles_f32(const float *frames, int32_t n_frames, int64_t height, int64_t width, const uint8_t *mask,
                                       const uint8_t *frame_masks, const double *params, float pixfrac, const int32_t *pattern_host,
                                       int32_t channel, float *image, float *weight, int64_t out_height, int64_t out_width, void *stream)
{
    return drizzle_launch<true>("apgpu_drizzle_tiles_f32", frames, n_frames, height, width, mask, frame_masks, params, pixfrac, pattern_host,
                                channel, image, weight, out_height, out_width, stream);
}

extern "C" int apgpu_drizzle_reject_tiles_u8(const float *frames, int32_t n_frames, int64_t height, int64_t width, const double *params,
                                             const float *ref, int64_t ref_height, int64_t ref_width, float k, float grow, uint8_t *mask_out,
                                             void *stream)
{
    return drizzle_reject_launch<true>("apgpu_drizzle_reject_tiles_u8", frames, n_frames, height, width, params, ref, ref_height, ref_width, k,
                                       grow, mask_out, stream);
}
