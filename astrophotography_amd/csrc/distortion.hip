// distortion.hip - F19: the per-tile affines of a polynomial distortion map (include/apgpu.h F19, DESIGN 4.3e'; the arithmetic is
// distortion_core.h, restated in tests/distortion_model.py).  The resample and drizzle kernels take one 2x3 transform per output tile;
// this kernel writes them on the device, a thread per (frame, tile): 64 frames of 4096 x 4096 are a million records that never
// touch the host.  All float64, no contraction.
#include "common.h"
#include "distortion_core.h"

namespace apgpu {
namespace {

constexpr int kTileBlock = 256;

// Thread t of block (bx, f): tile t = bx * kTileBlock + threadIdx.x of frame f, row-major over [tiles_y][tiles_x].  The frame's
// coefficients sit at a wave-uniform address.
template <int D>
__global__ __launch_bounds__(kTileBlock) void poly_tile_affines_kernel(const double *__restrict__ coef, PolyFrame fr, int tiles_y, int tiles_x,
                                                                       int tile_h, int tile_w, double s, int composed, double *__restrict__ out)
{
    const int f = blockIdx.y;
    const long long t = (long long)blockIdx.x * kTileBlock + threadIdx.x;
    if (t >= (long long)tiles_y * tiles_x) return;
    const int ty = (int)(t / tiles_x), tx = (int)(t % tiles_x);
    const double xc = (double)((long long)tile_w * tx) + ((double)tile_w - 1.0) / 2.0;
    const double yc = (double)((long long)tile_h * ty) + ((double)tile_h - 1.0) / 2.0;
    double A[6];
    poly_tile_affine<D>(coef + (size_t)f * 2 * poly_ncoef(D), fr, xc, yc, s, composed != 0, A);
    double *o = out + ((size_t)f * (size_t)tiles_y * (size_t)tiles_x + (size_t)t) * 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) o[i] = A[i];
}

template <int D>
void launch_tiles(dim3 grid, hipStream_t st, const double *coef, PolyFrame fr, int tiles_y, int tiles_x, int tile_h, int tile_w, double s,
                  int composed, double *out)
{
    hipLaunchKernelGGL(poly_tile_affines_kernel<D>, grid, dim3(kTileBlock), 0, st, coef, fr, tiles_y, tiles_x, tile_h, tile_w, s, composed, out);
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_poly_tile_affines(const double *coef, int32_t n_frames, int32_t degree, double x0, double y0, double scale_l,
                                       int64_t out_height, int64_t out_width, int32_t tile_scale, double scale, int32_t composed, double *affines, void *stream)
{
    if (!coef || !affines) return fail(APGPU_EINVAL, "poly_tile_affines: NULL pointer argument");
    if (n_frames < 1 || n_frames > 65535) return fail(APGPU_EINVAL, "poly_tile_affines: %d frames (1 .. 65535)", n_frames);
    if (degree < 1 || degree > kPolyMaxDegree) return fail(APGPU_EINVAL, "poly_tile_affines: degree %d is outside 1 .. %d", degree, kPolyMaxDegree);
    if (!(is_finite(x0) && is_finite(y0) && is_finite(scale_l) && scale_l > 0.0))
        return fail(APGPU_EINVAL, "poly_tile_affines: origin (%g, %g) must be finite and L = %g finite and positive", x0, y0, scale_l);
    if (!(is_finite(scale) && scale > 0.0)) return fail(APGPU_EINVAL, "poly_tile_affines: scale %g is not a positive number", scale);
    if (out_height < 1 || out_width < 1 || tile_scale < 1 || tile_scale > 16)
        return fail(APGPU_EINVAL, "poly_tile_affines: output %lld x %lld, tile_scale %d (1 .. 16)", (long long)out_height, (long long)out_width,
                    tile_scale);
    const long long th = 16LL * tile_scale, tw = 64LL * tile_scale;
    const long long ty = (out_height + th - 1) / th, tx = (out_width + tw - 1) / tw;
    if (ty > 0x7fffffffLL || tx > 0x7fffffffLL || ty * tx > 0x7fffffffLL)
        return fail(APGPU_EUNSUPPORTED, "poly_tile_affines: %lld x %lld tiles", ty, tx);
    const dim3 grid((unsigned)((ty * tx + kTileBlock - 1) / kTileBlock), (unsigned)n_frames);
    const PolyFrame fr{x0, y0, scale_l};
    hipStream_t st = as_stream(stream);
    switch (degree) {
    case 1: launch_tiles<1>(grid, st, coef, fr, (int)ty, (int)tx, (int)th, (int)tw, scale, (int)(composed != 0), affines); break;
    case 2: launch_tiles<2>(grid, st, coef, fr, (int)ty, (int)tx, (int)th, (int)tw, scale, (int)(composed != 0), affines); break;
    case 3: launch_tiles<3>(grid, st, coef, fr, (int)ty, (int)tx, (int)th, (int)tw, scale, (int)(composed != 0), affines); break;
    case 4: launch_tiles<4>(grid, st, coef, fr, (int)ty, (int)tx, (int)th, (int)tw, scale, (int)(composed != 0), affines); break;
    default: launch_tiles<5>(grid, st, coef, fr, (int)ty, (int)tx, (int)th, (int)tw, scale, (int)(composed != 0), affines); break;
    }
    return check_launch("poly_tile_affines");
}
