// plane_tile.h - what the tiled plane filters with "inside the image and finite" validity share (continuum.hip's blur, multiscale.hip's
// tile form): the staging of a tile and its halo in LDS, and the validity-weighted accumulate of their row passes.
#pragma once
#include <hip/hip_runtime.h>

#include "np_exact.h"

namespace apgpu {

// The LDS row pitch of a tile of tile_w columns with a halo of up to r: up to 3 columns of slack left of the halo, as the staged
// origin is a multiple of 4.
constexpr int halo_pitch(int tile_w, int r) { return tile_w + 2 * r + 4; }

// Stages image rows ty0 - R .. ty0 - R + rows - 1 and the columns tx0 - R .. tx0 + tile_w + R - 1 as float32, pixels outside the
// image as NaN (so "inside and finite" is one test), by a workgroup of BLOCK lanes.  The origin is rounded down to a multiple of
// four columns so that 16-byte loads serve when `wide` (the plane 16-byte aligned and W a multiple of 4: a group of four then lies
// inside the image or outside it).  Returns off = 0 .. 3: tile[r][off + j] is image column tx0 - R + j.  No barrier.
template <int PITCH, int BLOCK>
__device__ __forceinline__ int stage_halo(float (*tile)[PITCH], const float *__restrict__ data, long long H, long long W, long long tx0,
                                          long long ty0, int tile_w, int R, int rows, int wide)
{
    const long long gx0 = ((tx0 - R) >> 2) << 2;            // floor to a multiple of 4 (arithmetic shift: negative values too)
    const int off = (int)(tx0 - R - gx0);
    const int cols = (off + tile_w + 2 * R + 3) & ~3;       // staged columns, a multiple of 4 (<= PITCH)
    const float nanv = quiet_nan();
    const int groups = cols >> 2;
    for (int idx = threadIdx.x; idx < rows * groups; idx += BLOCK) {
        const int lr = idx / groups, g = idx - lr * groups;
        const long long gy = ty0 - R + lr, gx = gx0 + 4 * g;
        float4 v = make_float4(nanv, nanv, nanv, nanv);
        if (gy >= 0 && gy < H) {
            const float *row = data + (size_t)gy * (size_t)W;
            if (wide) {
                if (gx >= 0 && gx < W) v = *reinterpret_cast<const float4 *>(row + gx);
            } else {
                if (gx >= 0 && gx < W) v.x = row[gx];
                if (gx + 1 >= 0 && gx + 1 < W) v.y = row[gx + 1];
                if (gx + 2 >= 0 && gx + 2 < W) v.z = row[gx + 2];
                if (gx + 3 >= 0 && gx + 3 < W) v.w = row[gx + 3];
            }
        }
        *reinterpret_cast<float4 *>(&tile[lr][4 * g]) = v;
    }
    return off;
}

// One tap of a row pass: the value and its weight count where the value is finite.
__device__ __forceinline__ void row_add(double &a, double &m, float v, double w)
{
    const bool ok = is_finite(v);
    const double t = w * (double)v;
    a = ok ? a + t : a;
    m = ok ? m + w : m;
}

}  // namespace apgpu
