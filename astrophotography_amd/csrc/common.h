// Shared helpers for the libapgpu.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "apgpu.h"

namespace apgpu {

// Thread-local message behind apgpu_last_error().
char *err_buf();
int fail(int code, const char *fmt, ...);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Call after every kernel launch: turns a launch failure into APGPU_ELAUNCH.
int check_launch(const char *what);

constexpr int kWave = 64;       // gfx950 wavefront
constexpr int kNumCU = 256;     // MI355X

// ---- what the entry points of the plane filters check before they launch ----------------------------------------------------
inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// 16-byte loads and stores serve every row of these planes of width W (a NULL plane, one that is not passed, does not count).
template <typename... P>
inline bool wide_rows(long long W, const P *...planes)
{
    return (W & 3) == 0 && (aligned(planes, 16) && ...);
}

// A float32 image argument: not NULL, a positive shape, 4-byte aligned.
inline int check_plane(const char *what, const float *data, int64_t height, int64_t width)
{
    if (!data) return fail(APGPU_EINVAL, "%s: NULL pointer argument", what);
    if (height <= 0 || width <= 0) return fail(APGPU_EINVAL, "%s: image of %lld x %lld", what, (long long)height, (long long)width);
    if (!aligned(data, 4)) return fail(APGPU_EINVAL, "%s: the planes must be 4-byte aligned", what);
    return APGPU_OK;
}

// The launch grid of nx x ny workgroups over an image, or APGPU_EUNSUPPORTED past the limits of gridDim.x and gridDim.y.
inline int launch_grid(const char *what, int64_t height, int64_t width, long long nx, long long ny, dim3 *grid)
{
    if (nx > 0x7fffffffLL || ny > 65535)
        return fail(APGPU_EUNSUPPORTED, "%s: image of %lld x %lld is too large", what, (long long)height, (long long)width);
    *grid = dim3((unsigned)nx, (unsigned)ny);
    return APGPU_OK;
}

// ... of one workgroup per tile of tile_h x tile_w pixels.
inline int tile_grid(const char *what, int64_t height, int64_t width, int tile_h, int tile_w, dim3 *grid)
{
    return launch_grid(what, height, width, (width + tile_w - 1) / tile_w, (height + tile_h - 1) / tile_h, grid);
}

}  // namespace apgpu
