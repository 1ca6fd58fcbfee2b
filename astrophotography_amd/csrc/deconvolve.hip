// deconvolve.hip - F12: damped Richardson-Lucy deconvolution on gfx950: the norm plane, the forward convolution with the ratio, the
// back-projection with the multiplicative update.
//
// The reference has no such stage, so the arithmetic is this project's own definition (include/apgpu.h F12), restated
// in tests/deconvolve_model.py.  Every operation is float32 and rounds on its own (no contraction, no fmaf); accumulators start at
// +0; the 2-D tap order is row-major, j (PSF row) ascending outside and i ascending inside.
//
//   norm     n(y, x) = sum_{j,i} p[j][i] W(y + j - R, x + i - R), W = 1 where the pixel is inside and finite, else 0
//            inv = 1 / n where n >= min_weight, else 0
//   forward  c = (sum_{j,i} p[j][i] u(clampy(y + R - j), clampx(x + R - i))) + sky, then the ratio r (see ratio1)
//   update   q = sum_{j,i} p[j][i] r(y + j - R, x + i - R), taps outside the image +0;  u' = (u q) inv where inv != 0, else u
//
// One geometry serves the three: a workgroup of 256 lanes owns a tile of kTileH = 32 rows x kTileW = 64 columns and stages it with
// a halo of R in LDS as float32, applying the rule of its pass while it stages (edge replication forward, +0 backward, the 0 / 1
// validity plane for the norm), so that image edges and tile edges take one path.  A lane owns a horizontal run of kRun = 8
// outputs.  Per PSF row it reads the 8 + 2 R floats under its run into registers (ds_read_b128; the run starts on a 32-byte
// boundary of the LDS row) and walks i ascending over its eight accumulators: (8 + 2 R) / (8 K) LDS reads per tap.  The loop over
// the PSF rows is kept rolled and the weights of a row come through scalar loads from the kernel arguments (they are the same in
// every lane), so the body is K x 8 multiplies and as many adds.  The kernels are instantiated for every radius 0 .. 12: the
// trip count of the tap loop is what the register blocking is built on.  LDS per workgroup: (32 + 2 R)(60 + roundup4(8 + 2 R)) 4
// bytes, 20.1 KiB at R = 12.
#include "common.h"
#include "np_exact.h"

#include <cmath>

namespace apgpu {
namespace {

constexpr int kBlock = 256;
constexpr int kTileW = APGPU_DECONV_TILE_W, kTileH = APGPU_DECONV_TILE_H;
constexpr int kMaxR = APGPU_DECONV_MAX_RADIUS;
constexpr int kMaxK = 2 * kMaxR + 1;
constexpr int kRun = 8;                                     // outputs per lane, along x
constexpr int kRuns = kTileW / kRun;                        // runs per tile row
static_assert(kRuns * kTileH == kBlock, "a lane owns one run of the tile");

struct Psf {
    float w[kMaxK * kMaxK];                                 // [K][K], row stride K = 2 R + 1 of the launch
};

template <int R>
struct Geo {
    static constexpr int K = 2 * R + 1;
    static constexpr int NV = (kRun + 2 * R + 3) & ~3;      // floats a lane reads per PSF row, whole 16-byte groups
    static constexpr int ROWS = kTileH + 2 * R, COLS = kTileW + 2 * R;
    static constexpr int S = kTileW - kRun + NV + 4;        // LDS row stride: the last run's reads stay inside the row; 16-byte multiple
    static_assert(S >= COLS && S % 4 == 0, "LDS row stride");
};

enum { kForward = 0, kBackward = 1, kValidity = 2 };

// Stages rows ty0 - R .. ty0 + 31 + R, columns tx0 - R .. tx0 + 63 + R of `src` by the rule of the pass.  Every global read is
// inside the image: the forward rule clamps the coordinates, the other two test them.
template <int R, int RULE>
__device__ __forceinline__ void stage(float *tile, const float *__restrict__ src, long long H, long long W, long long ty0, long long tx0)
{
    using G = Geo<R>;
    for (int idx = threadIdx.x; idx < G::ROWS * G::COLS; idx += kBlock) {
        const int lr = idx / G::COLS, lc = idx - lr * G::COLS;
        long long gy = ty0 - R + lr, gx = tx0 - R + lc;
        float v;
        if (RULE == kForward) {
            gy = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);
            gx = gx < 0 ? 0 : (gx > W - 1 ? W - 1 : gx);
            v = src[(size_t)gy * (size_t)W + (size_t)gx];
        } else {
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
            v = in ? src[(size_t)gy * (size_t)W + (size_t)gx] : 0.0f;
            if (RULE == kValidity) v = in && is_finite(v) ? 1.0f : 0.0f;
        }
        tile[lr * G::S + lc] = v;
    }
}

// acc[o] = sum over the taps in row-major order, for the run of 8 outputs of tile row ly that starts at tile column 8 run.
// FLIP: the convolution (tap (j, i) reads the pixel at (+R - j, +R - i)); otherwise the correlation ((j - R, i - R)).
template <int R, bool FLIP>
__device__ __forceinline__ void taps_run(const float *tile, const Psf &psf, int ly, int run, float (&acc)[kRun])
{
    using G = Geo<R>;
#pragma unroll
    for (int o = 0; o < kRun; o++) acc[o] = 0.0f;
#pragma unroll 1
    for (int j = 0; j < G::K; j++) {
        const float4 *row = reinterpret_cast<const float4 *>(tile + (FLIP ? ly + 2 * R - j : ly + j) * G::S + kRun * run);
        float v[G::NV];
#pragma unroll
        for (int g = 0; g < G::NV / 4; g++) {
            const float4 t = row[g];
            v[4 * g] = t.x; v[4 * g + 1] = t.y; v[4 * g + 2] = t.z; v[4 * g + 3] = t.w;
        }
        const float *w = psf.w + j * G::K;
#pragma unroll
        for (int i = 0; i < G::K; i++) {
            const float wi = w[i];
#pragma unroll
            for (int o = 0; o < kRun; o++) acc[o] = acc[o] + wi * v[FLIP ? o + 2 * R - i : o + i];
        }
    }
}

// Four consecutive pixels of an image row, from column xs (a multiple of 4): one 16-byte access where `wide` (every plane 16-byte
// aligned and W a multiple of 4, so that the four lie inside the row together), single values inside the row otherwise.
__device__ __forceinline__ void load4(const float *__restrict__ p, size_t base, long long xs, long long W, int wide, float (&v)[4])
{
    if (wide) {
        const float4 t = *reinterpret_cast<const float4 *>(p + base + xs);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = xs + k < W ? p[base + xs + k] : 0.0f;
    }
}

__device__ __forceinline__ void store4(float *__restrict__ p, size_t base, long long xs, long long W, int wide, const float (&v)[4])
{
    if (wide) {
        *reinterpret_cast<float4 *>(p + base + xs) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (xs + k < W) p[base + xs + k] = v[k];
    }
}

struct RatioArgs {
    float sky, gain, rn2, t2;                               // rn2 = rn rn, t2 = T T, both rounded to float32 once
    int damped;                                             // T > 0
};

// The ratio of step 3 from the pixel d and the forward sum (before the sky is added).
__device__ __forceinline__ float ratio1(float d, float sum, const RatioArgs &a)
{
    const float c = sum + a.sky;
    if (!is_finite(d)) return 0.0f;
    if (!(c > 0.0f)) return 1.0f;
    float r;
    if (!a.damped) {
        r = d / c;
    } else {
        const float e = d - c;
        const float var = (c > 0.0f ? c : 0.0f) / a.gain + a.rn2;
        const float t = (e * e) / (a.t2 * var);
        const float U = t < 1.0f ? t : 1.0f;                // min(t, 1); a NaN (0 / 0) counts as 1
        const float U2 = U * U, U4 = U2 * U2, U8 = U4 * U4, U9 = U8 * U;
        const float w = U9 * (10.0f - 9.0f * U);
        r = 1.0f + (w * e) / c;
    }
    return r > 0.0f ? r : 0.0f;
}

template <int R>
__global__ __launch_bounds__(kBlock) void deconv_ratio_kernel(const float *__restrict__ u, const float *__restrict__ data, long long H, long long W,
                                                             const Psf psf, const RatioArgs a, int wide, float *__restrict__ rout)
{
    using G = Geo<R>;
    __shared__ __attribute__((aligned(16))) float tile[G::ROWS * G::S];
    const long long tx0 = (long long)blockIdx.x * kTileW, ty0 = (long long)blockIdx.y * kTileH;
    stage<R, kForward>(tile, u, H, W, ty0, tx0);
    __syncthreads();
    const int run = threadIdx.x % kRuns, ly = threadIdx.x / kRuns;
    float acc[kRun];
    taps_run<R, true>(tile, psf, ly, run, acc);
    const long long y = ty0 + ly, x0 = tx0 + kRun * run;
    if (y >= H) return;
    const size_t base = (size_t)y * (size_t)W;
#pragma unroll
    for (int h = 0; h < kRun / 4; h++) {
        const long long xs = x0 + 4 * h;
        if (xs >= W) break;
        float d[4], r[4];
        load4(data, base, xs, W, wide, d);
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = ratio1(d[k], acc[4 * h + k], a);
        store4(rout, base, xs, W, wide, r);
    }
}

// data NULL: out = u'.  data given (the last iteration): out = u' + sky where data is finite, NaN elsewhere.
template <int R>
__global__ __launch_bounds__(kBlock) void deconv_update_kernel(const float *__restrict__ u, const float *__restrict__ r, const float *__restrict__ inv,
                                                              const float *__restrict__ data, float sky, long long H, long long W, const Psf psf,
                                                              int wide, float *__restrict__ out)
{
    using G = Geo<R>;
    __shared__ __attribute__((aligned(16))) float tile[G::ROWS * G::S];
    const long long tx0 = (long long)blockIdx.x * kTileW, ty0 = (long long)blockIdx.y * kTileH;
    stage<R, kBackward>(tile, r, H, W, ty0, tx0);
    __syncthreads();
    const int run = threadIdx.x % kRuns, ly = threadIdx.x / kRuns;
    float acc[kRun];
    taps_run<R, false>(tile, psf, ly, run, acc);
    const long long y = ty0 + ly, x0 = tx0 + kRun * run;
    if (y >= H) return;
    const size_t base = (size_t)y * (size_t)W;
#pragma unroll
    for (int h = 0; h < kRun / 4; h++) {
        const long long xs = x0 + 4 * h;
        if (xs >= W) break;
        float uv[4], iv[4], o[4];
        load4(u, base, xs, W, wide, uv);
        load4(inv, base, xs, W, wide, iv);
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = iv[k] != 0.0f ? (uv[k] * acc[4 * h + k]) * iv[k] : uv[k];
        if (data) {
            float d[4];
            load4(data, base, xs, W, wide, d);
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = is_finite(d[k]) ? o[k] + sky : quiet_nan();
        }
        store4(out, base, xs, W, wide, o);
    }
}

// The norm plane, and on the way (the pixels are in LDS already) the start of the iteration: u0 = the start plane or the start
// level where u0 is given, and the output of zero iterations (u0 + sky, NaN at the invalid pixels) where out is given.
template <int R>
__global__ __launch_bounds__(kBlock) void deconv_norm_kernel(const float *__restrict__ data, long long H, long long W, const Psf psf, float min_weight,
                                                            const float *__restrict__ start_plane, float start_level, float sky, int wide,
                                                            float *__restrict__ inv, float *__restrict__ u0, float *__restrict__ out)
{
    using G = Geo<R>;
    __shared__ __attribute__((aligned(16))) float tile[G::ROWS * G::S];
    const long long tx0 = (long long)blockIdx.x * kTileW, ty0 = (long long)blockIdx.y * kTileH;
    stage<R, kValidity>(tile, data, H, W, ty0, tx0);
    __syncthreads();
    const int run = threadIdx.x % kRuns, ly = threadIdx.x / kRuns;
    float acc[kRun];
    taps_run<R, false>(tile, psf, ly, run, acc);
    const long long y = ty0 + ly, x0 = tx0 + kRun * run;
    if (y >= H) return;
    const size_t base = (size_t)y * (size_t)W;
#pragma unroll
    for (int h = 0; h < kRun / 4; h++) {
        const long long xs = x0 + 4 * h;
        if (xs >= W) break;
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = acc[4 * h + k] >= min_weight ? 1.0f / acc[4 * h + k] : 0.0f;
        store4(inv, base, xs, W, wide, o);
        if (!u0 && !out) continue;
        float s[4] = {start_level, start_level, start_level, start_level};
        if (start_plane) load4(start_plane, base, xs, W, wide, s);
        if (u0) store4(u0, base, xs, W, wide, s);
        if (out) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                o[k] = tile[(ly + R) * G::S + kRun * run + 4 * h + k + R] != 0.0f ? s[k] + sky : quiet_nan();
            store4(out, base, xs, W, wide, o);
        }
    }
}

inline size_t plane_bytes(int64_t height, int64_t width) { return (((size_t)height * (size_t)width * sizeof(float)) + 255) & ~(size_t)255; }

// The image shape and the stamp: what every entry point checks first.  Fills psf (row stride 2 radius + 1) and the grid.
int check_common(const char *what, int64_t height, int64_t width, const float *psf_host, int32_t radius, Psf *psf, dim3 *grid)
{
    if (height <= 0 || width <= 0) return fail(APGPU_EINVAL, "%s: image of %lld x %lld", what, (long long)height, (long long)width);
    if (!psf_host) return fail(APGPU_EINVAL, "%s: NULL pointer argument", what);
    if (radius < 0) return fail(APGPU_EINVAL, "%s: radius %d", what, radius);
    if (radius > kMaxR) return fail(APGPU_EUNSUPPORTED, "%s: radius %d, the kernels hold %d", what, radius, kMaxR);
    const int n = (2 * radius + 1) * (2 * radius + 1);
    double sum = 0.0;
    for (int k = 0; k < n; k++) {
        const float w = psf_host[k];
        if (!std::isfinite(w) || w < 0.0f) return fail(APGPU_EINVAL, "%s: PSF weight %d is %g: the weights must be finite and >= 0", what, k, (double)w);
        sum += (double)w;
    }
    if (!(sum > 0.0)) return fail(APGPU_EINVAL, "%s: the PSF weights sum to %g", what, sum);
    for (int k = 0; k < kMaxK * kMaxK; k++) psf->w[k] = k < n ? psf_host[k] : 0.0f;
    return tile_grid(what, height, width, kTileH, kTileW, grid);
}

#define APGPU_DECONV_RADII(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)

void launch_norm(int radius, dim3 grid, hipStream_t s, const float *data, long long H, long long W, const Psf &psf, float min_weight,
                 const float *start_plane, float start_level, float sky, float *inv, float *u0, float *out)
{
    const int wide = wide_rows(W, data, inv, start_plane, u0, out);
    switch (radius) {
#define X(RR) case RR: hipLaunchKernelGGL((deconv_norm_kernel<RR>), grid, dim3(kBlock), 0, s, data, H, W, psf, min_weight, start_plane, start_level, sky, wide, inv, u0, out); break;
        APGPU_DECONV_RADII(X)
#undef X
    }
}

void launch_ratio(int radius, dim3 grid, hipStream_t s, const float *u, const float *data, long long H, long long W, const Psf &psf,
                  const RatioArgs &a, float *rout)
{
    const int wide = wide_rows(W, data, rout);
    switch (radius) {
#define X(RR) case RR: hipLaunchKernelGGL((deconv_ratio_kernel<RR>), grid, dim3(kBlock), 0, s, u, data, H, W, psf, a, wide, rout); break;
        APGPU_DECONV_RADII(X)
#undef X
    }
}

void launch_update(int radius, dim3 grid, hipStream_t s, const float *u, const float *r, const float *inv, const float *data, float sky,
                   long long H, long long W, const Psf &psf, float *out)
{
    const int wide = wide_rows(W, u, inv, data, out);
    switch (radius) {
#define X(RR) case RR: hipLaunchKernelGGL((deconv_update_kernel<RR>), grid, dim3(kBlock), 0, s, u, r, inv, data, sky, H, W, psf, wide, out); break;
        APGPU_DECONV_RADII(X)
#undef X
    }
}

int check_noise(const char *what, float sky, float gain, float readnoise, float damp, RatioArgs *a)
{
    if (!(sky >= 0.0f) || !std::isfinite(sky)) return fail(APGPU_EINVAL, "%s: sky %g must be finite and >= 0", what, (double)sky);
    if (!(gain > 0.0f) || !std::isfinite(gain)) return fail(APGPU_EINVAL, "%s: gain %g must be finite and > 0", what, (double)gain);
    if (!(readnoise >= 0.0f) || !std::isfinite(readnoise)) return fail(APGPU_EINVAL, "%s: read noise %g must be finite and >= 0", what, (double)readnoise);
    if (!(damp >= 0.0f) || !std::isfinite(damp)) return fail(APGPU_EINVAL, "%s: damping threshold %g must be finite and >= 0", what, (double)damp);
    a->sky = sky;
    a->gain = gain;
    a->rn2 = readnoise * readnoise;
    a->t2 = damp * damp;
    a->damped = damp > 0.0f;
    return APGPU_OK;
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" size_t apgpu_deconv_ws_bytes(int64_t height, int64_t width)
{
    return height > 0 && width > 0 ? 4 * plane_bytes(height, width) : 0;
}

extern "C" int apgpu_deconv_norm_f32(const float *data, int64_t height, int64_t width, const float *psf_host, int32_t radius, float min_weight,
                                     float *inv, void *stream)
{
    Psf psf;
    dim3 grid;
    if (!data || !inv) return fail(APGPU_EINVAL, "deconv_norm: NULL pointer argument");
    if (const int rc = check_common("deconv_norm", height, width, psf_host, radius, &psf, &grid)) return rc;
    if (!(min_weight >= 0.0f)) return fail(APGPU_EINVAL, "deconv_norm: min_weight %g", (double)min_weight);
    if (data == inv) return fail(APGPU_EINVAL, "deconv_norm: inv must not be the input");
    if (!aligned(data, 4) || !aligned(inv, 4)) return fail(APGPU_EINVAL, "deconv_norm: data and inv must be 4-byte aligned");
    launch_norm(radius, grid, as_stream(stream), data, height, width, psf, min_weight, nullptr, 0.0f, 0.0f, inv, nullptr, nullptr);
    return check_launch("deconv_norm");
}

extern "C" int apgpu_deconv_ratio_f32(const float *u, const float *data, int64_t height, int64_t width, const float *psf_host, int32_t radius,
                                      float sky, float gain, float readnoise, float damp, float *ratio, void *stream)
{
    Psf psf;
    dim3 grid;
    RatioArgs a;
    if (!u || !data || !ratio) return fail(APGPU_EINVAL, "deconv_ratio: NULL pointer argument");
    if (const int rc = check_common("deconv_ratio", height, width, psf_host, radius, &psf, &grid)) return rc;
    if (const int rc = check_noise("deconv_ratio", sky, gain, readnoise, damp, &a)) return rc;
    if (ratio == u) return fail(APGPU_EINVAL, "deconv_ratio: ratio must not be u");
    if (!aligned(u, 4) || !aligned(data, 4) || !aligned(ratio, 4)) return fail(APGPU_EINVAL, "deconv_ratio: the planes must be 4-byte aligned");
    launch_ratio(radius, grid, as_stream(stream), u, data, height, width, psf, a, ratio);
    return check_launch("deconv_ratio");
}

extern "C" int apgpu_deconv_update_f32(const float *u, const float *ratio, const float *inv, int64_t height, int64_t width, const float *psf_host,
                                       int32_t radius, float *u_out, void *stream)
{
    Psf psf;
    dim3 grid;
    if (!u || !ratio || !inv || !u_out) return fail(APGPU_EINVAL, "deconv_update: NULL pointer argument");
    if (const int rc = check_common("deconv_update", height, width, psf_host, radius, &psf, &grid)) return rc;
    if (u_out == ratio) return fail(APGPU_EINVAL, "deconv_update: u_out must not be the ratio plane");
    if (!aligned(u, 4) || !aligned(ratio, 4) || !aligned(inv, 4) || !aligned(u_out, 4))
        return fail(APGPU_EINVAL, "deconv_update: the planes must be 4-byte aligned");
    launch_update(radius, grid, as_stream(stream), u, ratio, inv, nullptr, 0.0f, height, width, psf, u_out);
    return check_launch("deconv_update");
}

extern "C" int apgpu_richardson_lucy_f32(const float *data, int64_t height, int64_t width, const float *psf_host, int32_t radius, float sky, float gain,
                                         float readnoise, float damp, int32_t niter, float start_level, const float *start_plane, float min_weight,
                                         float *out, void *ws, size_t ws_bytes, void *stream)
{
    Psf psf;
    dim3 grid;
    RatioArgs a;
    if (!data || !out || !ws) return fail(APGPU_EINVAL, "richardson_lucy: NULL pointer argument");
    if (const int rc = check_common("richardson_lucy", height, width, psf_host, radius, &psf, &grid)) return rc;
    if (const int rc = check_noise("richardson_lucy", sky, gain, readnoise, damp, &a)) return rc;
    if (niter < 0) return fail(APGPU_EINVAL, "richardson_lucy: %d iterations", niter);
    if (!(min_weight >= 0.0f)) return fail(APGPU_EINVAL, "richardson_lucy: min_weight %g", (double)min_weight);
    if (!start_plane && (!(start_level > 0.0f) || !std::isfinite(start_level)))
        return fail(APGPU_EINVAL, "richardson_lucy: start level %g must be finite and > 0", (double)start_level);
    if (out == data || start_plane == out) return fail(APGPU_EINVAL, "richardson_lucy: out must not be the input or the start plane");
    if (!aligned(data, 4) || !aligned(out, 4) || !aligned(start_plane, 4) || !aligned(ws, 16))
        return fail(APGPU_EINVAL, "richardson_lucy: data, out and the start plane must be 4-byte aligned, ws 16-byte aligned");
    if (ws_bytes < apgpu_deconv_ws_bytes(height, width))
        return fail(APGPU_EINVAL, "richardson_lucy: workspace of %zu bytes, %zu needed", ws_bytes, apgpu_deconv_ws_bytes(height, width));
    const size_t pb = plane_bytes(height, width);
    char *base = static_cast<char *>(ws);
    float *ratio = reinterpret_cast<float *>(base), *inv = reinterpret_cast<float *>(base + pb);
    float *ua = reinterpret_cast<float *>(base + 2 * pb), *ub = reinterpret_cast<float *>(base + 3 * pb);
    hipStream_t s = as_stream(stream);
    launch_norm(radius, grid, s, data, height, width, psf, min_weight, start_plane, start_level, sky, inv, niter > 0 ? ua : nullptr,
                niter > 0 ? nullptr : out);
    if (const int rc = check_launch("richardson_lucy (norm)")) return rc;
    for (int it = 0; it < niter; it++) {
        const bool last = it == niter - 1;
        launch_ratio(radius, grid, s, ua, data, height, width, psf, a, ratio);
        launch_update(radius, grid, s, ua, ratio, inv, last ? data : nullptr, sky, height, width, psf, last ? out : ub);
        float *t = ua;
        ua = ub;
        ub = t;
    }
    return check_launch("richardson_lucy");
}
