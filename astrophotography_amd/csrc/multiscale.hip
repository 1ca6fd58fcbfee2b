// multiscale.hip - F13: the B3-spline a trous ("starlet") transform on gfx950, one launch per scale: the smoothing step c_j -> c_{j+1},
// the plane w_{j+1} = c_j - c_{j+1}, its threshold and gain, and the running sum of the reconstruction, fused.
//
// The reference has no such stage, so the arithmetic is this project's own definition (include/apgpu.h F13), restated in
// tests/multiscale_model.py.  No contraction anywhere: every multiply and add rounds on its own.
//
//   taps     h = {1, 4, 6, 4, 1} / 16 at offsets (k - 2) s, s = 2^j.  valid(y, x) = inside the image and finite.
//   step     row pass     a(y, x) = sum_k h[k] double(c(y, x + (k - 2) s)), m(y, x) = sum_k h[k], both over the valid taps, k ascending,
//                         float64, accumulators starting at +0
//            column pass  A(y, x) = sum_k h[k] a(y + (k - 2) s, x), M(y, x) = sum_k h[k] m(y + (k - 2) s, x) over the rows inside the image
//            next         c'(y, x) = float32(A / M) where valid(y, x), NaN elsewhere
//   plane    w = c - c' in float32 (NaN at the holes)
//   sum      acc' = acc + g T(w), acc = +0 in the first step; T: hard w where |w| >= t, else +0; soft w - t above t, w + t below -t,
//            else +0.  The last step adds g_res c'.  Holes are written as NaN.
//
// Two forms of the one kernel, the same sums in the same order, so the same bits:
//   tile     (spacing <= 8) a workgroup of 256 lanes owns 32 rows x 64 columns, stages them with a halo of 2 s in LDS (out-of-image
//            pixels as NaN, so "inside and finite" is one test; origin rounded down to a multiple of four columns for 16-byte loads),
//            writes (a, m) for the 32 + 4 s staged rows to LDS, a wavefront per row, and sums the columns from there: the layout of
//            continuum.hip's blur with dilated taps.  The halo is read again by the neighbours: (32 + 4 s)(64 + 4 s) / (32 64) times
//            the image, 1.2 at s = 1 and 3 at s = 8.
//   direct   (any spacing) a lane owns one column of a chain of kChain outputs s rows apart, y0 + i s.  Their column taps fall on
//            the same chain, so the lane computes (a, m) once per chain row, kChain + 4 of them for kChain outputs, keeps the last
//            five in registers and slides: 5 (kChain + 4) / kChain = 7.5 row-coalesced loads per output instead of 25, no LDS, no
//            barrier.  The taps a workgroup's neighbours read again come from L2 and the Infinity Cache.
// Rows outside the image enter the column sums as (a, m) = (+0, +0): h 0 = +0 leaves an accumulator (never -0) as it is, as skipping does.
#include "common.h"
#include "np_exact.h"
#include "plane_tile.h"

namespace apgpu {
namespace {

constexpr int kBlock = 256;
constexpr int kTileW = APGPU_STARLET_TILE_W, kTileH = APGPU_STARLET_TILE_H;
constexpr int kChain = APGPU_STARLET_CHAIN;
constexpr int kMaxSpacing = 1 << (APGPU_STARLET_MAX_SCALES - 1);
static_assert(kTileW == kWave, "a wavefront owns one tile row");

struct StepScalars {
    float t, gain, g_res;                                   // threshold, gain of this plane, gain of the residual
    int soft, first, last;
};

__device__ __forceinline__ double tap(int k) { return k == 2 ? 0.375 : (k == 1 || k == 3 ? 0.25 : 0.0625); }

// One output pixel: c is c_j there, (A, M) the column sums.
__device__ __forceinline__ void emit(float *__restrict__ c_out, float *__restrict__ w_out, float *__restrict__ acc, const StepScalars &p, size_t idx,
                                     float c, double A, double M)
{
    const float nanv = quiet_nan();
    const bool ok = is_finite(c);
    const float cn = ok ? (float)(A / M) : nanv;
    if (c_out) c_out[idx] = cn;
    const float w = ok ? c - cn : nanv;
    if (w_out) w_out[idx] = w;
    if (acc) {
        float tw;
        if (p.soft) tw = w > p.t ? w - p.t : (w < -p.t ? w + p.t : 0.0f);
        else tw = fabsf(w) >= p.t ? w : 0.0f;
        const float prev = p.first ? 0.0f : acc[idx];
        float v = prev + p.gain * tw;
        if (p.last) v = v + p.g_res * cn;
        acc[idx] = ok ? v : nanv;
    }
}

template <int S>
__global__ __launch_bounds__(kBlock) void starlet_tile_kernel(const float *__restrict__ in, float *__restrict__ c_out, float *__restrict__ w_out,
                                                             float *__restrict__ acc, long long H, long long W, int wide, const StepScalars p)
{
    constexpr int R = 2 * S;
    constexpr int kInH = kTileH + 2 * R;
    constexpr int kInW = halo_pitch(kTileW, R);
    __shared__ __attribute__((aligned(16))) float tile[kInH][kInW];
    __shared__ double sa[kInH][kTileW];
    __shared__ float sm[kInH][kTileW];                      // a sum of sixteenths, at most 1: exact in float32
    const long long tx0 = (long long)blockIdx.x * kTileW, ty0 = (long long)blockIdx.y * kTileH;
    const int off = stage_halo<kInW, kBlock>(tile, in, H, W, tx0, ty0, kTileW, R, kInH, wide);
    __syncthreads();

    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const bool col_in = tx0 + lane < W;
    // row pass: wavefront -> staged row, lane -> tile column
    for (int lr = wave; lr < kInH; lr += kBlock / kWave) {
        const long long gy = ty0 - R + lr;
        double a = 0.0, m = 0.0;
        if (gy >= 0 && gy < H && col_in) {
            const float *q = &tile[lr][off + lane];
#pragma unroll
            for (int k = 0; k < 5; k++) row_add(a, m, q[k * S], tap(k));
        }
        sa[lr][lane] = a;
        sm[lr][lane] = (float)m;
    }
    __syncthreads();

    // column pass: wavefront -> tile row, lane -> tile column
    if (!col_in) return;
    for (int ly = wave; ly < kTileH; ly += kBlock / kWave) {
        const long long gy = ty0 + ly;
        if (gy >= H) break;
        double A = 0.0, M = 0.0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            A = A + tap(k) * sa[ly + k * S][lane];
            M = M + tap(k) * (double)sm[ly + k * S][lane];
        }
        emit(c_out, w_out, acc, p, (size_t)gy * (size_t)W + (size_t)(tx0 + lane), tile[ly + R][off + R + lane], A, M);
    }
}

__global__ __launch_bounds__(kBlock) void starlet_direct_kernel(const float *__restrict__ in, float *__restrict__ c_out, float *__restrict__ w_out,
                                                               float *__restrict__ acc, long long H, long long W, int s, const StepScalars p)
{
    const long long x = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (x >= W) return;
    // chain blockIdx.y: group q = chain / s of s kChain rows, row rho = chain % s inside it; outputs y0 + i s, i = 0 .. kChain - 1
    const long long q = (long long)blockIdx.y / s, rho = (long long)blockIdx.y - q * s;
    const long long y0 = q * s * kChain + rho;
    if (y0 >= H) return;
    const float nanv = quiet_nan();
    long long xo[5];
    bool xin[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const long long xx = x + (long long)(k - 2) * s;
        xin[k] = xx >= 0 && xx < W;
        xo[k] = xin[k] ? xx : x;
    }
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    float centre[3] = {nanv, nanv, nanv};
#pragma unroll
    for (int i = -2; i < kChain + 2; i++) {
        const long long y = y0 + (long long)i * s;         // the chain row entering the window
        double ai = 0.0, mi = 0.0;
        float cv = nanv;
        if (y >= 0 && y < H) {
            const float *row = in + (size_t)y * (size_t)W;
            float v[5];
#pragma unroll
            for (int k = 0; k < 5; k++) v[k] = xin[k] ? row[xo[k]] : nanv;
#pragma unroll
            for (int k = 0; k < 5; k++) row_add(ai, mi, v[k], tap(k));
            cv = v[2];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            a[k] = a[k + 1];
            m[k] = m[k + 1];
        }
        a[4] = ai;
        m[4] = mi;
        centre[0] = centre[1];
        centre[1] = centre[2];
        centre[2] = cv;
        if (i >= 2) {                                       // the window holds rows yc - 2 s .. yc + 2 s
            const long long yc = y0 + (long long)(i - 2) * s;
            if (yc < H) {
                double A = 0.0, M = 0.0;
#pragma unroll
                for (int k = 0; k < 5; k++) {
                    A = A + tap(k) * a[k];
                    M = M + tap(k) * m[k];
                }
                emit(c_out, w_out, acc, p, (size_t)yc * (size_t)W + (size_t)x, centre[0], A, M);
            }
        }
    }
}

inline bool finite_f(float x) { return is_finite(x); }

inline size_t plane_stride(int64_t height, int64_t width) { return ((size_t)height * (size_t)width + 3) & ~(size_t)3; }

// One launch.  The planes are distinct and 4-byte aligned, spacing is a power of two <= kMaxSpacing: the callers have checked.
int launch_step(const char *what, const float *in, int64_t height, int64_t width, int spacing, float *c_out, float *w_out, float *acc,
                const StepScalars &p, int form, hipStream_t st)
{
    const long long H = height, W = width;
    dim3 grid;
    if (form == APGPU_STARLET_FORM_AUTO) form = spacing <= APGPU_STARLET_TILE_MAX_AUTO ? APGPU_STARLET_FORM_TILE : APGPU_STARLET_FORM_DIRECT;
    if (form == APGPU_STARLET_FORM_TILE) {
        if (spacing > APGPU_STARLET_TILE_MAX_SPACING)
            return fail(APGPU_EUNSUPPORTED, "%s: the tile form holds a spacing of %d, got %d", what, APGPU_STARLET_TILE_MAX_SPACING, spacing);
        if (int rc = tile_grid(what, H, W, kTileH, kTileW, &grid)) return rc;
        const int wide = wide_rows(W, in);
        if (spacing == 1) hipLaunchKernelGGL((starlet_tile_kernel<1>), grid, dim3(kBlock), 0, st, in, c_out, w_out, acc, H, W, wide, p);
        else if (spacing == 2) hipLaunchKernelGGL((starlet_tile_kernel<2>), grid, dim3(kBlock), 0, st, in, c_out, w_out, acc, H, W, wide, p);
        else if (spacing == 4) hipLaunchKernelGGL((starlet_tile_kernel<4>), grid, dim3(kBlock), 0, st, in, c_out, w_out, acc, H, W, wide, p);
        else hipLaunchKernelGGL((starlet_tile_kernel<8>), grid, dim3(kBlock), 0, st, in, c_out, w_out, acc, H, W, wide, p);
    } else {
        const long long blocks_x = (W + kBlock - 1) / kBlock;
        const long long chains = (H + (long long)spacing * kChain - 1) / ((long long)spacing * kChain) * spacing;
        if (int rc = launch_grid(what, H, W, blocks_x, chains, &grid)) return rc;
        hipLaunchKernelGGL(starlet_direct_kernel, grid, dim3(kBlock), 0, st, in, c_out, w_out, acc, H, W, spacing, p);
    }
    return check_launch(what);
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_starlet_step_f32(const float *c_in, int64_t height, int64_t width, int32_t spacing, float *c_out, float *w_out, float *acc,
                                      float threshold, float gain, float g_res, int32_t mode, int32_t flags, int32_t form, void *stream)
{
    if (int rc = check_plane("starlet_step", c_in, height, width)) return rc;
    if (!c_out && !w_out && !acc) return fail(APGPU_EINVAL, "starlet_step: no output plane");
    if (spacing < 1 || spacing > kMaxSpacing || (spacing & (spacing - 1)))
        return fail(APGPU_EINVAL, "starlet_step: spacing %d is not a power of two from 1 to %d", spacing, kMaxSpacing);
    if (c_out == c_in || w_out == c_in || acc == c_in || (c_out && (c_out == w_out || c_out == acc)) || (w_out && w_out == acc))
        return fail(APGPU_EINVAL, "starlet_step: the planes must be distinct");
    if (!aligned(c_out, 4) || !aligned(w_out, 4) || !aligned(acc, 4)) return fail(APGPU_EINVAL, "starlet_step: the planes must be 4-byte aligned");
    if (!(threshold >= 0.0f) || !finite_f(threshold)) return fail(APGPU_EINVAL, "starlet_step: threshold %g", (double)threshold);
    if (!finite_f(gain) || !finite_f(g_res)) return fail(APGPU_EINVAL, "starlet_step: gains %g, %g", (double)gain, (double)g_res);
    if (mode != APGPU_STARLET_HARD && mode != APGPU_STARLET_SOFT) return fail(APGPU_EINVAL, "starlet_step: mode %d", mode);
    if (flags & ~(APGPU_STARLET_FIRST | APGPU_STARLET_LAST)) return fail(APGPU_EINVAL, "starlet_step: flags %d", flags);
    if (form != APGPU_STARLET_FORM_AUTO && form != APGPU_STARLET_FORM_TILE && form != APGPU_STARLET_FORM_DIRECT)
        return fail(APGPU_EINVAL, "starlet_step: form %d", form);
    const StepScalars p = {threshold, gain, g_res, mode == APGPU_STARLET_SOFT, (flags & APGPU_STARLET_FIRST) != 0, (flags & APGPU_STARLET_LAST) != 0};
    return launch_step("starlet_step", c_in, height, width, spacing, c_out, w_out, acc, p, form, as_stream(stream));
}

extern "C" size_t apgpu_starlet_ws_bytes(int64_t height, int64_t width)
{
    return height > 0 && width > 0 ? 2 * plane_stride(height, width) * sizeof(float) : 0;
}

extern "C" int apgpu_starlet_plane1_f32(const float *data, int64_t height, int64_t width, float *w1, void *stream)
{
    if (int rc = check_plane("starlet_plane1", data, height, width)) return rc;
    if (!w1 || w1 == data || !aligned(w1, 4)) return fail(APGPU_EINVAL, "starlet_plane1: w1 must be a 4-byte aligned plane distinct from the input");
    const StepScalars p = {0.0f, 1.0f, 1.0f, 0, 1, 0};
    return launch_step("starlet_plane1", data, height, width, 1, nullptr, w1, nullptr, p, APGPU_STARLET_FORM_AUTO, as_stream(stream));
}

static int check_ws(const char *what, const float *data, int64_t height, int64_t width, int32_t scales, const float *out, size_t out_planes,
                    const void *ws, size_t ws_bytes)
{
    if (int rc = check_plane(what, data, height, width)) return rc;
    if (!out || !ws) return fail(APGPU_EINVAL, "%s: NULL pointer argument", what);
    if (scales < 1 || scales > APGPU_STARLET_MAX_SCALES) return fail(APGPU_EINVAL, "%s: %d scales, 1 to %d are built", what, scales, APGPU_STARLET_MAX_SCALES);
    if (!aligned(out, 4) || !aligned(ws, 16)) return fail(APGPU_EINVAL, "%s: out must be 4-byte aligned, ws 16-byte aligned", what);
    if (ws_bytes < apgpu_starlet_ws_bytes(height, width))
        return fail(APGPU_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, apgpu_starlet_ws_bytes(height, width));
    // out, the workspace and the input must not overlap
    const char *d0 = reinterpret_cast<const char *>(data), *d1 = d0 + (size_t)height * (size_t)width * sizeof(float);
    const char *o0 = reinterpret_cast<const char *>(out), *o1 = o0 + out_planes * (size_t)height * (size_t)width * sizeof(float);
    const char *w0 = static_cast<const char *>(ws), *w1 = w0 + apgpu_starlet_ws_bytes(height, width);
    if ((d0 < o1 && o0 < d1) || (d0 < w1 && w0 < d1) || (o0 < w1 && w0 < o1)) return fail(APGPU_EINVAL, "%s: data, out and ws must not overlap", what);
    return APGPU_OK;
}

extern "C" int apgpu_starlet_planes_f32(const float *data, int64_t height, int64_t width, int32_t scales, float *planes, void *ws, size_t ws_bytes,
                                        void *stream)
{
    if (int rc = check_ws("starlet_planes", data, height, width, scales, planes, (size_t)scales + 1, ws, ws_bytes)) return rc;
    const size_t npix = (size_t)height * (size_t)width, stride = plane_stride(height, width);
    float *pp[2] = {static_cast<float *>(ws), static_cast<float *>(ws) + stride};
    const StepScalars p = {0.0f, 1.0f, 1.0f, 0, 1, 0};
    const float *c = data;
    for (int j = 0; j < scales; j++) {
        float *next = j == scales - 1 ? planes + (size_t)scales * npix : pp[j & 1];
        if (int rc = launch_step("starlet_planes", c, height, width, 1 << j, next, planes + (size_t)j * npix, nullptr, p, APGPU_STARLET_FORM_AUTO,
                                 as_stream(stream)))
            return rc;
        c = next;
    }
    return APGPU_OK;
}

extern "C" int apgpu_multiscale_f32(const float *data, int64_t height, int64_t width, int32_t scales, const float *thresholds_host,
                                    const float *gains_host, float g_res, int32_t mode, float *out, void *ws, size_t ws_bytes, void *stream)
{
    if (int rc = check_ws("multiscale", data, height, width, scales, out, 1, ws, ws_bytes)) return rc;
    if (!thresholds_host || !gains_host) return fail(APGPU_EINVAL, "multiscale: NULL pointer argument");
    if (mode != APGPU_STARLET_HARD && mode != APGPU_STARLET_SOFT) return fail(APGPU_EINVAL, "multiscale: mode %d", mode);
    if (!finite_f(g_res)) return fail(APGPU_EINVAL, "multiscale: residual gain %g", (double)g_res);
    for (int j = 0; j < scales; j++) {
        if (!(thresholds_host[j] >= 0.0f) || !finite_f(thresholds_host[j]))
            return fail(APGPU_EINVAL, "multiscale: threshold %d is %g", j + 1, (double)thresholds_host[j]);
        if (!finite_f(gains_host[j])) return fail(APGPU_EINVAL, "multiscale: gain %d is %g", j + 1, (double)gains_host[j]);
    }
    const size_t stride = plane_stride(height, width);
    float *pp[2] = {static_cast<float *>(ws), static_cast<float *>(ws) + stride};
    const float *c = data;
    for (int j = 0; j < scales; j++) {
        const bool last = j == scales - 1;
        float *next = last ? nullptr : pp[j & 1];           // c_J is only needed inside its own launch
        const StepScalars p = {thresholds_host[j], gains_host[j], g_res, mode == APGPU_STARLET_SOFT, j == 0, last};
        if (int rc = launch_step("multiscale", c, height, width, 1 << j, next, nullptr, out, p, APGPU_STARLET_FORM_AUTO, as_stream(stream))) return rc;
        c = next;
    }
    return APGPU_OK;
}
