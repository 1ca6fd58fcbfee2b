// continuum.hip - F11: narrow-band continuum subtraction on gfx950: the normalised Gaussian blur that matches the two PSFs, the six
// moments behind the straight-line fit N' = s C' + b, and the fused subtraction.
//
// The reference lists the stage as "Not yet" (doc/iTelescope_processing.md), so the arithmetic is this project's own definition
// (DESIGN 4.3h), restated in tests/continuum_model.py.  No contraction anywhere: every multiply and add rounds on its own.
//
//   blur     taps w[0 .. 2R] float64, R <= 32.  valid(y, x) = inside the image and finite.
//            row pass     a(y, x) = sum_k w[k] v(y, x + k - R), m(y, x) = sum_k w[k], both over the valid taps, k ascending, float64,
//                         accumulators starting at +0
//            column pass  A(y, x) = sum_k w[k] a(y + k - R, x), M(y, x) = sum_k w[k] m(y + k - R, x) over the rows inside the image
//            out          float32(A / M) where valid(y, x) and M >= min_weight, NaN elsewhere
//   moments  over the pixels with n, c finite, mask == 0 and lo <= r <= hi, r = double(n) - (s double(c) + b):
//            count, sum c, sum n, sum c c, sum c n, sum n n in float64, in an order that depends on n_pixels alone
//   combine  out = (float32(ca x) + float32(cb y)) + c0 in float32, NaN where x or y is not finite
//
// The blur kernel: a workgroup of 256 lanes owns a tile of kTileH = 32 rows x kTileW = 64 columns.  It stages the tile and a halo of
// R on every side in LDS as float32 (out-of-image pixels as NaN, so "inside and finite" is one test), origin rounded down to a
// multiple of four columns so that 16-byte loads serve whenever the image rows are 16-byte aligned.  The row pass then writes
// (a, m) as one 16-byte pair per element for the 32 + 2 R rows, a wavefront per row and a lane per column (consecutive lanes read
// consecutive floats and write consecutive pairs: no bank conflicts), and the column pass reads those pairs back (ds_read_b128, lanes
// consecutive) and writes the image.  The kernel is instantiated for R <= 4, 8, 16 and 32: the LDS of an instance is
// (32 + 2 RMAX) (68 + 2 RMAX) 4 + (32 + 2 RMAX) 64 16 bytes, 149 KiB of the 160 KiB of a CU for RMAX = 32 and 52 KiB for RMAX = 4.
#include "common.h"
#include "np_exact.h"
#include "plane_tile.h"

namespace apgpu {
namespace {

constexpr int kBlock = 256;
constexpr int kTileW = APGPU_BLUR_TILE_W, kTileH = APGPU_BLUR_TILE_H;
constexpr int kMaxR = APGPU_BLUR_MAX_RADIUS;
static_assert(kTileW == kWave, "a wavefront owns one tile row");

struct BlurTaps {
    double w[2 * kMaxR + 1];
};

template <int RMAX>
__global__ __launch_bounds__(kBlock) void gauss_blur_kernel(const float *__restrict__ data, long long H, long long W, const BlurTaps taps, int R,
                                                           double min_weight, int wide, float *__restrict__ out)
{
    constexpr int kInH = kTileH + 2 * RMAX;
    constexpr int kInW = halo_pitch(kTileW, RMAX);
    __shared__ __attribute__((aligned(16))) float tile[kInH][kInW];
    __shared__ __attribute__((aligned(16))) double2 am[kInH][kTileW];
    __shared__ double wt[2 * RMAX + 1];
    const long long tx0 = (long long)blockIdx.x * kTileW, ty0 = (long long)blockIdx.y * kTileH;
    const int rows = kTileH + 2 * R;                        // staged rows: image rows ty0 - R .. ty0 + kTileH + R - 1
    const float nanv = quiet_nan();

    if (threadIdx.x <= 2 * R) wt[threadIdx.x] = taps.w[threadIdx.x];
    const int off = stage_halo<kInW, kBlock>(tile, data, H, W, tx0, ty0, kTileW, R, rows, wide);
    __syncthreads();

    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const bool col_in = tx0 + lane < W;
    // row pass: wavefront -> staged row, lane -> tile column
    for (int lr = wave; lr < rows; lr += kBlock / kWave) {
        const long long gy = ty0 - R + lr;
        double a = 0.0, m = 0.0;
        if (gy >= 0 && gy < H && col_in) {
            const float *p = &tile[lr][off + lane];
            for (int k = 0; k <= 2 * R; k++) row_add(a, m, p[k], wt[k]);
        }
        am[lr][lane] = make_double2(a, m);
    }
    __syncthreads();

    // column pass: wavefront -> tile row, lane -> tile column.  Rows outside the image hold (0, 0): adding w 0 = +0 leaves an
    // accumulator (never -0) unchanged, as skipping the tap does.
    if (!col_in) return;
    for (int ly = wave; ly < kTileH; ly += kBlock / kWave) {
        const long long gy = ty0 + ly;
        if (gy >= H) break;
        double A = 0.0, M = 0.0;
        for (int k = 0; k <= 2 * R; k++) {
            const double2 q = am[ly + k][lane];
            const double w = wt[k];
            A = A + w * q.x;
            M = M + w * q.y;
        }
        const float c = tile[ly + R][off + R + lane];
        const bool ok = is_finite(c) && M >= min_weight;
        out[(size_t)gy * (size_t)W + (size_t)(tx0 + lane)] = ok ? (float)(A / M) : nanv;
    }
}

// ---- the six moments ---------------------------------------------------------------------------------------------------------
constexpr int kMaxMomentBlocks = 1024;
constexpr int kMomentHeader = 64;                           // bytes: the int32 ticket of the last-block reduction

struct Moments {
    unsigned long long n;
    double c, y, cc, cy, yy;
};

__device__ __forceinline__ void moments_add(Moments &t, float nv, float cv, unsigned mk, double s, double b, double lo, double hi)
{
    if (mk != 0 || !is_finite(nv) || !is_finite(cv)) return;
    const double y = (double)nv, c = (double)cv;
    const double r = y - (s * c + b);
    if (!(r >= lo && r <= hi)) return;
    t.n += 1;
    t.c = t.c + c;
    t.y = t.y + y;
    t.cc = t.cc + c * c;
    t.cy = t.cy + c * y;
    t.yy = t.yy + y * y;
}

// Sums the 256 records of a workgroup in LDS, lane 0 of the block ends with the total: a binary tree in a fixed order.
__device__ __forceinline__ void block_reduce(Moments &t, unsigned long long (&sn)[kBlock], double (&sd)[5][kBlock])
{
    const int i = threadIdx.x;
    sn[i] = t.n;
    sd[0][i] = t.c; sd[1][i] = t.y; sd[2][i] = t.cc; sd[3][i] = t.cy; sd[4][i] = t.yy;
    __syncthreads();
    for (int step = kBlock / 2; step > 0; step >>= 1) {
        if (i < step) {
            sn[i] += sn[i + step];
            for (int q = 0; q < 5; q++) sd[q][i] = sd[q][i] + sd[q][i + step];
        }
        __syncthreads();
    }
    t.n = sn[0];
    t.c = sd[0][0]; t.y = sd[1][0]; t.cc = sd[2][0]; t.cy = sd[3][0]; t.yy = sd[4][0];
}

// Lane t of block b owns the quads (b 256 + t) + j gridDim 256, j = 0, 1, ..., a quad being four consecutive pixels: the
// assignment and so the order of every sum depends on n_pixels alone, not on the alignment that decides how a quad is loaded.
__global__ __launch_bounds__(kBlock) void pair_moments_kernel(const float *__restrict__ nimg, const float *__restrict__ cimg,
                                                             const uint8_t *__restrict__ mask, long long npix, double s, double b, double lo,
                                                             double hi, int wide, int wide_mask, double *__restrict__ partial,
                                                             int *__restrict__ ticket, double *__restrict__ out6)
{
    __shared__ unsigned long long sn[kBlock];
    __shared__ double sd[5][kBlock];
    __shared__ int last;
    Moments t = {0ull, 0.0, 0.0, 0.0, 0.0, 0.0};
    const long long nquads = (npix + 3) >> 2;
    const long long step = (long long)gridDim.x * kBlock;
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < nquads; q += step) {
        const long long p = q << 2;
        float nv[4], cv[4];
        unsigned mk[4] = {0u, 0u, 0u, 0u};
        const int cnt = (int)(npix - p < 4 ? npix - p : 4);
        if (cnt == 4 && wide) {
            const float4 a = *reinterpret_cast<const float4 *>(nimg + p), c = *reinterpret_cast<const float4 *>(cimg + p);
            nv[0] = a.x; nv[1] = a.y; nv[2] = a.z; nv[3] = a.w;
            cv[0] = c.x; cv[1] = c.y; cv[2] = c.z; cv[3] = c.w;
        } else {
            for (int j = 0; j < 4; j++) {
                nv[j] = j < cnt ? nimg[p + j] : 0.0f;
                cv[j] = j < cnt ? cimg[p + j] : 0.0f;
            }
        }
        if (mask) {
            if (cnt == 4 && wide_mask) {
                const unsigned w = *reinterpret_cast<const unsigned *>(mask + p);
                mk[0] = w & 0xffu; mk[1] = (w >> 8) & 0xffu; mk[2] = (w >> 16) & 0xffu; mk[3] = w >> 24;
            } else {
                for (int j = 0; j < cnt; j++) mk[j] = mask[p + j];
            }
        }
        for (int j = 0; j < 4; j++)
            if (j < cnt) moments_add(t, nv[j], cv[j], mk[j], s, b, lo, hi);
    }
    block_reduce(t, sn, sd);
    if (threadIdx.x == 0) {
        double *rec = partial + 6 * (size_t)blockIdx.x;
        rec[0] = __longlong_as_double((long long)t.n);
        rec[1] = t.c; rec[2] = t.y; rec[3] = t.cc; rec[4] = t.cy; rec[5] = t.yy;
        __threadfence();
        last = atomicAdd(ticket, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    // the last workgroup to finish: the partial records in index order, lane t the records t, t + 256, ..., then the same tree
    __threadfence();
    Moments u = {0ull, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g = threadIdx.x; g < (int)gridDim.x; g += kBlock) {
        const volatile double *rec = partial + 6 * (size_t)g;
        u.n += (unsigned long long)__double_as_longlong(rec[0]);
        u.c = u.c + rec[1]; u.y = u.y + rec[2]; u.cc = u.cc + rec[3]; u.cy = u.cy + rec[4]; u.yy = u.yy + rec[5];
    }
    block_reduce(u, sn, sd);
    if (threadIdx.x == 0) {
        out6[0] = (double)u.n;
        out6[1] = u.c; out6[2] = u.y; out6[3] = u.cc; out6[4] = u.cy; out6[5] = u.yy;
        *ticket = 0;
    }
}

// ---- the subtraction ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float combine1(float x, float y, bool has_y, float ca, float cb, float c0)
{
    if (!is_finite(x) || (has_y && !is_finite(y))) return quiet_nan();
    float v = ca * x;
    if (has_y) v = v + cb * y;
    return v + c0;
}

// (no __restrict__: out may be x or y; every lane reads its own elements before it writes them)
__global__ __launch_bounds__(kBlock) void linear_combine_kernel(const float *x, const float *y, float ca, float cb, float c0, float *out,
                                                               long long npix, int wide)
{
    const long long nquads = (npix + 3) >> 2;
    const long long step = (long long)gridDim.x * kBlock;
    const bool has_y = y != nullptr;
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < nquads; q += step) {
        const long long p = q << 2;
        if (wide && npix - p >= 4) {
            const float4 a = *reinterpret_cast<const float4 *>(x + p);
            const float4 c = has_y ? *reinterpret_cast<const float4 *>(y + p) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            *reinterpret_cast<float4 *>(out + p) = make_float4(combine1(a.x, c.x, has_y, ca, cb, c0), combine1(a.y, c.y, has_y, ca, cb, c0),
                                                               combine1(a.z, c.z, has_y, ca, cb, c0), combine1(a.w, c.w, has_y, ca, cb, c0));
        } else {
            for (long long j = p; j < p + 4 && j < npix; j++) out[j] = combine1(x[j], has_y ? y[j] : 0.0f, has_y, ca, cb, c0);
        }
    }
}

inline long long moment_blocks(long long npix)
{
    const long long b = (((npix + 3) >> 2) + kBlock - 1) / kBlock;
    return b < 1 ? 1 : (b > kMaxMomentBlocks ? kMaxMomentBlocks : b);
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_gauss_blur_norm_f32(const float *data, int64_t height, int64_t width, const double *taps_host, int32_t radius,
                                         double min_weight, float *out, void *stream)
{
    if (!data || !out || !taps_host) return fail(APGPU_EINVAL, "gauss_blur_norm: NULL pointer argument");
    if (height <= 0 || width <= 0) return fail(APGPU_EINVAL, "gauss_blur_norm: image of %lld x %lld", (long long)height, (long long)width);
    if (radius < 0) return fail(APGPU_EINVAL, "gauss_blur_norm: radius %d", radius);
    if (radius > kMaxR) return fail(APGPU_EUNSUPPORTED, "gauss_blur_norm: radius %d, the kernel holds %d", radius, kMaxR);
    if (!(min_weight >= 0.0)) return fail(APGPU_EINVAL, "gauss_blur_norm: min_weight %g", min_weight);
    if (data == out) return fail(APGPU_EINVAL, "gauss_blur_norm: out must not be the input");
    if (!aligned(data, 4) || !aligned(out, 4)) return fail(APGPU_EINVAL, "gauss_blur_norm: data and out must be 4-byte aligned");
    dim3 grid;
    if (int rc = tile_grid("gauss_blur_norm", height, width, kTileH, kTileW, &grid)) return rc;
    BlurTaps t;
    for (int k = 0; k < 2 * kMaxR + 1; k++) t.w[k] = k <= 2 * radius ? taps_host[k] : 0.0;
    const int wide = wide_rows(width, data);
    hipStream_t s = as_stream(stream);
    const long long H = height, W = width;
    if (radius <= 4) hipLaunchKernelGGL((gauss_blur_kernel<4>), grid, dim3(kBlock), 0, s, data, H, W, t, (int)radius, min_weight, wide, out);
    else if (radius <= 8) hipLaunchKernelGGL((gauss_blur_kernel<8>), grid, dim3(kBlock), 0, s, data, H, W, t, (int)radius, min_weight, wide, out);
    else if (radius <= 16) hipLaunchKernelGGL((gauss_blur_kernel<16>), grid, dim3(kBlock), 0, s, data, H, W, t, (int)radius, min_weight, wide, out);
    else hipLaunchKernelGGL((gauss_blur_kernel<32>), grid, dim3(kBlock), 0, s, data, H, W, t, (int)radius, min_weight, wide, out);
    return check_launch("gauss_blur_norm");
}

extern "C" size_t apgpu_pair_moments_ws_bytes(int64_t n_pixels)
{
    return n_pixels > 0 ? (size_t)kMomentHeader + (size_t)moment_blocks(n_pixels) * 6 * sizeof(double) : 0;
}

extern "C" int apgpu_pair_moments_f64(const float *n_img, const float *c_img, const uint8_t *mask, int64_t n_pixels, double s, double b,
                                      double lo, double hi, double *out6, void *ws, size_t ws_bytes, void *stream)
{
    if (!n_img || !c_img || !out6 || !ws) return fail(APGPU_EINVAL, "pair_moments: NULL pointer argument");
    if (n_pixels <= 0) return fail(APGPU_EINVAL, "pair_moments: %lld pixels", (long long)n_pixels);
    if (!aligned(n_img, 4) || !aligned(c_img, 4) || !aligned(out6, 8) || !aligned(ws, 8))
        return fail(APGPU_EINVAL, "pair_moments: the images must be 4-byte aligned, out6 and ws 8-byte aligned");
    if (ws_bytes < apgpu_pair_moments_ws_bytes(n_pixels))
        return fail(APGPU_EWORKSPACE, "pair_moments: workspace of %zu bytes, %zu needed", ws_bytes, apgpu_pair_moments_ws_bytes(n_pixels));
    if (lo != lo || hi != hi || s != s || b != b) return fail(APGPU_EINVAL, "pair_moments: s, b, lo and hi must not be NaN");
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(ws, 0, kMomentHeader, st) != hipSuccess) return fail(APGPU_ELAUNCH, "pair_moments: hipMemsetAsync failed");
    const int wide = aligned(n_img, 16) && aligned(c_img, 16), wide_mask = mask && aligned(mask, 4);
    double *partial = reinterpret_cast<double *>(static_cast<char *>(ws) + kMomentHeader);
    hipLaunchKernelGGL(pair_moments_kernel, dim3((unsigned)moment_blocks(n_pixels)), dim3(kBlock), 0, st, n_img, c_img, mask, (long long)n_pixels,
                       s, b, lo, hi, wide, wide_mask, partial, static_cast<int *>(ws), out6);
    return check_launch("pair_moments");
}

extern "C" int apgpu_linear_combine_f32(const float *x, const float *y, float ca, float cb, float c0, float *out, int64_t n_pixels, void *stream)
{
    if (!x || !out) return fail(APGPU_EINVAL, "linear_combine: NULL pointer argument");
    if (n_pixels <= 0) return fail(APGPU_EINVAL, "linear_combine: %lld pixels", (long long)n_pixels);
    if (!aligned(x, 4) || !aligned(out, 4) || (y && !aligned(y, 4))) return fail(APGPU_EINVAL, "linear_combine: x, y and out must be 4-byte aligned");
    const int wide = aligned(x, 16) && aligned(out, 16) && (!y || aligned(y, 16));
    long long blocks = (((n_pixels + 3) >> 2) + kBlock - 1) / kBlock;
    blocks = blocks > 16LL * kNumCU ? 16LL * kNumCU : blocks;
    hipLaunchKernelGGL(linear_combine_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), x, y, ca, cb, c0, out, (long long)n_pixels, wide);
    return check_launch("linear_combine");
}
