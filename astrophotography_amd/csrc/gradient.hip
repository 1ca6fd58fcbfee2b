// gradient.hip - F20: removal of the large-scale sky gradient of a co-add on gfx950 (the rule: include/apgpu.h F20,
// restated in tests/gradient_model.py).  The reference has no such stage, so the arithmetic is this project's own definition.  No
// contraction anywhere: every multiply and add rounds on its own.
//
//   samples  the sigma-clipped median / std of square boxes about a list of centres: box_stats.h's kernel with its origin taken
//            from the list, one workgroup per sample, the box (at most 65 x 65 values) staged in LDS once; the std of the final
//            survivors summed in the box's row-major order, as numpy does, so that all four outputs equal the oracle's bits
//   lattice  the fitted surface (a polynomial, or a thin-plate spline of up to 4096 centres) at the nodes of a coarse lattice, in
//            float64: a lane per node, the centres and weights staged in LDS (every lane reads the same one: a broadcast), the K
//            terms added in index order - the same bits on every run
//   apply    the Keys cubic-convolution interpolant (a = -1/2, x first and then y, float64) of the lattice at every pixel, subtracted
//            from or divided into the float32 image in the same pass; optionally the surface itself as a second float32 plane
//
// The apply kernel: a workgroup of 256 lanes owns a tile of kTileH = 32 rows x kTileW = 128 columns and stages the lattice nodes under
// it in LDS (at most 13 x 37 float64).  A lane owns four consecutive columns - their sixteen column weights are formed once - and
// the rows ly, ly + 8, ly + 16, ly + 24 of the tile, forming the four row weights once per row.  With 16-byte aligned planes and
// W % 4 == 0 a lane's four pixels are one 16-byte load and one (or two) 16-byte stores.  8 bytes of memory traffic per pixel, 12 with
// the surface plane, sixteen 8-byte LDS reads and about 50 float64 operations.  Measured on a 4096 x 4096 image it runs at 40 % of the
// rate of a device copy: not bound by memory (by the count it is the LDS reads and the float64 arithmetic, no counters taken).
#include "box_stats.h"
#include "common.h"
#include "np_exact.h"

namespace apgpu {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxSamples = APGPU_GRADIENT_MAX_SAMPLES, kMaxRadius = APGPU_GRADIENT_MAX_RADIUS;
constexpr int kMinStep = APGPU_GRADIENT_MIN_STEP, kMaxStep = APGPU_GRADIENT_MAX_STEP;
constexpr int kMaxDegree = APGPU_GRADIENT_MAX_DEGREE;
constexpr int kTileH = APGPU_GRADIENT_TILE_H, kTileW = APGPU_GRADIENT_TILE_W;

// ---- the lattice ------------------------------------------------------------------------------------------------------------------
constexpr int kChunk = 512;                                 // centres staged per trip: 3 x 512 float64 = 12 KiB

// phi(q) = r^2 log r with q = r^2: 0 at q = 0
__device__ __forceinline__ double tps_phi(double q) { return q == 0.0 ? 0.0 : 0.5 * q * log(q); }

// S = ((sum_k w_k phi(q_k) + a0) + a1 u) + a2 v, the sum from +0 in index order.  params = a0, a1, a2, w_0 .. w_{K-1}; uv = u_k, v_k.
__global__ __launch_bounds__(kWave) void lattice_tps_kernel(const double *__restrict__ params, const double *__restrict__ uv, int K, double x0,
                                                           double y0, double L, int s, int ny, int nx, double *__restrict__ out)
{
    __shared__ double su[kChunk], sv[kChunk], sw[kChunk];
    const int node = blockIdx.x * kWave + threadIdx.x;
    const bool live = node < ny * nx;
    const int iy = live ? node / nx : 0, ix = live ? node - iy * nx : 0;
    const double u = ((double)((ix - 1) * s) - x0) / L, v = ((double)((iy - 1) * s) - y0) / L;
    double acc = 0.0;
    for (int k0 = 0; k0 < K; k0 += kChunk) {
        const int m = min(kChunk, K - k0);
        __syncthreads();
        for (int j = threadIdx.x; j < m; j += kWave) {
            su[j] = uv[2 * (size_t)(k0 + j)];
            sv[j] = uv[2 * (size_t)(k0 + j) + 1];
            sw[j] = params[3 + k0 + j];
        }
        __syncthreads();
        for (int j = 0; j < m; j++) {
            const double du = u - su[j], dv = v - sv[j];
            const double q = du * du + dv * dv;
            acc = acc + sw[j] * tps_phi(q);
        }
    }
    if (live) out[node] = ((acc + params[0]) + params[1] * u) + params[2] * v;
}

// S = sum over t = 0 .. degree, j = 0 .. t of c[t (t + 1) / 2 + j] (u^(t-j) v^j), from +0 in that order; the powers by repeated
// multiplication (u^i = u^(i-1) u).
__global__ __launch_bounds__(kWave) void lattice_poly_kernel(const double *__restrict__ coef, int degree, double x0, double y0, double L, int s,
                                                            int ny, int nx, double *__restrict__ out)
{
    const int node = blockIdx.x * kWave + threadIdx.x;
    if (node >= ny * nx) return;
    const int iy = node / nx, ix = node - iy * nx;
    const double u = ((double)((ix - 1) * s) - x0) / L, v = ((double)((iy - 1) * s) - y0) / L;
    double pu[kMaxDegree + 1], pv[kMaxDegree + 1];
    pu[0] = pv[0] = 1.0;
#pragma unroll
    for (int i = 1; i <= kMaxDegree; i++) {
        pu[i] = pu[i - 1] * u;
        pv[i] = pv[i - 1] * v;
    }
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t <= kMaxDegree; t++) {
        if (t > degree) break;
#pragma unroll
        for (int j = 0; j <= t; j++) acc = acc + coef[t * (t + 1) / 2 + j] * (pu[t - j] * pv[j]);
    }
    out[node] = acc;
}

// ---- the apply pass ---------------------------------------------------------------------------------------------------------------
constexpr int kNodeRows = kTileH / kMinStep + 5, kNodeCols = kTileW / kMinStep + 5;      // 13 x 37: the most nodes under one tile

// Keys' cubic convolution kernel, a = -1/2, at the four nodes about a point t in [0, 1) past the second of them
__device__ __forceinline__ void keys_weights(double t, double (&w)[4])
{
    w[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    w[1] = (1.5 * t - 2.5) * t * t + 1.0;
    w[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    w[3] = (0.5 * t - 0.5) * t * t;
}

__device__ __forceinline__ float apply1(float d, double S, int divide, double p)
{
    if (!is_finite(d)) return quiet_nan();
    if (!divide) return (float)(((double)d - S) + p);
    if (!(S > 0.0) || S == __builtin_inf()) return quiet_nan();
    return (float)(((double)d / S) * p);
}

// (no __restrict__ on data and out: out may be data; a lane reads its own pixels before it writes them)
__global__ __launch_bounds__(kBlock) void surface_apply_kernel(const float *data, const double *__restrict__ lattice, long long H, long long W,
                                                              int ny, int nx, int s, int divide, double p, int wide, float *out,
                                                              float *__restrict__ surface)
{
    __shared__ double node[kNodeRows][kNodeCols];
    const long long tx0 = (long long)blockIdx.x * kTileW, ty0 = (long long)blockIdx.y * kTileH;
    const int jx0 = (int)(tx0 / s), jy0 = (int)(ty0 / s);     // the first node column / row under the tile
    const long long txl = min(tx0 + kTileW, W) - 1, tyl = min(ty0 + kTileH, H) - 1;
    const int ncols = (int)(txl / s) - jx0 + 4, nrows = (int)(tyl / s) - jy0 + 4;
    for (int idx = threadIdx.x; idx < nrows * ncols; idx += kBlock) {
        const int r = idx / ncols, c = idx - r * ncols;
        node[r][c] = (jy0 + r < ny && jx0 + c < nx) ? lattice[(size_t)(jy0 + r) * nx + (jx0 + c)] : 0.0;
    }
    __syncthreads();

    const int quad = threadIdx.x % (kTileW / 4), ly0 = threadIdx.x / (kTileW / 4);
    const long long gx = tx0 + 4 * quad;
    if (gx >= W) return;
    const int cnt = (int)(W - gx < 4 ? W - gx : 4);
    double wx[4][4];
    int cx[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const long long x = gx + (j < cnt ? j : 0);
        const int ix = (int)(x / s);
        cx[j] = ix - jx0;
        keys_weights((double)(int)(x - (long long)ix * s) / (double)s, wx[j]);
    }
    for (int ly = ly0; ly < kTileH; ly += kBlock / (kTileW / 4)) {
        const long long gy = ty0 + ly;
        if (gy >= H) break;
        const int iy = (int)(gy / s), cy = iy - jy0;
        double wy[4];
        keys_weights((double)(int)(gy - (long long)iy * s) / (double)s, wy);
        const size_t base = (size_t)gy * (size_t)W + (size_t)gx;
        float d[4];
        if (wide) {
            const float4 q = *reinterpret_cast<const float4 *>(data + base);
            d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) d[j] = j < cnt ? data[base + j] : 0.0f;
        }
        float o[4], sf[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double rowv[4];
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const double *n = &node[cy + a][cx[j]];
                rowv[a] = ((wx[j][0] * n[0] + wx[j][1] * n[1]) + wx[j][2] * n[2]) + wx[j][3] * n[3];
            }
            const double S = ((wy[0] * rowv[0] + wy[1] * rowv[1]) + wy[2] * rowv[2]) + wy[3] * rowv[3];
            o[j] = apply1(d[j], S, divide, p);
            sf[j] = (float)S;
        }
        if (wide) {
            *reinterpret_cast<float4 *>(out + base) = make_float4(o[0], o[1], o[2], o[3]);
            if (surface) *reinterpret_cast<float4 *>(surface + base) = make_float4(sf[0], sf[1], sf[2], sf[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (j < cnt) {
                    out[base + j] = o[j];
                    if (surface) surface[base + j] = sf[j];
                }
            }
        }
    }
}

inline int lattice_nodes(int64_t n, int s) { return (int)((n - 1) / s) + 4; }

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_sample_clipped_stats_f32(const float *data, const uint8_t *mask, int64_t height, int64_t width, const int32_t *centres,
                                              int32_t n_samples, int32_t radius, double sigma, int32_t maxiters, double *stats_out, void *stream)
{
    if (int rc = check_plane("sample_clipped_stats", data, height, width)) return rc;
    if (height > (1 << 30) || width > (1 << 30)) return fail(APGPU_EUNSUPPORTED, "sample_clipped_stats: image of %lld x %lld", (long long)height, (long long)width);
    if (n_samples < 0 || n_samples > kMaxSamples) return fail(APGPU_EINVAL, "sample_clipped_stats: %d samples, at most %d", n_samples, kMaxSamples);
    if (radius < 0 || radius > kMaxRadius) return fail(APGPU_EINVAL, "sample_clipped_stats: radius %d, at most %d", radius, kMaxRadius);
    if (!(sigma >= 0.0) || maxiters < 0) return fail(APGPU_EINVAL, "sample_clipped_stats: bad clip parameters");
    if (n_samples == 0) return APGPU_OK;
    if (!centres || !stats_out) return fail(APGPU_EINVAL, "sample_clipped_stats: NULL pointer argument");
    if (!aligned(centres, 4) || !aligned(stats_out, 8)) return fail(APGPU_EINVAL, "sample_clipped_stats: centres must be 4-byte, stats_out 8-byte aligned");
    if (maxiters == 0) maxiters = 0x7fffffff;               // SigmaClip stores `maxiters or np.inf`: 0 clips until nothing changes
    const int side = 2 * radius + 1;
    const ListOrigin origin = {centres, radius};
    hipLaunchKernelGGL((box_stats_kernel<256, true, ListOrigin>), dim3((unsigned)n_samples), dim3(256), (size_t)side * side * sizeof(float),
                       as_stream(stream), data, mask, (int)height, (int)width, side, side, origin, sigma, maxiters, stats_out);
    return check_launch("sample_clipped_stats");
}

extern "C" int apgpu_surface_lattice_f64(int32_t model, const double *params, const double *centres_uv, int32_t n_terms, double x0, double y0,
                                         double half_size, int32_t step, int32_t ny, int32_t nx, double *lattice_out, void *stream)
{
    if (!params || !lattice_out) return fail(APGPU_EINVAL, "surface_lattice: NULL pointer argument");
    if (!aligned(params, 8) || !aligned(lattice_out, 8) || !aligned(centres_uv, 8)) return fail(APGPU_EINVAL, "surface_lattice: the arrays must be 8-byte aligned");
    if (step < kMinStep || step > kMaxStep) return fail(APGPU_EINVAL, "surface_lattice: step %d outside %d .. %d", step, kMinStep, kMaxStep);
    if (ny < 4 || nx < 4 || (int64_t)ny * nx > (1 << 26)) return fail(APGPU_EINVAL, "surface_lattice: lattice of %d x %d nodes", ny, nx);
    if (!(half_size > 0.0) || half_size == __builtin_inf() || x0 != x0 || y0 != y0) return fail(APGPU_EINVAL, "surface_lattice: bad normalisation");
    const dim3 grid((unsigned)(((int64_t)ny * nx + kWave - 1) / kWave));
    if (model == APGPU_SURFACE_POLY) {
        if (n_terms < 1 || n_terms > kMaxDegree) return fail(APGPU_EINVAL, "surface_lattice: degree %d outside 1 .. %d", n_terms, kMaxDegree);
        hipLaunchKernelGGL(lattice_poly_kernel, grid, dim3(kWave), 0, as_stream(stream), params, (int)n_terms, x0, y0, half_size, (int)step, (int)ny,
                           (int)nx, lattice_out);
    } else if (model == APGPU_SURFACE_TPS) {
        if (n_terms < 0 || n_terms > kMaxSamples) return fail(APGPU_EINVAL, "surface_lattice: %d centres, at most %d", n_terms, kMaxSamples);
        if (n_terms > 0 && !centres_uv) return fail(APGPU_EINVAL, "surface_lattice: NULL pointer argument");
        hipLaunchKernelGGL(lattice_tps_kernel, grid, dim3(kWave), 0, as_stream(stream), params, centres_uv, (int)n_terms, x0, y0, half_size, (int)step,
                           (int)ny, (int)nx, lattice_out);
    } else {
        return fail(APGPU_EINVAL, "surface_lattice: unknown model %d", model);
    }
    return check_launch("surface_lattice");
}

extern "C" int apgpu_surface_apply_f32(const float *data, const double *lattice, int64_t height, int64_t width, int32_t ny, int32_t nx,
                                       int32_t step, int32_t mode, double pedestal, float *out, float *surface_out, void *stream)
{
    if (int rc = check_plane("surface_apply", data, height, width)) return rc;
    if (!lattice || !out) return fail(APGPU_EINVAL, "surface_apply: NULL pointer argument");
    if (!aligned(out, 4) || !aligned(surface_out, 4) || !aligned(lattice, 8))
        return fail(APGPU_EINVAL, "surface_apply: the planes must be 4-byte aligned, the lattice 8-byte aligned");
    if (step < kMinStep || step > kMaxStep) return fail(APGPU_EINVAL, "surface_apply: step %d outside %d .. %d", step, kMinStep, kMaxStep);
    if (ny != lattice_nodes(height, step) || nx != lattice_nodes(width, step))
        return fail(APGPU_EINVAL, "surface_apply: lattice of %d x %d nodes, an image of %lld x %lld at step %d has %d x %d", ny, nx, (long long)height,
                    (long long)width, step, lattice_nodes(height, step), lattice_nodes(width, step));
    if (mode != APGPU_GRADIENT_SUBTRACT && mode != APGPU_GRADIENT_DIVIDE) return fail(APGPU_EINVAL, "surface_apply: unknown mode %d", mode);
    if (pedestal != pedestal) return fail(APGPU_EINVAL, "surface_apply: the pedestal must not be NaN");
    if (surface_out && (surface_out == out || surface_out == data)) return fail(APGPU_EINVAL, "surface_apply: surface_out must be a plane of its own");
    dim3 grid;
    if (int rc = tile_grid("surface_apply", height, width, kTileH, kTileW, &grid)) return rc;
    const int wide = surface_out ? wide_rows(width, data, out, surface_out) : wide_rows(width, data, out);
    hipLaunchKernelGGL(surface_apply_kernel, grid, dim3(kBlock), 0, as_stream(stream), data, lattice, (long long)height, (long long)width, (int)ny, (int)nx,
                       (int)step, (int)(mode == APGPU_GRADIENT_DIVIDE), pedestal, wide, out, surface_out);
    return check_launch("surface_apply");
}
