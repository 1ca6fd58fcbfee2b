// subtract.hip - F23: optimal image subtraction (Alard & Lupton 1998, Alard 2000) on gfx950: the per-stamp normal equations of the
// kernel fit and the application of the fitted, spatially varying kernel.
//
// The reference has no such stage, so the arithmetic is this project's own definition, restated in
// tests/subtract_model.py.  No contraction anywhere: every multiply and add rounds on its own.
//
//   stamps   per stamp s (centre cx, cy; half-size h; n = 2 h + 1), all float64, every accumulator starting at +0:
//              R_f(x, y') = sum_{u = -r .. r} filters[f][u + r] T(x - u, y')                     (u ascending)
//              c_n(x, y)  = sum_{v = -r .. r} filters[col[n]][v + r] R_{row[n]}(x, y - v)        (v ascending)
//              V_n = scale[n] c_n, minus V_0 where even[n] and n > 0;  V_Nb = 1;  V_{Nb+1} = I
//              gram[a][b] = gram[b][a] = sum over the stamp's pixels, row-major, of (w V_a) V_b  (a <= b)
//            status bits: 1 the footprint h + r leaves the image, else 2 a non-finite template pixel in the footprint, 4 a
//            non-finite image pixel in the stamp, 8 a non-zero mask pixel in the stamp; a refused stamp has zeros and count 0.
//   apply    conv_t(x, y) = sum_u sum_v A_t[v + r][u + r] S(x - u, y - v) in float32, u ascending outside, v ascending inside, S with
//            its non-finite and out-of-image pixels as NaN; conv = sum_t float32(phi_t) conv_t (t ascending, from +0);
//            B = float32(sum_t c_t phi_t); matched = conv + B; diff = (O - conv) - B, or ((conv + B) - O) / a0 with
//            APGPU_SUBTRACT_CONVOLVED_IMAGE; NaN where O is not finite; every NaN written is the quiet NaN 0x7fc00000.
//
// The stamps kernel: one workgroup of 256 lanes per stamp.  The footprint (at most 61 x 61 float32) is staged in LDS once; the
// stamp is then walked one row at a time: for each 1-D filter the 2 r + 1 row-filtered lines that the row needs, then the column
// filter of every basis function on that filter, so that the row's Nb + 2 vectors (at most 66 x 31 float64) are complete in LDS
// and every pair (a, b) adds its row to its own accumulator in LDS - one lane owns a pair for the whole stamp, so the order of
// every sum is fixed and no atomic is involved.  Row-filtered lines are computed again for every stamp row (2 r + 1 times the
// arithmetic of a rolling buffer): the buffer for all filters, 15 x 31 x 31 float64 at the defaults and four times that at the
// limits, does not fit beside the vectors; DESIGN 4.3o has the count.
//
// The apply kernel: a workgroup of 256 lanes owns a tile of 32 rows x 64 columns and stages it with a halo of r in LDS
// (plane_tile.h).  A wavefront owns 8 rows, a lane a column of 8 pixels: for each kernel column u it keeps the 8 template values of
// its pixels in registers and slides them down the kernel's rows (one 4-byte LDS read per tap, consecutive lanes on consecutive
// banks), and every value feeds the NT accumulators of each of the 8 pixels: 2 NT 8 float32 operations per LDS read.  The kernel
// values are the same for every lane: scalar loads.  Instantiated for NT = 1, 3, 6, 10 (kernel degree 0 .. 3).
#include "common.h"
#include "np_exact.h"
#include "plane_tile.h"
#include "subtract_core.h"

namespace apgpu {
namespace {

constexpr int kBlock = 256;
static_assert(kSubMaxRadius == APGPU_SUBTRACT_MAX_RADIUS && kSubMaxBasis == APGPU_SUBTRACT_MAX_BASIS &&
              kSubMaxDegree == APGPU_SUBTRACT_MAX_DEGREE, "subtract_core.h and apgpu.h state the same limits");

// ---- stamps -------------------------------------------------------------------------------------------------------------------
constexpr int kMaxHalf = APGPU_SUBTRACT_MAX_HALF;
constexpr int kMaxN = 2 * kMaxHalf + 1;                              // stamp side
constexpr int kMaxKw = 2 * kSubMaxRadius + 1;                        // kernel side
constexpr int kMaxFoot = 2 * (kMaxHalf + kSubMaxRadius) + 1;         // footprint side
constexpr int kMaxVec = kSubMaxBasis + 2;
constexpr int kMaxPairs = kMaxVec * (kMaxVec + 1) / 2;

struct StampBasis {
    double scale[kSubMaxBasis];
    uint8_t row[kSubMaxBasis], col[kSubMaxBasis], even[kSubMaxBasis];
    int nb, nf;
};

__global__ __launch_bounds__(kBlock) void subtract_stamps_kernel(const float *__restrict__ tmpl, const float *__restrict__ img,
                                                                const uint8_t *__restrict__ mask, long long H, long long W,
                                                                const int32_t *__restrict__ centers, int h, int r,
                                                                const double *__restrict__ filters, const StampBasis basis, double var0,
                                                                double gain, double *__restrict__ gram, int32_t *__restrict__ status,
                                                                int32_t *__restrict__ count)
{
    __shared__ float foot[kMaxFoot * kMaxFoot];
    __shared__ double rf[kMaxKw][kMaxN];
    __shared__ double vec[kMaxVec][kMaxN];
    __shared__ double wrow[kMaxN];
    __shared__ double acc[kMaxPairs];
    __shared__ double bscale[kSubMaxBasis];
    __shared__ uint8_t brow[kSubMaxBasis], bcol[kSubMaxBasis], beven[kSubMaxBasis];
    __shared__ uint8_t pair_a[kMaxPairs], pair_b[kMaxPairs];
    __shared__ int sbad;

    const int tid = threadIdx.x, s = blockIdx.x;
    const int n = 2 * h + 1, kw = 2 * r + 1, F = h + r, nfoot = 2 * F + 1;
    const int nb = basis.nb, nvec = nb + 2, npairs = nvec * (nvec + 1) / 2;
    const long long cx = centers[2LL * s], cy = centers[2LL * s + 1];
    double *out = gram + (size_t)s * (size_t)nvec * (size_t)nvec;

    const bool inside = cx - F >= 0 && cx + F < W && cy - F >= 0 && cy + F < H;      // (uniform)
    int bad = inside ? 0 : 1;
    if (tid == 0) sbad = bad;
    __syncthreads();
    if (inside) {
        for (int idx = tid; idx < nfoot * nfoot; idx += kBlock) {
            const int fy = idx / nfoot, fx = idx - fy * nfoot;
            const float v = tmpl[(size_t)(cy - F + fy) * (size_t)W + (size_t)(cx - F + fx)];
            foot[idx] = v;
            if (!is_finite(v)) bad |= 2;
        }
        for (int idx = tid; idx < n * n; idx += kBlock) {
            const int yy = idx / n, xx = idx - yy * n;
            const size_t p = (size_t)(cy - h + yy) * (size_t)W + (size_t)(cx - h + xx);
            const float v = img[p];
            if (!is_finite(v)) bad |= 4;
            if (mask && mask[p] != 0) bad |= 8;
        }
    }
    if (bad) atomicOr(&sbad, bad);                                   // (an integer OR: the result does not depend on the order)
    __syncthreads();
    bad = sbad;
    if (bad) {                                                       // (uniform) refused: zeros, count 0
        for (int idx = tid; idx < nvec * nvec; idx += kBlock) out[idx] = 0.0;
        if (tid == 0) {
            status[s] = bad;
            count[s] = 0;
        }
        return;
    }

    if (tid < nb) {
        bscale[tid] = basis.scale[tid];
        brow[tid] = basis.row[tid];
        bcol[tid] = basis.col[tid];
        beven[tid] = basis.even[tid];
    }
    for (int a = tid; a < nvec; a += kBlock) {                       // pair q of (a, b), a <= b: the rows of the upper triangle in order
        int q = a * nvec - a * (a - 1) / 2;
        for (int b = a; b < nvec; ++b, ++q) {
            pair_a[q] = (uint8_t)a;
            pair_b[q] = (uint8_t)b;
        }
    }
    for (int q = tid; q < npairs; q += kBlock) acc[q] = 0.0;
    __syncthreads();

    for (int yy = 0; yy < n; ++yy) {
        if (tid < n) {
            const double iv = (double)img[(size_t)(cy - h + yy) * (size_t)W + (size_t)(cx - h + tid)];
            vec[nb][tid] = 1.0;
            vec[nb + 1][tid] = iv;
            wrow[tid] = gain > 0.0 ? 1.0 / (var0 + (iv > 0.0 ? iv : 0.0) / gain) : 1.0;
        }
        for (int f = 0; f < basis.nf; ++f) {
            const double *fr = filters + (size_t)f * kw;
            // the row-filtered lines k = 0 .. 2 r: footprint rows yy + k
            for (int idx = tid; idx < kw * n; idx += kBlock) {
                const int k = idx / n, xx = idx - k * n;
                const float *src = foot + (yy + k) * nfoot + xx + r;
                double a = 0.0;
                for (int u = -r; u <= r; ++u) a = a + fr[u + r] * (double)src[-u];
                rf[k][xx] = a;
            }
            __syncthreads();
            for (int idx = tid; idx < nb * n; idx += kBlock) {
                const int nn = idx / n, xx = idx - nn * n;
                if (brow[nn] != f) continue;
                const double *fc = filters + (size_t)bcol[nn] * kw;
                double a = 0.0;
                for (int v = -r; v <= r; ++v) a = a + fc[v + r] * rf[r - v][xx];
                vec[nn][xx] = bscale[nn] * a;
            }
            __syncthreads();
        }
        for (int idx = n + tid; idx < nb * n; idx += kBlock) {       // (n + tid: function 0 stays)
            const int nn = idx / n, xx = idx - nn * n;
            if (beven[nn]) vec[nn][xx] = vec[nn][xx] - vec[0][xx];
        }
        __syncthreads();
        for (int q = tid; q < npairs; q += kBlock) {
            const double *va = vec[pair_a[q]], *vb = vec[pair_b[q]];
            double a = acc[q];
            for (int xx = 0; xx < n; ++xx) a = a + (wrow[xx] * va[xx]) * vb[xx];
            acc[q] = a;
        }
        __syncthreads();
    }
    for (int q = tid; q < npairs; q += kBlock) {
        const int a = pair_a[q], b = pair_b[q];
        out[a * nvec + b] = acc[q];
        out[b * nvec + a] = acc[q];
    }
    if (tid == 0) {
        status[s] = 0;
        count[s] = n * n;
    }
}

// ---- apply --------------------------------------------------------------------------------------------------------------------
constexpr int kTileW = APGPU_SUBTRACT_TILE_W, kTileH = APGPU_SUBTRACT_TILE_H;
constexpr int kPix = 8;                                              // pixels of a lane: a column of 8
static_assert(kTileW == kWave && kTileH == kPix * (kBlock / kWave), "a wavefront owns 8 rows of 64 columns");

struct SubBackground {
    double c[kSubMaxTerms];
    int deg;
};

template <int KDEG>
__global__ __launch_bounds__(kBlock) void subtract_apply_kernel(const float *__restrict__ src, const float *__restrict__ other, long long H,
                                                               long long W, const float *__restrict__ kern, int R, const SubBackground bg,
                                                               int convolved_image, float a0, int wide, float *__restrict__ diff,
                                                               float *__restrict__ matched)
{
    constexpr int NT = (KDEG + 1) * (KDEG + 2) / 2;
    constexpr int kInH = kTileH + 2 * kSubMaxRadius;
    constexpr int kInW = (halo_pitch(kTileW, kSubMaxRadius) + 3) & ~3;     // 100: stage_halo writes 16 bytes at a time, so every row starts on 16
    static_assert(kInW % 4 == 0 && kInW >= halo_pitch(kTileW, kSubMaxRadius), "16-byte aligned rows that hold the halo");
    __shared__ __attribute__((aligned(16))) float tile[kInH][kInW];
    const long long tx0 = (long long)blockIdx.x * kTileW, ty0 = (long long)blockIdx.y * kTileH;
    const int rows = kTileH + 2 * R, kw = 2 * R + 1;
    const float nanv = quiet_nan();

    const int off = stage_halo<kInW, kBlock>(tile, src, H, W, tx0, ty0, kTileW, R, rows, wide);
    __syncthreads();
    const int cols = (off + kTileW + 2 * R + 3) & ~3;                // the staged columns (stage_halo)
    for (int idx = threadIdx.x; idx < rows * cols; idx += kBlock) {  // +-inf count as no data
        const int lr = idx / cols, lc = idx - lr * cols;
        if (!is_finite(tile[lr][lc])) tile[lr][lc] = nanv;
    }
    __syncthreads();

    const int lane = threadIdx.x % kWave, ly0 = (threadIdx.x / kWave) * kPix;
    float acc[NT][kPix];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int p = 0; p < kPix; ++p) acc[t][p] = 0.0f;

    for (int u = -R; u <= R; ++u) {
        const int lc = off + R + lane - u;
        float w[kPix];
#pragma unroll
        for (int p = 0; p < kPix; ++p) w[p] = tile[ly0 + p + 2 * R][lc];     // tap v = -R: pixel row ly0 + p reads staged row ly0 + p + R - v
        for (int v = -R;; ++v) {
            const float *kp = kern + (v + R) * kw + (u + R);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float k = kp[t * kw * kw];
#pragma unroll
                for (int p = 0; p < kPix; ++p) acc[t][p] = acc[t][p] + k * w[p];
            }
            if (v == R) break;
#pragma unroll
            for (int p = kPix - 1; p > 0; --p) w[p] = w[p - 1];
            w[0] = tile[ly0 + R - v - 1][lc];
        }
    }

    const long long gx = tx0 + lane;
    if (gx >= W) return;
    const double X = subtract_norm_coord(gx, W);
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
        const long long gy = ty0 + ly0 + p;
        if (gy >= H) break;
        const double Y = subtract_norm_coord(gy, H);
        double phi[NT];
        subtract_poly_terms(KDEG, X, Y, phi);
        float conv = 0.0f;
#pragma unroll
        for (int t = 0; t < NT; ++t) conv = conv + (float)phi[t] * acc[t][p];
        double B = 0.0;
        int t = 0;
        for (int i = 0; i <= bg.deg; ++i)
            for (int j = 0; i + j <= bg.deg; ++j, ++t) B = B + bg.c[t] * (subtract_ipow(X, i) * subtract_ipow(Y, j));
        const float Bf = (float)B;
        const size_t at = (size_t)gy * (size_t)W + (size_t)gx;
        const float o = other[at];
        const float m = conv + Bf;
        float d = convolved_image ? (m - o) / a0 : (o - conv) - Bf;
        if (!is_finite(o) || d != d) d = nanv;                       // (every NaN written is the one quiet NaN)
        diff[at] = d;
        if (matched) matched[at] = m != m ? nanv : m;
    }
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_subtract_basis_f64(const double *sigmas_host, const int32_t *degrees_host, int32_t n_gauss, int32_t radius,
                                        double *filters_host, int32_t *row_host, int32_t *col_host, double *scale_host,
                                        int32_t *even_host, int32_t *n_filters_host, int32_t *n_basis_host)
{
    if (!sigmas_host || !degrees_host || !filters_host || !row_host || !col_host || !scale_host || !even_host || !n_filters_host ||
        !n_basis_host)
        return fail(APGPU_EINVAL, "subtract_basis: NULL pointer argument");
    if (n_gauss < 1 || n_gauss > kSubMaxBasis) return fail(APGPU_EINVAL, "subtract_basis: %d Gaussians", n_gauss);
    if (radius < 1) return fail(APGPU_EINVAL, "subtract_basis: radius %d", radius);
    if (radius > kSubMaxRadius) return fail(APGPU_EUNSUPPORTED, "subtract_basis: radius %d, the kernels hold %d", radius, kSubMaxRadius);
    for (int g = 0; g < n_gauss; ++g) {
        if (!(sigmas_host[g] > 0.0) || !(sigmas_host[g] < INFINITY)) return fail(APGPU_EINVAL, "subtract_basis: sigma %g", sigmas_host[g]);
        if (degrees_host[g] < 0) return fail(APGPU_EINVAL, "subtract_basis: degree %d", degrees_host[g]);
    }
    if (subtract_basis_count(n_gauss, degrees_host) < 0)
        return fail(APGPU_EUNSUPPORTED, "subtract_basis: more than %d basis functions", kSubMaxBasis);
    int nf = 0;
    *n_basis_host = subtract_basis_build(n_gauss, sigmas_host, degrees_host, radius, filters_host, row_host, col_host, scale_host, even_host, &nf);
    *n_filters_host = nf;
    for (int n = 0; n < *n_basis_host; ++n)
        if (!(fabs(scale_host[n]) < INFINITY)) return fail(APGPU_EINVAL, "subtract_basis: function %d has no finite sum at radius %d", n, radius);
    return APGPU_OK;
}

extern "C" int apgpu_subtract_stamps_f32(const float *tmpl, const float *image, const uint8_t *mask, int64_t height, int64_t width,
                                         const int32_t *centers, int32_t n_stamps, int32_t half, int32_t radius, const double *filters,
                                         int32_t n_filters, const int32_t *row_host, const int32_t *col_host, const double *scale_host,
                                         const int32_t *even_host, int32_t n_basis, double gain, double readnoise, double *gram_out,
                                         int32_t *status_out, int32_t *count_out, void *stream)
{
    if (int rc = check_plane("subtract_stamps", tmpl, height, width)) return rc;
    if (int rc = check_plane("subtract_stamps", image, height, width)) return rc;
    if (n_stamps < 0) return fail(APGPU_EINVAL, "subtract_stamps: negative stamp count %d", n_stamps);
    if (half < 1 || radius < 1) return fail(APGPU_EINVAL, "subtract_stamps: half-size %d or radius %d is below 1", half, radius);
    if (half > kMaxHalf || radius > kSubMaxRadius)
        return fail(APGPU_EUNSUPPORTED, "subtract_stamps: half-size %d or radius %d, the kernel holds %d and %d", half, radius, kMaxHalf, kSubMaxRadius);
    if (n_basis < 1 || n_filters < 1) return fail(APGPU_EINVAL, "subtract_stamps: %d basis functions on %d filters", n_basis, n_filters);
    if (n_basis > kSubMaxBasis || n_filters > kSubMaxBasis)
        return fail(APGPU_EUNSUPPORTED, "subtract_stamps: %d basis functions on %d filters, the kernel holds %d", n_basis, n_filters, kSubMaxBasis);
    if (!row_host || !col_host || !scale_host || !even_host) return fail(APGPU_EINVAL, "subtract_stamps: NULL pointer argument");
    if (!(gain >= 0.0) || !(gain < INFINITY) || !(readnoise >= 0.0) || !(readnoise < INFINITY) || (gain > 0.0 && !(readnoise > 0.0)))
        return fail(APGPU_EINVAL, "subtract_stamps: gain %g or readnoise %g is not valid (a gain needs a read noise above 0)", gain, readnoise);
    StampBasis b;
    b.nb = n_basis;
    b.nf = n_filters;
    for (int n = 0; n < kSubMaxBasis; ++n) {
        const bool in = n < n_basis;
        if (in && (row_host[n] < 0 || row_host[n] >= n_filters || col_host[n] < 0 || col_host[n] >= n_filters))
            return fail(APGPU_EINVAL, "subtract_stamps: function %d names the filters %d and %d of %d", n, row_host[n], col_host[n], n_filters);
        if (in && !(fabs(scale_host[n]) < INFINITY)) return fail(APGPU_EINVAL, "subtract_stamps: the scale of function %d is not finite", n);
        b.row[n] = in ? (uint8_t)row_host[n] : 0;
        b.col[n] = in ? (uint8_t)col_host[n] : 0;
        b.even[n] = in && n > 0 && even_host[n] != 0;
        b.scale[n] = in ? scale_host[n] : 0.0;
    }
    if (n_stamps == 0) return APGPU_OK;
    if (!centers || !filters || !gram_out || !status_out || !count_out || !aligned(centers, 4) || !aligned(filters, 8) ||
        !aligned(gram_out, 8) || !aligned(status_out, 4) || !aligned(count_out, 4))
        return fail(APGPU_EINVAL, "subtract_stamps: NULL or misaligned pointer argument");
    const double var0 = gain > 0.0 ? (readnoise * readnoise) / (gain * gain) : 0.0;
    hipLaunchKernelGGL(subtract_stamps_kernel, dim3((unsigned)n_stamps), dim3(kBlock), 0, as_stream(stream), tmpl, image, mask,
                       (long long)height, (long long)width, centers, (int)half, (int)radius, filters, b, var0, gain, gram_out, status_out,
                       count_out);
    return check_launch("subtract_stamps");
}

extern "C" int apgpu_subtract_apply_f32(const float *convolved, const float *other, int64_t height, int64_t width, const float *kernels,
                                        int32_t radius, int32_t kernel_degree, const double *bg_host, int32_t bg_degree, int32_t flags,
                                        float a0, float *diff_out, float *matched_out, void *stream)
{
    if (int rc = check_plane("subtract_apply", convolved, height, width)) return rc;
    if (int rc = check_plane("subtract_apply", other, height, width)) return rc;
    if (!kernels || !bg_host || !diff_out || !aligned(kernels, 4) || !aligned(diff_out, 4) || !aligned(matched_out, 4))
        return fail(APGPU_EINVAL, "subtract_apply: NULL or misaligned pointer argument");
    if (radius < 1) return fail(APGPU_EINVAL, "subtract_apply: radius %d", radius);
    if (radius > kSubMaxRadius) return fail(APGPU_EUNSUPPORTED, "subtract_apply: radius %d, the kernel holds %d", radius, kSubMaxRadius);
    if (kernel_degree < 0 || bg_degree < 0 || kernel_degree > kSubMaxDegree || bg_degree > kSubMaxDegree)
        return fail(APGPU_EINVAL, "subtract_apply: degrees %d and %d are outside 0 .. %d", kernel_degree, bg_degree, kSubMaxDegree);
    if (flags & ~APGPU_SUBTRACT_CONVOLVED_IMAGE) return fail(APGPU_EINVAL, "subtract_apply: flags 0x%x", flags);
    const int conv_image = (flags & APGPU_SUBTRACT_CONVOLVED_IMAGE) != 0;
    if (conv_image && (!(fabsf(a0) < INFINITY) || a0 == 0.0f)) return fail(APGPU_EINVAL, "subtract_apply: a0 = %g", (double)a0);
    if (diff_out == convolved || diff_out == other || (matched_out && (matched_out == convolved || matched_out == other || matched_out == diff_out)))
        return fail(APGPU_EINVAL, "subtract_apply: the outputs must be planes of their own");
    SubBackground bg;
    bg.deg = bg_degree;
    const int ntb = subtract_poly_count(bg_degree);
    for (int t = 0; t < kSubMaxTerms; ++t) {
        if (t < ntb && !(fabs(bg_host[t]) < INFINITY)) return fail(APGPU_EINVAL, "subtract_apply: background coefficient %d is not finite", t);
        bg.c[t] = t < ntb ? bg_host[t] : 0.0;
    }
    dim3 grid;
    if (int rc = tile_grid("subtract_apply", height, width, kTileH, kTileW, &grid)) return rc;
    const int wide = wide_rows(width, convolved);
    hipStream_t s = as_stream(stream);
    const long long H = height, W = width;
#define APGPU_SUBTRACT_LAUNCH(D)                                                                                                          \
    hipLaunchKernelGGL((subtract_apply_kernel<D>), grid, dim3(kBlock), 0, s, convolved, other, H, W, kernels, (int)radius, bg, conv_image, a0, \
                       wide, diff_out, matched_out)
    if (kernel_degree == 0) APGPU_SUBTRACT_LAUNCH(0);
    else if (kernel_degree == 1) APGPU_SUBTRACT_LAUNCH(1);
    else if (kernel_degree == 2) APGPU_SUBTRACT_LAUNCH(2);
    else APGPU_SUBTRACT_LAUNCH(3);
#undef APGPU_SUBTRACT_LAUNCH
    return check_launch("subtract_apply");
}
