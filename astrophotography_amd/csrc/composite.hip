// composite.hip - F9: the colour composite of three co-added planes (the STIFF step of scripts/composite_all.sh) on gfx950.
//
// STIFF is not part of the reference tree, so the arithmetic is this project's own definition (PARITY
// UNPINNED), restated in tests/composite_model.py.  Everything is float32 in the stated order, no contraction.
//
//   levels     v = the finite values of a channel in ascending order; level(q) = v[floor(q (n - 1))]: an exact order
//              statistic by radix select on the order-preserving key of the float (OrderKey<float> of np_exact.h), 8-bit
//              digits, four levels.  All three channels and both targets (min, max) go through the same four reads of
//              the planes; the digit of each target is picked on the device by a one-workgroup kernel between them.
//   composite  scale_c = 1 / (hi_c - lo_c)                     (0 unless hi_c > lo_c)
//              s_c = pos((x_c - lo_c) scale_c)                  pos(a) = a > 0 ? a : 0  (NaN -> 0)
//              Y   = ((s_0 + s_1) + s_2) float32(1/3)
//              c_c = pos(Y + sat (s_c - Y))
//              o_c = c_c G(Y) < 1 ? c_c G(Y) : 1                (NaN -> 1)
//              pixel_c = (unsigned)(o_c (2^bits - 1) + 0.5f);   any x_c not finite: the pixel is black
//              G(Y) = Y^(1 / gamma) / Y from a float32 table indexed by the bits of Y (256 knots per octave, 2^-40 .. 1),
//              linear in between: G[i] + t (G[i + 1] - G[i]); Y < 2^-40 -> G = 0, Y > 1 -> G(1).
//              One pass: a lane reads four consecutive pixels of the three planes once and writes them for every variant
//              (a variant = a table and a saturation), as 3 or 6 whole dwords where the destination is dword aligned.
#include "common.h"
#include "np_exact.h"

namespace apgpu {
namespace {

constexpr int kLevBlock = 512;
constexpr int kLevDigit = 8;
constexpr int kLevBins = 1 << kLevDigit;
constexpr int kLevPasses = 32 / kLevDigit;
constexpr int kLevMaxGroups = 512;          // workgroups per channel of a histogram pass
constexpr unsigned kNoDigit = 0xffffffffu;

constexpr int kCompBlock = 256;
constexpr int kMaxVariants = APGPU_COMPOSITE_MAX_VARIANTS;
constexpr int kTableLen = APGPU_TONE_TABLE_LEN;
constexpr unsigned kTableBase = (127u - 40u) << 8;          // (bits >> 15) of 2^-40

struct LevelState {
    unsigned long long n[3];                // finite values per channel
    unsigned long long k[3][2];             // rank searched, relative to the prefix
    unsigned prefix[3][2];                  // key bits found so far
    unsigned hist[3][2][kLevBins];
};

// One level of the select: the histogram of the digit at `shift` over the finite values whose higher key bits equal the
// target's prefix.  blockIdx.y = channel.  On the first level the prefix is empty and both targets share histogram 0.
// A lane's consecutive equal digits are added in one LDS atomic (sky pixels share their leading digits).
__global__ __launch_bounds__(kLevBlock) void level_hist_kernel(const float *__restrict__ planes, long long n_pixels,
                                                              LevelState *__restrict__ st, int pass)
{
    const int c = blockIdx.y;
    const float *p = planes + (size_t)c * n_pixels;
    const int shift = 32 - kLevDigit * (pass + 1);
    const int ntargets = pass == 0 ? 1 : 2;
    const unsigned pre0 = st->prefix[c][0], pre1 = st->prefix[c][1];
    __shared__ unsigned h[2][kLevBins];
    for (int t = threadIdx.x; t < 2 * kLevBins; t += kLevBlock) (&h[0][0])[t] = 0;
    __syncthreads();
    unsigned cur_d[2] = {kNoDigit, kNoDigit}, cur_n[2] = {0, 0};
    auto add = [&](float x) {
        if (!is_finite(x)) return;
        const unsigned key = OrderKey<float>::to(x);
        const unsigned d = (key >> shift) & (kLevBins - 1);
        const unsigned top = pass == 0 ? 0u : key >> (shift + kLevDigit);
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (t < ntargets && top == (t ? pre1 : pre0)) {
                if (d != cur_d[t]) {
                    if (cur_d[t] != kNoDigit) atomicAdd(&h[t][cur_d[t]], cur_n[t]);
                    cur_d[t] = d;
                    cur_n[t] = 0;
                }
                cur_n[t]++;
            }
        }
    };
    // scalar head up to the first 16-byte boundary, float4 body, scalar tail
    long long head = (long long)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4);
    head = head < n_pixels ? head : n_pixels;
    const long long nvec = (n_pixels - head) / 4;
    const long long tail0 = head + nvec * 4;
    const long long tid = (long long)blockIdx.x * kLevBlock + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * kLevBlock;
    if (tid < head) add(p[tid]);
    const float4 *pv = reinterpret_cast<const float4 *>(p + head);
    for (long long i = tid; i < nvec; i += nthreads) {
        const float4 v = pv[i];
        add(v.x); add(v.y); add(v.z); add(v.w);
    }
    if (tail0 + tid < n_pixels) add(p[tail0 + tid]);
#pragma unroll
    for (int t = 0; t < 2; t++)
        if (cur_d[t] != kNoDigit) atomicAdd(&h[t][cur_d[t]], cur_n[t]);
    __syncthreads();
    for (int t = threadIdx.x; t < ntargets * kLevBins; t += kLevBlock) {
        const unsigned v = (&h[0][0])[t];
        if (v) atomicAdd(&st->hist[c][0][t], v);
    }
}

// Closes a level: wavefront w = 2 c + t finds the bin of its target's rank (4 bins per lane + a wavefront scan), extends
// the prefix and clears the histogram for the next level.  The first level also fixes n and the two ranks; the last
// one publishes the levels.
__global__ __launch_bounds__(6 * kWave) void level_pick_kernel(LevelState *__restrict__ st, int pass, const double *__restrict__ q,
                                                              const float *__restrict__ manual, float *__restrict__ levels,
                                                              long long *__restrict__ n_finite)
{
    const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int c = w / 2, t = w % 2;
    unsigned *h = st->hist[c][pass == 0 ? 0 : t];
    unsigned cnt[4];
    unsigned long long sum = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        cnt[j] = h[lane * 4 + j];
        sum += cnt[j];
    }
    unsigned long long inc = sum;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    unsigned long long n, k;
    if (pass == 0) {
        n = __shfl(inc, kWave - 1);
        // np.quantile(method='lower'): floor(q (n - 1)), the product in float64
        double r = n > 0 ? floor(q[2 * c + t] * (double)(n - 1)) : 0.0;
        r = r > 0.0 ? r : 0.0;
        k = n > 0 ? (unsigned long long)r : 0;
        if (n > 0 && k > n - 1) k = n - 1;
    } else {
        n = st->n[c];
        k = st->k[c][t];
    }
    __syncthreads();                                        // both targets have read histogram 0 of the first level
    const unsigned long long exc = inc - sum;
    if (n > 0 && k >= exc && k < inc) {
        unsigned long long run = exc;                       // values below the bin that holds rank k
        int digit = -1;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (digit < 0) {
                if (k < run + cnt[j]) digit = lane * 4 + j;
                else run += cnt[j];
            }
        }
        const unsigned prefix = pass == 0 ? (unsigned)digit : ((st->prefix[c][t] << kLevDigit) | (unsigned)digit);
        st->prefix[c][t] = prefix;
        st->k[c][t] = k - run;
        if (pass == 0 && t == 0) st->n[c] = n;
        if (pass == kLevPasses - 1) {
            const float m = manual ? manual[2 * c + t] : __builtin_nanf("");
            levels[2 * c + t] = m == m ? m : OrderKey<float>::from(prefix);
        }
    }
    if (n == 0 && lane == 0) {
        if (pass == 0 && t == 0) st->n[c] = 0;
        if (pass == kLevPasses - 1) {
            const float m = manual ? manual[2 * c + t] : __builtin_nanf("");
            levels[2 * c + t] = m == m ? m : __builtin_nanf("");
        }
    }
    if (pass == kLevPasses - 1 && t == 0 && lane == 0) n_finite[c] = (long long)n;
    __syncthreads();
    if (pass > 0 || t == 0) {
#pragma unroll
        for (int j = 0; j < 4; j++) h[lane * 4 + j] = 0;
    }
}

struct CompositeArgs {
    const float *planes;
    const float *levels;
    const float *tables;
    void *out;
    long long height, width;
    int n_variants, flip;
    float sat[kMaxVariants];
};

__device__ __forceinline__ float pos(float a) { return a > 0.0f ? a : 0.0f; }

// What the variants share of one pixel: s_c, Y, the table cell and the weight inside it.
struct PixelCommon {
    float s[3], y, t;
    unsigned idx;           // table cell; kTableLen: G = 0 (Y < 2^-40)
    bool black;
};

__device__ __forceinline__ PixelCommon pixel_common(const float (&x)[3], const float (&lo)[3], const float (&scale)[3])
{
    PixelCommon p;
    p.black = !(is_finite(x[0]) && is_finite(x[1]) && is_finite(x[2]));
#pragma unroll
    for (int c = 0; c < 3; c++) p.s[c] = pos((x[c] - lo[c]) * scale[c]);
    p.y = ((p.s[0] + p.s[1]) + p.s[2]) * (float)(1.0 / 3.0);
    const float yl = p.y > 1.0f ? 1.0f : p.y;
    const unsigned b = __float_as_uint(yl);
    const bool tiny = !(yl >= 0x1p-40f);
    p.idx = tiny ? (unsigned)kTableLen : (b >> 15) - kTableBase;
    p.t = (float)(b & 0x7fffu) * 0x1p-15f;
    return p;
}

template <typename OutT>
__device__ __forceinline__ void pixel_variant(const PixelCommon &p, const float *__restrict__ table, float sat, OutT (&o)[3])
{
    constexpr float maxv = sizeof(OutT) == 1 ? 255.0f : 65535.0f;
    float g = 0.0f;
    if (p.idx < (unsigned)kTableLen) {
        const float g0 = table[p.idx];
        const float g1 = table[p.idx + 1 < (unsigned)kTableLen ? p.idx + 1 : p.idx];   // the closing knot (Y = 1) has t = 0
        const float d = g1 - g0;
        const float m = p.t * d;
        g = g0 + m;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float dc = p.s[c] - p.y;
        const float sc = sat * dc;
        const float cc = pos(p.y + sc);
        const float v = cc * g;
        const float oc = v < 1.0f ? v : 1.0f;
        const float r = oc * maxv;
        o[c] = p.black ? (OutT)0 : (OutT)(unsigned)(r + 0.5f);
    }
}

// A lane owns the four consecutive pixels x0 .. x0 + 3 of one output row.
template <typename OutT>
__global__ __launch_bounds__(kCompBlock) void composite_kernel(const CompositeArgs a)
{
    const long long W = a.width, H = a.height;
    const long long groups_per_row = (W + 3) / 4;
    const long long gid = (long long)blockIdx.x * kCompBlock + threadIdx.x;
    if (gid >= groups_per_row * H) return;
    const long long r = gid / groups_per_row;                       // output row
    const long long x0 = (gid - r * groups_per_row) * 4;
    const long long src_row = a.flip ? H - 1 - r : r;
    const int npix = (int)(W - x0 < 4 ? W - x0 : 4);
    const size_t plane = (size_t)H * (size_t)W;
    const float *src = a.planes + (size_t)src_row * (size_t)W + (size_t)x0;

    float lo[3], scale[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float l = a.levels[2 * c], h = a.levels[2 * c + 1];
        lo[c] = l;
        scale[c] = h > l ? 1.0f / (h - l) : 0.0f;                   // IEEE division; NaN levels compare false
    }

    float x[3][4];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float *pc = src + (size_t)c * plane;
        if (npix == 4 && (reinterpret_cast<uintptr_t>(pc) & 15) == 0) {
            const float4 v = *reinterpret_cast<const float4 *>(pc);
            x[c][0] = v.x; x[c][1] = v.y; x[c][2] = v.z; x[c][3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) x[c][j] = j < npix ? pc[j] : 0.0f;
        }
    }
    PixelCommon px[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float xj[3] = {x[0][j], x[1][j], x[2][j]};
        px[j] = pixel_common(xj, lo, scale);
    }

    constexpr int kWords = 3 * (int)sizeof(OutT);                   // dwords of four pixels
    const size_t image = plane * 3;                                 // components of one variant's image
    OutT *dst = static_cast<OutT *>(a.out) + ((size_t)r * (size_t)W + (size_t)x0) * 3;
    const bool whole = npix == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0 && ((image * sizeof(OutT)) & 3) == 0;
    for (int v = 0; v < a.n_variants; v++, dst += image) {
        const float *table = a.tables + (size_t)v * kTableLen;
        const float sat = a.sat[v];
        union {
            OutT o[4][3];
            unsigned w[kWords];
        } u;
#pragma unroll
        for (int j = 0; j < 4; j++) pixel_variant<OutT>(px[j], table, sat, u.o[j]);
        if (whole) {
            unsigned *d = reinterpret_cast<unsigned *>(dst);
#pragma unroll
            for (int i = 0; i < kWords; i++) d[i] = u.w[i];
        } else {
            // row tails and rows that do not start on a dword: component by component
            for (int j = 0; j < npix; j++) {
#pragma unroll
                for (int c = 0; c < 3; c++) dst[j * 3 + c] = u.o[j][c];
            }
        }
    }
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" size_t apgpu_quantile_levels_ws_bytes(int64_t height, int64_t width)
{
    if (height <= 0 || width <= 0) return 0;
    return (sizeof(LevelState) + 255) & ~(size_t)255;
}

extern "C" int apgpu_quantile_levels_f32(const float *planes, int64_t height, int64_t width, const double *q, const float *manual,
                                         float *levels, int64_t *n_finite, void *ws, size_t ws_bytes, void *stream)
{
    if (!planes || !q || !levels || !n_finite || !ws) return fail(APGPU_EINVAL, "quantile_levels: NULL pointer argument");
    if (height <= 0 || width <= 0) return fail(APGPU_EINVAL, "quantile_levels: image of %lld x %lld", (long long)height, (long long)width);
    if (ws_bytes < sizeof(LevelState)) return fail(APGPU_EWORKSPACE, "quantile_levels: workspace %zu < %zu bytes", ws_bytes, sizeof(LevelState));
    if (reinterpret_cast<uintptr_t>(ws) & 15) return fail(APGPU_EINVAL, "quantile_levels: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(planes) & 3) return fail(APGPU_EINVAL, "quantile_levels: planes must be 4-byte aligned");
    hipStream_t s = as_stream(stream);
    LevelState *st = static_cast<LevelState *>(ws);
    if (hipMemsetAsync(st, 0, sizeof(LevelState), s) != hipSuccess) return fail(APGPU_ELAUNCH, "quantile_levels: hipMemsetAsync failed");
    const long long n = (long long)height * (long long)width;
    const long long want = (n + (long long)kLevBlock * 16 - 1) / ((long long)kLevBlock * 16);       // 16 values per lane
    const unsigned groups = (unsigned)(want < 1 ? 1 : (want > kLevMaxGroups ? kLevMaxGroups : want));
    for (int pass = 0; pass < kLevPasses; pass++) {
        hipLaunchKernelGGL(level_hist_kernel, dim3(groups, 3), dim3(kLevBlock), 0, s, planes, n, st, pass);
        hipLaunchKernelGGL(level_pick_kernel, dim3(1), dim3(6 * kWave), 0, s, st, pass, q, manual, levels, (long long *)n_finite);
    }
    return check_launch("quantile_levels");
}

extern "C" int apgpu_composite_rgb(const float *planes, int64_t height, int64_t width, const float *levels, const float *tables,
                                   const float *colour_sat_host, int32_t n_variants, int32_t bits, int32_t flip, void *out, void *stream)
{
    if (!planes || !levels || !tables || !colour_sat_host || !out) return fail(APGPU_EINVAL, "composite_rgb: NULL pointer argument");
    if (height <= 0 || width <= 0) return fail(APGPU_EINVAL, "composite_rgb: image of %lld x %lld", (long long)height, (long long)width);
    if (n_variants < 1 || n_variants > kMaxVariants)
        return fail(APGPU_EINVAL, "composite_rgb: %d variants (1 .. %d)", n_variants, kMaxVariants);
    if (bits != 8 && bits != 16) return fail(APGPU_EINVAL, "composite_rgb: %d bits per channel (8 or 16)", bits);
    if ((reinterpret_cast<uintptr_t>(planes) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
        return fail(APGPU_EINVAL, "composite_rgb: planes and out must be 4-byte aligned");
    const long long groups = ((long long)width + 3) / 4 * (long long)height;
    const long long blocks = (groups + kCompBlock - 1) / kCompBlock;
    if (blocks > 0x7fffffffLL) return fail(APGPU_EUNSUPPORTED, "composite_rgb: image of %lld x %lld is too large", (long long)height, (long long)width);
    CompositeArgs a;
    a.planes = planes; a.levels = levels; a.tables = tables; a.out = out;
    a.height = height; a.width = width; a.n_variants = n_variants; a.flip = flip != 0;
    for (int v = 0; v < kMaxVariants; v++) a.sat[v] = v < n_variants ? colour_sat_host[v] : 0.0f;
    hipStream_t s = as_stream(stream);
    if (bits == 8) hipLaunchKernelGGL(composite_kernel<uint8_t>, dim3((unsigned)blocks), dim3(kCompBlock), 0, s, a);
    else hipLaunchKernelGGL(composite_kernel<uint16_t>, dim3((unsigned)blocks), dim3(kCompBlock), 0, s, a);
    return check_launch("composite_rgb");
}
