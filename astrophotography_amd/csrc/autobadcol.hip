// autobadcol.hip - F5: ApAutoBadcols.process (core/ApAutoBadcols.py:180-258), the bad column / row finder, on gfx950.
//
// Reference:
//     medn_cols = np.nanmedian(data, axis=0); medn_rows = np.nanmedian(data, axis=1)         (:196, :200)
//     for each median array m (length L):  _sliding_stats_1d(m, window_len)                   (:143-167)
//         window i = m[max(0, i - hw) : min(L, i + hw + 1)], hw = int((window_len - 1) / 2)
//         mean[i], _, std[i] = sigma_clipped_stats(window)   (sigma 3, maxiters 5, axis=None: _sigmaclip_noaxis)
//     nsig = |m - mean| / std (float64), bad = nsig >= nsigma                                  (:225-227)
//
// 1. axis_median_kernel<T, COLS>: exact np.nanmedian of a line by radix select on order-preserving keys (8-bit digits,
//    4 levels for float32, 8 for float64) with LDS histograms.  For columns a workgroup owns 32 of them: lane c of every
//    half-wavefront reads column c0 + c (a 128-byte row segment per row, coalesced; 128 workgroups for one 4096-wide
//    frame) and the 32 half-wavefronts interleave the rows; for rows each wavefront owns one contiguous row (4 per
//    workgroup).  Every level re-reads the lines (a
//    column tile of 64 x H values and a row stay in L2 / the Infinity Cache between levels).  numpy 1.26 takes
//    lines shorter than 600 through np.ma.median - the middle value of an odd count is T(x + x) / 2 there - and
//    longer ones through np.median; an even count is T(a + b) / 2 on both paths, an all-NaN line NaN.  uint16 pixels
//    are widened to float64 as they are loaded (numpy's median of integers is float64).
// 2. sliding_stats_kernel<T>: one lane per output index.  The lane compacts its window's finite values, in order, into
//    its slot of the workspace and runs astropy's noaxis clip on them with sigclip_global.hip's definitions: median by
//    exact selection, numpy's summation order (np_exact.h), np.var's float32 mean T(sum) / T(n), var T(float64(s2) / n),
//    mean T(float64(sum) / n), float64 bounds demoted to T for the comparison.  The default window (11) keeps everything
//    in one lane; any window_len >= 1 works (long windows are slow but exact).
// Both kernels run on the caller's stream with no host synchronisation; the host reads back only the per-line results.
#include "common.h"
#include "np_exact.h"

namespace {
using namespace apgpu;

constexpr int kMedBlock = 256;               // rows: 4 per workgroup (one per wavefront); the sliding statistics
constexpr int kColBlock = 1024;               // columns: 32 per workgroup (one per lane), 32 half-wavefronts interleave the rows
constexpr int kLinesPerGroup = 32;
constexpr int kDigitBits = 8;
constexpr int kDigitBins = 1 << kDigitBits;
constexpr long long kMaPathLen = 600;         // numpy _nanmedian: a.shape[axis] < 600 -> _nanmedian_small (np.ma.median)

// ---- 1. axis medians ---------------------------------------------------------------------------------------------------
// Per-line selection state, in LDS.
template <typename T>
struct LineSel {
    typename OrderKey<T>::U prefix;        // key bits found so far (upper middle element, rank k of the non-NaN values)
    typename OrderKey<T>::U below;         // largest key below the final key (even count, found by the extra pass)
    long long n;                      // non-NaN values
    long long k;                      // rank still searched inside the current prefix
    int need_below;                   // even count whose lower middle element is not fixed by the histograms
    int lo_digit;                     // highest occupied bin below the picked one at the last level (-1: none)
};

// In: the stored pixel type (T, or uint16_t widened exactly to T = double on load)
template <typename In, typename T, bool COLS>
__global__ __launch_bounds__(COLS ? kColBlock : kMedBlock) void axis_median_kernel(const In *__restrict__ data, long long H, long long W, T *__restrict__ out)
{
    using K = OrderKey<T>;
    using U = typename K::U;
    constexpr int levels = K::bits / kDigitBits;
    constexpr int BS = COLS ? kColBlock : kMedBlock;
    constexpr int LPG = COLS ? kLinesPerGroup : kMedBlock / kWave;          // lines per workgroup
    constexpr int TPL = BS / LPG;                                           // threads per line
    const long long frame = blockIdx.y;
    const In *img = data + frame * H * W;
    const long long nlines = COLS ? W : H;                                  // lines of this frame
    const long long len = COLS ? H : W;                                     // values per line
    const long long line0 = (long long)blockIdx.x * LPG;
    const int t = threadIdx.x;
    const int ln = COLS ? (t % LPG) : (t / TPL);                            // line of this thread inside the group
    const int ph = COLS ? (t / LPG) : (t % TPL);                            // its phase along the line
    const long long line = line0 + ln;
    const bool valid = line < nlines;

    __shared__ unsigned hist[LPG][kDigitBins + 1];          // +1: lanes of different lines on different banks
    __shared__ LineSel<T> sel[LPG];
    __shared__ unsigned long long below_sh[LPG];

    auto at = [&](long long e) -> T { return (T)(COLS ? img[e * W + line] : img[line * W + e]); };

    for (int i = t; i < LPG * (kDigitBins + 1); i += BS) (&hist[0][0])[i] = 0u;
    if (t < LPG) { sel[t].prefix = 0; sel[t].below = 0; sel[t].n = 0; sel[t].k = 0; sel[t].need_below = 0; sel[t].lo_digit = -1; }
    __syncthreads();

    for (int level = 0; level < levels; level++) {
        const int shift = K::bits - kDigitBits * (level + 1);
        const U pfx = sel[ln].prefix;
        if (valid) {
            for (long long e = ph; e < len; e += TPL) {
                const T x = at(e);
                if (x != x) continue;                                       // NaN: dropped
                const U key = K::to(x);
                // the bits above this level's digit must equal the prefix found so far
                if (level > 0 && (key >> (shift + kDigitBits)) != pfx) continue;
                atomicAdd(&hist[ln][(unsigned)(key >> shift) & (kDigitBins - 1)], 1u);
            }
        }
        __syncthreads();
        if (t < LPG && line0 + t < nlines) {
            LineSel<T> &s = sel[t];
            if (level == 0) {
                long long n = 0;
                for (int b = 0; b < kDigitBins; b++) n += hist[t][b];
                s.n = n;
                s.k = n / 2;                                                // upper middle (odd: the median)
            }
            if (s.n > 0) {
                long long run = 0;
                int pick = 0, lo = -1;
                for (int b = 0; b < kDigitBins; b++) {
                    const unsigned c = hist[t][b];
                    if (s.k < run + c) { pick = b; break; }
                    if (c) lo = b;
                    run += c;
                }
                s.k -= run;
                s.prefix = (s.prefix << kDigitBits) | (U)pick;
                s.lo_digit = lo;
            }
            for (int b = 0; b < kDigitBins; b++) hist[t][b] = 0u;
        }
        __syncthreads();
    }
    // even count, lower middle element: the same key if the upper one is not the first of its key; the highest lower bin
    // of the last level; otherwise the largest key below the found key (one more read of the line)
    if (t < LPG) {
        LineSel<T> &s = sel[t];
        below_sh[t] = 0;
        s.need_below = (s.n > 0 && (s.n & 1) == 0 && s.k == 0 && s.lo_digit < 0) ? 1 : 0;
        if (s.n > 0 && (s.n & 1) == 0) {
            if (s.k >= 1) s.below = s.prefix;
            else if (s.lo_digit >= 0) s.below = (s.prefix & ~(U)(kDigitBins - 1)) | (U)s.lo_digit;
        }
    }
    __syncthreads();
    if (valid && sel[ln].need_below) {
        const U top = sel[ln].prefix;
        unsigned long long best = 0;                                        // keys of non-NaN values are never 0
        for (long long e = ph; e < len; e += TPL) {
            const T x = at(e);
            if (x != x) continue;
            const U key = K::to(x);
            if (key < top && (unsigned long long)key > best) best = (unsigned long long)key;
        }
        if (best) atomicMax(&below_sh[ln], best);
    }
    __syncthreads();
    if (t < LPG && line0 + t < nlines) {
        const LineSel<T> &s = sel[t];
        T med;
        if (s.n == 0) {
            med = (T)__builtin_nan("");
        } else {
            // both of numpy's paths sum the middle element(s) from +0: a median of -0.0 is +0.0
            const T hi = K::from(s.prefix);
            if (s.n & 1) {
                med = len < kMaPathLen ? (T)((T)0 + hi + hi) / (T)2 : (T)0 + hi;   // np.ma.median sums the duplicated middle value
            } else {
                const T lo = K::from(s.need_below ? (U)below_sh[t] : s.below);
                med = (T)((T)0 + lo + hi) / (T)2;
            }
        }
        out[frame * nlines + line0 + t] = med;
    }
}

// ---- 2. sliding clipped statistics ---------------------------------------------------------------------------------------
// the terms of numpy's two sums: the values, and their squared deviations from the mean
template <typename T>
struct Values {
    const T *a;
    __device__ T operator()(long long i) const { return a[i]; }
};
template <typename T>
struct SquaredDev {
    const T *a;
    T mean;
    __device__ T operator()(long long i) const { const T d = a[i] - mean; return d * d; }
};

// np.add.reduce of the terms f(0) .. f(n - 1) (csrc/np_exact.h) by this lane, its stack private: every lane runs a sum of
// its own.  Out of line, so that the common short windows below do not carry the tree's registers.
template <typename T, typename F>
__device__ __noinline__ T numpy_tree_sum(long long n, F f)
{
    NpSumStack<T> st;
    return np_add_reduce<T>(n, f, st);
}

// windows of up to 128 values (the default 11 among them) are one leaf and stay in registers
template <typename T, typename F>
__device__ __forceinline__ T numpy_sum(long long n, F f)
{
    if (n <= 128) return (T)0 + np_leaf_sum<T>((int)n, f);
    return numpy_tree_sum<T>(n, f);
}

// k-th smallest (0-based) of a[0 .. n) by bitwise search on the order-preserving keys (no reordering of a)
template <typename T>
__device__ typename OrderKey<T>::U select_key(const T *a, long long n, long long k)
{
    using K = OrderKey<T>;
    using U = typename K::U;
    if (n <= 24) {                              // rank counting: n^2 compares, cheaper than `bits` passes for short windows
        for (long long i = 0; i < n; i++) {
            const U ki = K::to(a[i]);
            long long less = 0, eq = 0;
            for (long long j = 0; j < n; j++) {
                const U kj = K::to(a[j]);
                less += kj < ki;
                eq += kj == ki;
            }
            if (less <= k && k < less + eq) return ki;
        }
        return 0;
    }
    U ans = 0;
    for (int b = K::bits - 1; b >= 0; b--) {
        const U cand = ans | ((U)1 << b);
        long long less = 0;
        for (long long i = 0; i < n; i++) less += K::to(a[i]) < cand;
        if (less <= k) ans = cand;
    }
    return ans;
}

// np.median of a[0 .. n), n >= 1, no NaN (np.median: the middle value, or the mean of the two in T)
template <typename T>
__device__ T median_of(const T *a, long long n)
{
    using K = OrderKey<T>;
    const T hi = K::from(select_key<T>(a, n, n / 2));
    if (n & 1) return hi;
    const T lo = K::from(select_key<T>(a, n, n / 2 - 1));
    return (T)(lo + hi) / (T)2;
}

// np.nanstd of a[0 .. n), n >= 1 (as sigclip_global.hip): mean T(sum) / T(n), float32 sum of squares, T(float64(s2) / n)
template <typename T>
__device__ T std_of(const T *a, long long n, T sum)
{
    const T mean = sum / (T)n;
    const T s2 = numpy_sum<T>(n, SquaredDev<T>{a, mean});
    const T var = (T)((double)s2 / (double)n);
    return (T)sqrt((double)var);
}

template <typename T>
__global__ __launch_bounds__(kMedBlock) void sliding_stats_kernel(const T *__restrict__ v, long long nlines, long long L, long long hw,
                                                                 double sigma, int maxiters, double nsigma, double *__restrict__ mean_out,
                                                                 double *__restrict__ std_out, double *__restrict__ nsig_out,
                                                                 uint8_t *__restrict__ flag_out, T *__restrict__ scratch, long long wcap,
                                                                 long long first, long long count)
{
    const long long slot = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    T *buf = scratch + slot * wcap;
    for (long long o = first + slot; o < first + count; o += stride) {
        const long long line = o / L, i = o % L;
        const T *m = v + line * L;
        const long long a = i - hw < 0 ? 0 : i - hw;
        const long long b = i + hw + 1 < L ? i + hw + 1 : L;
        long long n = 0;
        for (long long j = a; j < b; j++) {
            const T x = m[j];
            if (is_finite(x)) buf[n++] = x;                                 // finite values, in order
        }
        // astropy _sigmaclip_noaxis: while something was removed and iteration < maxiters
        for (int it = 0; n > 0 && (maxiters < 0 || it < maxiters); it++) {
            const T med = median_of<T>(buf, n);
            const T sd = std_of<T>(buf, n, numpy_sum<T>(n, Values<T>{buf}));
            // SigmaClip._compute_bounds: T scalars * python float -> float64, demoted to T for the comparison
            const T lo = (T)((double)med - (double)sd * sigma), hi = (T)((double)med + (double)sd * sigma);
            long long k = 0;
            for (long long j = 0; j < n; j++) {
                const T x = buf[j];
                if (x >= lo && x <= hi) buf[k++] = x;
            }
            const bool changed = k != n;
            n = k;
            if (!changed) break;
        }
        double mean = __builtin_nan(""), sd = __builtin_nan("");
        if (n > 0) {
            const T sum = numpy_sum<T>(n, Values<T>{buf});
            mean = (double)(T)((double)sum / (double)n);                    // np.mean: T(float64(sum) / n)
            sd = (double)std_of<T>(buf, n, sum);
        }
        const double ns = fabs((double)m[i] - mean) / sd;
        mean_out[o] = mean;
        std_out[o] = sd;
        nsig_out[o] = ns;
        flag_out[o] = ns >= nsigma ? 1 : 0;
    }
}

constexpr long long kScratchBudget = 64ll << 20;      // bytes of per-lane window buffers
constexpr long long kMaxSlots = 65536;

long long window_cap(long long L, long long window_len)
{
    const long long hw = (window_len - 1) / 2;
    const long long w = 2 * hw + 1;
    return w < L ? w : L;
}

long long slots_for(long long total, long long wcap, size_t elem)
{
    long long s = kScratchBudget / (wcap * (long long)elem);
    if (s > kMaxSlots) s = kMaxSlots;
    s = (s / kMedBlock) * kMedBlock;
    if (s < kMedBlock) s = kMedBlock;
    const long long need = (total + kMedBlock - 1) / kMedBlock * kMedBlock;
    return s < need ? s : need;
}

template <typename In, typename T>
int run_axis_median(const In *data, int64_t N, int64_t H, int64_t W, int axis, T *out, hipStream_t s)
{
    if (axis == 0) {
        const dim3 grid((unsigned)((W + kLinesPerGroup - 1) / kLinesPerGroup), (unsigned)N);
        hipLaunchKernelGGL((axis_median_kernel<In, T, true>), grid, dim3(kColBlock), 0, s, data, (long long)H, (long long)W, out);
    } else {
        constexpr int rpg = kMedBlock / kWave;
        const dim3 grid((unsigned)((H + rpg - 1) / rpg), (unsigned)N);
        hipLaunchKernelGGL((axis_median_kernel<In, T, false>), grid, dim3(kMedBlock), 0, s, data, (long long)H, (long long)W, out);
    }
    return check_launch("axis_nanmedian");
}

template <typename T>
int run_sliding(const T *v, int64_t nlines, int64_t L, int64_t window_len, double sigma, int maxiters, double nsigma, double *mean,
                double *sd, double *nsig, uint8_t *flag, void *ws, hipStream_t s)
{
    const long long wcap = window_cap(L, window_len);
    const long long total = nlines * L;
    const long long slots = slots_for(total, wcap, sizeof(T));
    const long long hw = (window_len - 1) / 2;
    // one launch per `slots` outputs when the window buffers cannot cover them all at once
    const long long per_launch = slots * 64;
    for (long long first = 0; first < total; first += per_launch) {
        const long long count = total - first < per_launch ? total - first : per_launch;
        hipLaunchKernelGGL(sliding_stats_kernel<T>, dim3((unsigned)(slots / kMedBlock)), dim3(kMedBlock), 0, s, v, (long long)nlines,
                           (long long)L, hw, sigma, maxiters, nsigma, mean, sd, nsig, flag, static_cast<T *>(ws), wcap, first, count);
        if (int rc = check_launch("sliding_clipped_stats")) return rc;
    }
    return 0;
}

}  // namespace

extern "C" int apgpu_axis_nanmedian(const void *data, int dtype, int64_t n_frames, int64_t height, int64_t width, int axis, void *out,
                                    void *stream)
{
    if (!data || !out) return fail(APGPU_EINVAL, "axis_nanmedian: NULL pointer argument");
    if (n_frames <= 0 || height <= 0 || width <= 0)
        return fail(APGPU_EINVAL, "axis_nanmedian: bad shape [%lld, %lld, %lld]", (long long)n_frames, (long long)height,
                    (long long)width);
    if (n_frames > 65535) return fail(APGPU_EUNSUPPORTED, "axis_nanmedian: more than 65535 frames in one call");
    if (axis != 0 && axis != 1) return fail(APGPU_EINVAL, "axis_nanmedian: axis must be 0 or 1, got %d", axis);
    hipStream_t s = as_stream(stream);
    if (dtype == APGPU_F32) return run_axis_median<float, float>((const float *)data, n_frames, height, width, axis, (float *)out, s);
    if (dtype == APGPU_F64) return run_axis_median<double, double>((const double *)data, n_frames, height, width, axis, (double *)out, s);
    if (dtype == APGPU_U16)
        return run_axis_median<uint16_t, double>((const uint16_t *)data, n_frames, height, width, axis, (double *)out, s);
    return fail(APGPU_EINVAL, "axis_nanmedian: dtype must be APGPU_F32, APGPU_F64 or APGPU_U16, got %d", dtype);
}

extern "C" size_t apgpu_sliding_clipped_stats_ws_bytes(int dtype, int64_t n_lines, int64_t length, int64_t window_len)
{
    if ((dtype != APGPU_F32 && dtype != APGPU_F64) || n_lines <= 0 || length <= 0 || window_len < 1) return 0;
    const size_t elem = dtype == APGPU_F64 ? sizeof(double) : sizeof(float);
    const long long wcap = window_cap(length, window_len);
    return (size_t)slots_for((long long)n_lines * length, wcap, elem) * (size_t)wcap * elem;
}

extern "C" int apgpu_sliding_clipped_stats(const void *values, int dtype, int64_t n_lines, int64_t length, int64_t window_len, double sigma,
                                           int maxiters, double nsigma, double *mean, double *std, double *nsig, uint8_t *flag, void *ws,
                                           size_t ws_bytes, void *stream)
{
    if (!values || !mean || !std || !nsig || !flag || !ws) return fail(APGPU_EINVAL, "sliding_clipped_stats: NULL pointer argument");
    if (n_lines <= 0 || length <= 0)
        return fail(APGPU_EINVAL, "sliding_clipped_stats: bad shape [%lld, %lld]", (long long)n_lines, (long long)length);
    if (window_len < 1) return fail(APGPU_EINVAL, "sliding_clipped_stats: window_len = %lld < 1", (long long)window_len);
    if (dtype != APGPU_F32 && dtype != APGPU_F64)
        return fail(APGPU_EINVAL, "sliding_clipped_stats: dtype must be APGPU_F32 or APGPU_F64, got %d", dtype);
    const size_t need = apgpu_sliding_clipped_stats_ws_bytes(dtype, n_lines, length, window_len);
    if (ws_bytes < need) return fail(APGPU_EWORKSPACE, "sliding_clipped_stats: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t s = as_stream(stream);
    if (dtype == APGPU_F32)
        return run_sliding<float>((const float *)values, n_lines, length, window_len, sigma, maxiters, nsigma, mean, std, nsig, flag, ws, s);
    return run_sliding<double>((const double *)values, n_lines, length, window_len, sigma, maxiters, nsigma, mean, std, nsig, flag, ws, s);
}
