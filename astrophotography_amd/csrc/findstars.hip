// findstars.hip - F6: ApFindStars (core/ApFindStars.py:87-201, 299-340, 363-446), DAOFIND star detection and aperture
// photometry, on gfx950.
//
// The reference hands the numerics to photutils (DAOStarFinder, find_peaks, aperture_photometry), which is not in the build
// container: the kernels implement the published DAOFIND algorithm (Stetson 1987) as restated in tests/findstars_model.py
// (parity with photutils itself is unpinned); the annulus statistic is astropy's noaxis sigma clip with sigclip_global.hip's
// definitions (golden group G16).
//
// 1. daofind_convolve_kernel: a 16 x 64 output tile per workgroup, the tile plus a halo of R staged in LDS with the
//    background subtracted on load (one float32 subtraction) and zeros outside the image; every output is the float64 sum
//    of float64(d) * K over all (2R+1)^2 taps in row-major tap order (separately rounded multiply and add), rounded once.
// 2. local_peaks_kernel: one lane per pixel; the threshold, mask and border tests reject nearly every pixel before the
//    footprint is walked.  Survivors are appended to the caller's list through one atomic counter: the counter always
//    counts, the list is written only while index < capacity.
// 3. daofind_measure_kernel: one wavefront per candidate; the lanes share the taps of the two cut-outs, the eight sums are
//    combined across the wavefront and every lane evaluates the same scalar arithmetic; lane 0 writes the record.
// 4. aperture_phot_kernel: one workgroup per source; exact circle-pixel overlap areas in float64, the annulus values
//    compacted in row-major order into LDS, the clip on them (median by a workgroup-wide bitwise selection, numpy's
//    float32 sums, np_exact.h, by one lane).
#include "common.h"
#include "np_exact.h"

namespace {
using namespace apgpu;

constexpr int kMaxR = 12;                       // largest kernel radius (fwhm < 20.4)
constexpr int kTileH = 16, kTileW = 64;
constexpr int kConvBlock = 256;
constexpr int kMaxSide = 2 * kMaxR + 1;
constexpr int kMaxFoot = 64;                    // largest footprint side of local_peaks
constexpr int kNQ = 6;                          // weight planes of the data cut-out (tests/findstars_model.py)
constexpr int kRec = 16;                        // doubles per record
constexpr int kAnnCap = 4096;                   // annulus values one workgroup holds in LDS (16 KiB)
constexpr int kPhotBlock = 256;

// ---- 1. convolution ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kConvBlock) void daofind_convolve_kernel(const float *__restrict__ data, long long H, long long W, int R,
                                                                     const double *__restrict__ kern, float bg,
                                                                     float *__restrict__ out)
{
    __shared__ float tile[(kTileH + 2 * kMaxR) * (kTileW + 2 * kMaxR)];
    __shared__ double wts[kMaxSide * kMaxSide];
    const int side = 2 * R + 1;
    const int tw = kTileW + 2 * R, th = kTileH + 2 * R;
    const long long i0 = (long long)blockIdx.y * kTileH, j0 = (long long)blockIdx.x * kTileW;
    for (int t = threadIdx.x; t < side * side; t += kConvBlock) wts[t] = kern[t];
    for (int t = threadIdx.x; t < tw * th; t += kConvBlock) {
        const int ty = t / tw, tx = t - ty * tw;
        const long long i = i0 + ty - R, j = j0 + tx - R;
        float v = 0.0f;
        if (i >= 0 && i < H && j >= 0 && j < W) v = data[i * W + j] - bg;
        tile[t] = v;
    }
    __syncthreads();
    const int tx = threadIdx.x & (kTileW - 1);
    const long long j = j0 + tx;
    if (j >= W) return;
    for (int ty = threadIdx.x / kTileW; ty < kTileH; ty += kConvBlock / kTileW) {
        const long long i = i0 + ty;
        if (i >= H) break;
        double acc = 0.0;
        // out[i, j] = sum_{a, b} K[a, b] * d[i + R - a, j + R - b]; d[i + R - a, .] is tile row ty + 2R - a
        for (int a = 0; a < side; a++) {
            const float *row = tile + (ty + 2 * R - a) * tw + tx + 2 * R;
            const double *wr = wts + a * side;
            for (int b = 0; b < side; b++) acc = __dadd_rn(acc, __dmul_rn((double)row[-b], wr[b]));
        }
        out[i * W + j] = (float)acc;
    }
}

// ---- 2. local peaks ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void local_peaks_kernel(const float *__restrict__ v, long long H, long long W,
                                                          const uint8_t *__restrict__ fp, int fh, int fw, double thr,
                                                          const uint8_t *__restrict__ mask, int border, int *__restrict__ list,
                                                          int capacity, int *__restrict__ count)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= H * W) return;
    const long long i = q / W, j = q - i * W;
    if (i < border || i >= H - border || j < border || j >= W - border) return;
    const float c = v[q];
    if (!((double)c > thr)) return;
    if (mask && mask[q]) return;
    const int ch = fh / 2, cw = fw / 2;
    for (int a = 0; a < fh; a++) {
        const long long ii = i + a - ch;
        for (int b = 0; b < fw; b++) {
            if (!fp[a * fw + b]) continue;
            const long long jj = j + b - cw;
            const float nb = (ii >= 0 && ii < H && jj >= 0 && jj < W) ? v[ii * W + jj] : 0.0f;
            if (nb > c) return;
        }
    }
    const int slot = atomicAdd(count, 1);
    if (slot < capacity) list[slot] = (int)q;
}

// ---- 3. measurement ------------------------------------------------------------------------------------------------------
// consts: 0 npixels - 1, 1 threshold_eff, 2 sharplo, 3 sharphi, 4 roundlo, 5 roundhi, 6 sigma^2, 7 p,
//         8..12 x: sumg, sumgsq, sdgd, sdgds, sgdgd; 13..17 y: the same
__global__ __launch_bounds__(256) void daofind_measure_kernel(const float *__restrict__ data, const float *__restrict__ conv, long long H,
                                                              long long W, const int *__restrict__ cand, int n, int R, float bg,
                                                              const double *__restrict__ tables, const double *__restrict__ quad,
                                                              const double *__restrict__ consts, double *__restrict__ rec,
                                                              uint8_t *__restrict__ keep)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int k = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (k >= n) return;                                              // whole wavefronts leave together
    const long long q = cand[k];
    const long long i = q / W, j = q - i * W;
    const int side = 2 * R + 1, ntap = side * side;
    double s[kNQ + 2];
#pragma unroll
    for (int t = 0; t < kNQ + 2; t++) s[t] = 0.0;
    const bool inside = q >= 0 && q < H * W && i >= R && i < H - R && j >= R && j < W - R;   // the peak finder guarantees it
    if (inside) {
        for (int t = lane; t < ntap; t += kWave) {
            const int a = t / side, b = t - a * side;
            const long long p = (i + a - R) * W + (j + b - R);
            const double d = (double)(data[p] - bg);
            const double c = (double)conv[p];
#pragma unroll
            for (int u = 0; u < kNQ; u++) s[u] = s[u] + d * tables[u * ntap + t];
            s[kNQ] = s[kNQ] + c * quad[t];
            s[kNQ + 1] = s[kNQ + 1] + ((a == R && b == R) ? 0.0 : fabs(c));
        }
    }
#pragma unroll
    for (int t = 0; t < kNQ + 2; t++) s[t] = wave_sum(s[t]);
    if (lane != 0) return;
    double *r = rec + (long long)k * kRec;
    if (!inside) {
        for (int t = 0; t < kRec; t++) r[t] = __builtin_nan("");
        keep[k] = 0;
        return;
    }
    const double nan = __builtin_nan("");
    const double peak = (double)(data[q] - bg), cpk = (double)conv[q];
    const double npm1 = consts[0], thr = consts[1], sigsq = consts[6], p = consts[7];
    const double sumd = s[1];
    const double sharp = (peak - (s[0] - peak) / npm1) / cpk;
    const double sum2 = s[kNQ], sum4 = s[kNQ + 1];
    const double round1 = sum2 == 0.0 ? 0.0 : (sum4 <= 0.0 ? nan : 2.0 * sum2 / sum4);
    double h[2], dd[2];
#pragma unroll
    for (int ax = 0; ax < 2; ax++) {
        const double *c = consts + 8 + 5 * ax;
        const double sumg = c[0], sumgsq = c[1], sdgd = c[2], sdgds = c[3], sgdgd = c[4];
        h[ax] = (s[2 + 2 * ax] - sumg * sumd / p) / (sumgsq - sumg * sumg / p);
        dd[ax] = (sgdgd - (s[3 + 2 * ax] - sdgd * sumd)) / (h[ax] * sdgds / sigsq);
    }
    const double round2 = 2.0 * (h[0] - h[1]) / (h[0] + h[1]);
    const double flux = cpk / thr;
    const double mag = flux > 0.0 ? -2.5 * log10(flux) : nan;
    const double xc = (double)j + dd[0], yc = (double)i + dd[1];
    r[0] = (double)j; r[1] = (double)i; r[2] = (double)ntap; r[3] = peak; r[4] = cpk; r[5] = sharp; r[6] = round1; r[7] = round2;
    r[8] = dd[0]; r[9] = dd[1]; r[10] = h[0]; r[11] = h[1]; r[12] = xc; r[13] = yc; r[14] = flux; r[15] = mag;
    bool ok = h[0] > 0.0 && h[1] > 0.0;
    ok = ok && sharp > consts[2] && sharp < consts[3] && round1 > consts[4] && round1 < consts[5] && round2 > consts[4] && round2 < consts[5];
    ok = ok && !(fabs(dd[0]) > (double)R) && !(fabs(dd[1]) > (double)R);
    ok = ok && is_finite(xc) && is_finite(yc) && is_finite(sharp) && is_finite(round1) && is_finite(round2) && is_finite(peak) &&
         is_finite(flux);
    keep[k] = ok ? 1 : 0;
}

// ---- 4. aperture photometry ------------------------------------------------------------------------------------------------
// integral of sqrt(r^2 - x^2) over [u, v]: trapezoid under the chord + circular segment
__device__ double arc_integral(double u, double v, double r)
{
    if (!(v > u)) return 0.0;
    const double hu = sqrt(fmax(r * r - u * u, 0.0));
    const double hv = sqrt(fmax(r * r - v * v, 0.0));
    const double w = v - u, dh = hv - hu;
    const double c = sqrt(w * w + dh * dh);
    double s = c / (2.0 * r);
    if (s > 1.0) s = 1.0;
    const double t = 2.0 * asin(s);
    return w * (hu + hv) / 2.0 + r * r / 2.0 * (t - sin(t));
}

// integral over [X0, X1] (inside [-r, r]) of clamp(y, -h(x), h(x))
__device__ double clamp_integral(double y, double X0, double X1, double r)
{
    const double ya = fabs(y);
    double val;
    if (ya >= r) {
        val = arc_integral(X0, X1, r);
    } else {
        const double a = sqrt(r * r - ya * ya);
        val = 0.0;
        double lo = X0, hi = fmin(X1, -a);
        if (hi > lo) val = val + arc_integral(lo, hi, r);
        lo = fmax(X0, -a); hi = fmin(X1, a);
        if (hi > lo) val = val + ya * (hi - lo);
        lo = fmax(X0, a); hi = X1;
        if (hi > lo) val = val + arc_integral(lo, hi, r);
    }
    return y < 0.0 ? -val : val;
}

__device__ double pixel_overlap(double x0, double x1, double y0, double y1, double r)
{
    const double fx = fmax(fabs(x0), fabs(x1)), fy = fmax(fabs(y0), fabs(y1));
    if (fx * fx + fy * fy <= r * r) return 1.0;
    const double nx = (x0 <= 0.0 && 0.0 <= x1) ? 0.0 : fmin(fabs(x0), fabs(x1));
    const double ny = (y0 <= 0.0 && 0.0 <= y1) ? 0.0 : fmin(fabs(y0), fabs(y1));
    if (nx * nx + ny * ny >= r * r) return 0.0;
    const double X0 = fmax(x0, -r), X1 = fmin(x1, r);
    if (!(X1 > X0)) return 0.0;
    const double a = clamp_integral(y1, X0, X1, r) - clamp_integral(y0, X0, X1, r);
    return a > 0.0 ? a : 0.0;
}

// the noaxis clip's float32 sums in numpy's order (np_exact.h: n <= kAnnCap < 8192 is one piece), by one lane; st is in LDS
template <typename F>
__device__ float numpy_sum(int n, F f, NpSumStack<float> &st)
{
    return 0.0f + np_pairwise_sum<float>(n, f, st);
}

using Key = OrderKey<float>;

// k-th smallest key of buf[0 .. n) (0-based), all lanes of the workgroup take part; cnt is one LDS word
__device__ unsigned block_select(const float *buf, int n, int k, int *cnt)
{
    unsigned ans = 0;
    for (int b = 31; b >= 0; b--) {
        const unsigned cand = ans | (1u << b);
        if (threadIdx.x == 0) *cnt = 0;
        __syncthreads();
        int less = 0;
        for (int t = threadIdx.x; t < n; t += kPhotBlock) less += Key::to(buf[t]) < cand;
        if (less) atomicAdd(cnt, less);
        __syncthreads();
        if (*cnt <= k) ans = cand;
        __syncthreads();
    }
    return ans;
}

// np.median of buf[0 .. n), n >= 1, no NaN: np.mean of the middle element(s), whose sum starts from +0 (a median of -0.0 is +0.0)
__device__ float block_median(const float *buf, int n, int *cnt)
{
    const float hi = Key::from(block_select(buf, n, n / 2, cnt));
    if (n & 1) return 0.0f + hi;
    const float lo = Key::from(block_select(buf, n, n / 2 - 1, cnt));
    return (0.0f + lo + hi) / 2.0f;
}

__global__ __launch_bounds__(kPhotBlock) void aperture_phot_kernel(const float *__restrict__ data, long long H, long long W,
                                                                   const double *__restrict__ xc, const double *__restrict__ yc, int n_src,
                                                                   double r_ap, double r_in, double r_out, double sigma, int maxiters,
                                                                   double *__restrict__ sum_out, float *__restrict__ bkg_out,
                                                                   int *__restrict__ nann_out, double *__restrict__ area_out)
{
    __shared__ float buf[kAnnCap];
    __shared__ double red[2][kPhotBlock / kWave];
    __shared__ int s_n, s_cnt, s_go;
    __shared__ int wave_cnt[kPhotBlock / kWave];
    __shared__ float s_lo, s_hi;
    __shared__ NpSumStack<float> sum_stack;
    const int k = blockIdx.x;
    if (k >= n_src) return;
    const double cx = xc[k], cy = yc[k];
    const int tid = threadIdx.x;

    // aperture sum: the pixels whose square can touch the circle
    double sum = 0.0, area = 0.0;
    if (fabs(cx) < 1e15 && fabs(cy) < 1e15) {
        long long i0 = (long long)ceil(cy - r_ap - 0.5), i1 = (long long)floor(cy + r_ap + 0.5);
        long long j0 = (long long)ceil(cx - r_ap - 0.5), j1 = (long long)floor(cx + r_ap + 0.5);
        if (i0 < 0) i0 = 0;
        if (j0 < 0) j0 = 0;
        if (i1 > H - 1) i1 = H - 1;
        if (j1 > W - 1) j1 = W - 1;
        const long long bw = j1 - j0 + 1, bh = i1 - i0 + 1;
        if (bw > 0 && bh > 0) {
            for (long long t = tid; t < bw * bh; t += kPhotBlock) {
                const long long i = i0 + t / bw, j = j0 + t % bw;
                const double a = pixel_overlap(((double)j - 0.5) - cx, ((double)j + 0.5) - cx, ((double)i - 0.5) - cy,
                                               ((double)i + 0.5) - cy, r_ap);
                if (a > 0.0) {
                    sum = sum + a * (double)data[i * W + j];
                    area = area + a;
                }
            }
        }
    }
    sum = wave_sum(sum);
    area = wave_sum(area);
    if ((tid & (kWave - 1)) == 0) { red[0][tid / kWave] = sum; red[1][tid / kWave] = area; }
    if (tid == 0) s_n = 0;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0, a = 0.0;
        for (int w = 0; w < kPhotBlock / kWave; w++) { s = s + red[0][w]; a = a + red[1][w]; }
        sum_out[k] = s;
        area_out[k] = a;
    }

    // annulus: pixel centres with r_in^2 <= d2 <= r_out^2, row-major, compacted in order one row chunk at a time
    int n_ann = 0;
    if (fabs(cx) < 1e15 && fabs(cy) < 1e15) {
        long long i0 = (long long)ceil(cy - r_out - 0.5), i1 = (long long)floor(cy + r_out + 0.5);
        long long j0 = (long long)ceil(cx - r_out - 0.5), j1 = (long long)floor(cx + r_out + 0.5);
        if (i0 < 0) i0 = 0;
        if (j0 < 0) j0 = 0;
        if (i1 > H - 1) i1 = H - 1;
        if (j1 > W - 1) j1 = W - 1;
        const long long bw = j1 - j0 + 1, bh = i1 - i0 + 1;
        const long long total = (bw > 0 && bh > 0) ? bw * bh : 0;
        for (long long base = 0; base < total; base += kPhotBlock) {
            const long long t = base + tid;
            bool in = false;
            float val = 0.0f;
            if (t < total) {
                const long long i = i0 + t / bw, j = j0 + t % bw;
                const double dx = (double)j - cx, dy = (double)i - cy;
                const double d2 = dx * dx + dy * dy;
                in = d2 >= r_in * r_in && d2 <= r_out * r_out;
                if (in) val = data[i * W + j];
            }
            const unsigned long long bal = __ballot(in);
            const int lane = tid & (kWave - 1), wv = tid / kWave;
            if (lane == 0) wave_cnt[wv] = __popcll(bal);
            __syncthreads();
            int off = n_ann, tot = 0;
            for (int w = 0; w < kPhotBlock / kWave; w++) {
                if (w < wv) off += wave_cnt[w];
                tot += wave_cnt[w];
            }
            if (in) {
                const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
                if (pos < kAnnCap) buf[pos] = val;              // the host rejects radii whose annulus cannot fit
            }
            n_ann += tot;
            __syncthreads();
        }
    }
    if (n_ann > kAnnCap) n_ann = kAnnCap;
    if (tid == 0) {
        nann_out[k] = n_ann;
        // drop the non-finite values, in order
        int m = 0;
        for (int t = 0; t < n_ann; t++) {
            const float x = buf[t];
            if (is_finite(x)) buf[m++] = x;
        }
        s_n = m;
    }
    __syncthreads();
    // astropy _sigmaclip_noaxis: while something was removed and iteration < maxiters
    for (int it = 0; maxiters < 0 || it < maxiters; it++) {
        const int n = s_n;
        if (n <= 0) break;
        const float med = block_median(buf, n, &s_cnt);
        if (tid == 0) {
            const float sm = numpy_sum(n, [&](int i) { return buf[i]; }, sum_stack);
            const float mean = sm / (float)n;
            const float s2 = numpy_sum(n, [&](int i) { const float d = buf[i] - mean; return d * d; }, sum_stack);
            const float var = (float)((double)s2 / (double)n);
            const float sd = (float)sqrt((double)var);
            s_lo = (float)((double)med - (double)sd * sigma);
            s_hi = (float)((double)med + (double)sd * sigma);
            const float lo = s_lo, hi = s_hi;
            int m = 0;
            for (int t = 0; t < n; t++) {
                const float x = buf[t];
                if (x >= lo && x <= hi) buf[m++] = x;
            }
            s_go = m != n;
            s_n = m;
        }
        __syncthreads();
        const int go = s_go;
        __syncthreads();
        if (!go) break;
    }
    const int n = s_n;
    float med = __builtin_nanf("");
    if (n > 0) med = block_median(buf, n, &s_cnt);
    if (tid == 0) bkg_out[k] = med;
}

}  // namespace

extern "C" int apgpu_daofind_convolve_f32(const float *data, int64_t height, int64_t width, const double *kernel, int32_t radius,
                                          float bg_median, float *out, void *stream)
{
    if (!data || !kernel || !out) return fail(APGPU_EINVAL, "daofind_convolve: NULL pointer argument");
    if (height <= 0 || width <= 0) return fail(APGPU_EINVAL, "daofind_convolve: bad shape [%lld, %lld]", (long long)height, (long long)width);
    if (radius < 1) return fail(APGPU_EINVAL, "daofind_convolve: radius = %d < 1", radius);
    if (radius > kMaxR) return fail(APGPU_EUNSUPPORTED, "daofind_convolve: kernel radius %d > %d (fwhm too large)", radius, kMaxR);
    const long long gy = (height + kTileH - 1) / kTileH, gx = (width + kTileW - 1) / kTileW;
    if (gy > 65535) return fail(APGPU_EUNSUPPORTED, "daofind_convolve: more than %d rows", 65535 * kTileH);
    hipLaunchKernelGGL(daofind_convolve_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kConvBlock), 0, as_stream(stream), data,
                       (long long)height, (long long)width, (int)radius, kernel, bg_median, out);
    return check_launch("daofind_convolve");
}

extern "C" int apgpu_local_peaks_f32(const float *values, int64_t height, int64_t width, const uint8_t *footprint, int32_t fp_height,
                                     int32_t fp_width, double threshold, const uint8_t *mask, int32_t border, int32_t *list,
                                     int32_t capacity, int32_t *count_out, void *stream)
{
    if (!values || !footprint || !count_out) return fail(APGPU_EINVAL, "local_peaks: NULL pointer argument");
    if (capacity < 0 || (capacity > 0 && !list)) return fail(APGPU_EINVAL, "local_peaks: capacity %d without a list", capacity);
    if (height <= 0 || width <= 0) return fail(APGPU_EINVAL, "local_peaks: bad shape [%lld, %lld]", (long long)height, (long long)width);
    if (height * width >= (1ll << 31)) return fail(APGPU_EUNSUPPORTED, "local_peaks: 2^31 pixels or more");
    if (fp_height < 1 || fp_width < 1 || fp_height > kMaxFoot || fp_width > kMaxFoot)
        return fail(APGPU_EINVAL, "local_peaks: footprint %d x %d outside 1 .. %d", fp_height, fp_width, kMaxFoot);
    if (border < 0) return fail(APGPU_EINVAL, "local_peaks: border = %d < 0", border);
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(count_out, 0, sizeof(int32_t), s) != hipSuccess) return fail(APGPU_ELAUNCH, "local_peaks: hipMemsetAsync failed");
    const long long P = height * width;
    hipLaunchKernelGGL(local_peaks_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, values, (long long)height, (long long)width,
                       footprint, (int)fp_height, (int)fp_width, threshold, mask, (int)border, list, (int)capacity, count_out);
    return check_launch("local_peaks");
}

extern "C" int apgpu_daofind_measure(const float *data, const float *conv, int64_t height, int64_t width, const int32_t *candidates,
                                     int32_t n_candidates, int32_t radius, float bg_median, const double *tables, const double *quad,
                                     const double *consts, double *records, uint8_t *keep, void *stream)
{
    if (n_candidates == 0) return APGPU_OK;
    if (!data || !conv || !candidates || !tables || !quad || !consts || !records || !keep)
        return fail(APGPU_EINVAL, "daofind_measure: NULL pointer argument");
    if (height <= 0 || width <= 0 || n_candidates < 0)
        return fail(APGPU_EINVAL, "daofind_measure: bad shape [%lld, %lld] or count %d", (long long)height, (long long)width, n_candidates);
    if (height * width >= (1ll << 31)) return fail(APGPU_EUNSUPPORTED, "daofind_measure: 2^31 pixels or more");
    if (radius < 1) return fail(APGPU_EINVAL, "daofind_measure: radius = %d < 1", radius);
    if (radius > kMaxR) return fail(APGPU_EUNSUPPORTED, "daofind_measure: kernel radius %d > %d (fwhm too large)", radius, kMaxR);
    const int per = 256 / kWave;
    hipLaunchKernelGGL(daofind_measure_kernel, dim3((unsigned)((n_candidates + per - 1) / per)), dim3(256), 0, as_stream(stream), data, conv,
                       (long long)height, (long long)width, candidates, (int)n_candidates, (int)radius, bg_median, tables, quad, consts,
                       records, keep);
    return check_launch("daofind_measure");
}

extern "C" int apgpu_aperture_phot_f32(const float *data, int64_t height, int64_t width, const double *xc, const double *yc,
                                       int32_t n_sources, double r_aperture, double r_in, double r_out, double sigma, int32_t maxiters,
                                       double *sum_raw, float *bkg_median, int32_t *n_annulus, double *area, void *stream)
{
    if (n_sources == 0) return APGPU_OK;
    if (!data || !xc || !yc || !sum_raw || !bkg_median || !n_annulus || !area)
        return fail(APGPU_EINVAL, "aperture_phot: NULL pointer argument");
    if (height <= 0 || width <= 0 || n_sources < 0)
        return fail(APGPU_EINVAL, "aperture_phot: bad shape [%lld, %lld] or count %d", (long long)height, (long long)width, n_sources);
    if (!(r_aperture > 0.0) || !(r_in >= 0.0) || !(r_out > r_in) || !(r_out < 1e6))
        return fail(APGPU_EINVAL, "aperture_phot: bad radii %g, %g, %g", r_aperture, r_in, r_out);
    // pixel centres inside the annulus lie in the ring r_in - sqrt(1/2) .. r_out + sqrt(1/2) of unit squares: its area bounds the count
    const double h = 0.70710678118654757, ri = r_in > h ? r_in - h : 0.0, ro = r_out + h;
    const double bound = 3.14159265358979312 * (ro * ro - ri * ri);
    if (bound > (double)kAnnCap)
        return fail(APGPU_EUNSUPPORTED, "aperture_phot: an annulus %g .. %g may hold %.0f pixels, more than %d (fwhm too large)", r_in, r_out,
                    bound, kAnnCap);
    hipLaunchKernelGGL(aperture_phot_kernel, dim3((unsigned)n_sources), dim3(kPhotBlock), 0, as_stream(stream), data, (long long)height,
                       (long long)width, xc, yc, (int)n_sources, r_aperture, r_in, r_out, sigma, (int)maxiters, sum_raw,
                       bkg_median, n_annulus, area);
    return check_launch("aperture_phot");
}
