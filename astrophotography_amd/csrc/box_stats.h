// box_stats.h - the sigma-clipped median / std of a box of pixels, one workgroup per box (exact radix-select medians): the kernel
// behind apgpu_box_clipped_stats_f32 (background.hip: the boxes of a mesh) and apgpu_sample_clipped_stats_f32 (gradient.hip: boxes
// about a list of centres).  Where a box lies is the ORIGIN's business; everything else is one definition.
//
// Per-box sigma-clipped statistics: one workgroup per box.  astropy's SigmaClip(sigma, maxiters, median / std)
// along the box: every pass computes the median (exact, 4-pass 8-bit radix select on order-preserving keys) and the
// standard deviation of the current survivors and keeps lo <= x <= hi; clipping only ever shrinks the interval, so the
// survivors of pass k are exactly the unmasked finite values inside the running [lo, hi] - no compaction: a box of up to
// 32768 pixels is staged in LDS once (NaN = masked) and every pass walks the LDS copy; larger boxes re-read the image.  Pixels outside the image (edge_method 'pad'), masked or non-finite
// pixels count as masked.  Output per box (float64): median, std of the final survivors, number of survivors,
// number of masked pixels before clipping.
#pragma once
#include "common.h"
#include "np_exact.h"

namespace apgpu {

struct BoxView {
    const float *data;
    const uint8_t *mask;
    int H, W, r0, c0, bh, bw;
};

// The boxes of a mesh: box i is the (i / nx)-th row and (i % nx)-th column of boxes, its origin never negative.
struct MeshOrigin {
    static constexpr bool kSigned = false;
    static constexpr bool kOrderedStd = false;
    int nx;
    __device__ __forceinline__ void place(BoxView &b, int box) const
    {
        b.r0 = (box / nx) * b.bh;
        b.c0 = (box % nx) * b.bw;
    }
};

// Square boxes of half-size r about centres[box] = (x, y): the origin may lie left of or above the image.  A centre more than r
// outside the image has no pixel inside it; its origin is put at (H, W) so that no coordinate sum can overflow.
struct ListOrigin {
    static constexpr bool kSigned = true;
    static constexpr bool kOrderedStd = true;              // the std of the final survivors as the oracle forms it: see the kernel's end
    const int *centres;
    int r;
    __device__ __forceinline__ void place(BoxView &b, int box) const
    {
        const int x = centres[2 * box], y = centres[2 * box + 1];
        const bool out = x < -r || y < -r || x >= b.W + r || y >= b.H + r;
        b.r0 = out ? b.H : y - r;
        b.c0 = out ? b.W : x - r;
    }
};

// value of box element e (row-major inside the box) or NaN if masked / outside / non-finite
template <bool SIGNED>
__device__ __forceinline__ float box_value(const BoxView &b, int e)
{
    const int rr = b.r0 + e / b.bw, cc = b.c0 + e % b.bw;
    if (rr >= b.H || cc >= b.W) return __builtin_nanf("");
    if constexpr (SIGNED)
        if (rr < 0 || cc < 0) return __builtin_nanf("");
    const int64_t p = (int64_t)rr * b.W + cc;
    if (b.mask && b.mask[p]) return __builtin_nanf("");
    const float x = b.data[p];
    return is_finite(x) ? x : __builtin_nanf("");
}

template <int NT>
__device__ double block_sum(double v, double *scratch)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
    __syncthreads();
    if ((threadIdx.x % kWave) == 0) scratch[threadIdx.x / kWave] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < NT / kWave; w++) t += scratch[w];       // every thread forms the same ordered sum
    return t;
}

constexpr int kBoxDigit = 11;               // radix-select digit: 11 + 11 + 10 bits of the order-preserving float32 key
constexpr int kBoxBins = 1 << kBoxDigit;
constexpr int kBoxLdsPixels = 32768;        // boxes up to this many pixels are staged in LDS (128 KB of the 160 KB)
constexpr unsigned kNoDigit = 0xffffffffu;

struct DigitPick {
    int digit;          // bin that holds the searched rank
    unsigned cum;       // values in the bins below it
    int dlow;           // highest occupied bin below it (-1: none)
};

// Wavefront 0 finds the bin of rank k in hist[0 .. kBoxBins) (32 bins per lane + a wavefront scan) and publishes it.
__device__ __forceinline__ DigitPick pick_digit(const unsigned *hist, unsigned k, DigitPick *shared_pick)
{
    if (threadIdx.x < kWave) {
        const int lane = threadIdx.x;
        constexpr int per = kBoxBins / kWave;
        unsigned tot = 0;
#pragma unroll 4
        for (int j = 0; j < per; j++) tot += hist[lane * per + j];
        unsigned inc = tot;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        const unsigned exc = inc - tot;
        int dlow = -1;
        if (k >= exc && k < inc) {
            unsigned run = exc;
#pragma unroll 1
            for (int j = 0; j < per; j++) {
                const unsigned c = hist[lane * per + j];
                if (k < run + c) { shared_pick->digit = lane * per + j; shared_pick->cum = run; break; }
                if (c) dlow = lane * per + j;
                run += c;
            }
        } else if (k >= inc) {
#pragma unroll 1
            for (int j = per - 1; j >= 0; j--)
                if (hist[lane * per + j]) { dlow = lane * per + j; break; }
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const int o = __shfl_down(dlow, d);
            dlow = o > dlow ? o : dlow;
        }
        if (lane == 0) shared_pick->dlow = dlow;
    }
    __syncthreads();
    const DigitPick r = *shared_pick;
    __syncthreads();
    return r;
}

// NT threads per box: 256 for small boxes, 1024 for the 16 x 16 meshes of full frames (one workgroup per CU, 16 wavefronts).
// RES: the box (<= kBoxLdsPixels pixels) is staged in LDS once, masked / outside / non-finite pixels as NaN; otherwise every
// pass walks the image rows of the box (coalesced runs, L2 / Infinity Cache resident after the first pass).
// Passes: the first iteration makes four - (a) count + sum, (b) sum of squared deviations + first select level, (c) second
// level, (d) third level + the largest survivor below the found prefix (the lower middle element of an even count comes from
// the last histogram or from (d)'s maximum, not from a second select); every later iteration makes two - count, moments about
// the previous median, first level and a speculated second level in one, then (d).
template <int NT, bool RES, typename ORIGIN>
__global__ __launch_bounds__(NT) void box_stats_kernel(const float *__restrict__ data, const uint8_t *__restrict__ mask, int H, int W,
                                                      int bh, int bw, const ORIGIN origin, double sigma, int maxiters, double *__restrict__ out)
{
    static_assert(RES || !ORIGIN::kSigned, "only an LDS-resident box may start outside the image");
    static_assert(RES || !ORIGIN::kOrderedStd, "the ordered std walks the LDS copy of the box");
    extern __shared__ float vals[];
    __shared__ unsigned hist[kBoxBins], hist2[kBoxBins];
    __shared__ double scratch[NT / kWave];
    __shared__ unsigned s_below[NT / kWave];
    __shared__ DigitPick s_pick;
    BoxView b;
    b.data = data; b.mask = mask; b.H = H; b.W = W; b.bh = bh; b.bw = bw;
    const int box = blockIdx.x;
    origin.place(b, box);
    const int npix = bh * bw;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if constexpr (RES) {
        for (int r = wave; r < bh; r += NT / kWave)
            for (int c = lane; c < bw; c += kWave) vals[r * bw + c] = box_value<ORIGIN::kSigned>(b, r * bw + c);
        __syncthreads();
    }
    // f(x) for every candidate value (RES: NaN marks the excluded ones and fails every comparison)
    auto for_each = [&](auto f) {
        if constexpr (RES) {
            for (int e = threadIdx.x; e < npix; e += NT) f(vals[e]);
        } else {
            // two rows x four 64-column chunks per trip: 16 independent loads in flight per lane (one load at a time leaves
            // the pass bound by the Infinity Cache latency)
            constexpr int RU = 2, CU = 4;
            const int cend = min(bw, W - b.c0);
            const int rend = min(bh, H - b.r0);
            for (int r = wave * RU; r < rend; r += (NT / kWave) * RU) {
                for (int c0 = 0; c0 < cend; c0 += CU * kWave) {
                    float x[RU][CU];
                    uint8_t m[RU][CU];
#pragma unroll
                    for (int u = 0; u < RU; u++) {
                        const int64_t rowp = (int64_t)(b.r0 + r + u) * W + b.c0;
#pragma unroll
                        for (int q = 0; q < CU; q++) {
                            const int c = c0 + q * kWave + lane;
                            const bool in = (r + u) < rend && c < cend;
                            m[u][q] = in ? (mask ? mask[rowp + c] : (uint8_t)0) : (uint8_t)1;
                            x[u][q] = in ? data[rowp + c] : 0.0f;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < RU; u++)
#pragma unroll
                        for (int q = 0; q < CU; q++)
                            if (!m[u][q]) f(x[u][q]);
                }
            }
        }
    };
    auto zero_hist = [&]() {
        for (int t = threadIdx.x; t < kBoxBins; t += NT) hist[t] = 0;
        __syncthreads();
    };
    // Working set of the clipping passes: values inside the running intersection [lo_run, hi_run] of all bounds so far
    // (astropy packs its buffer the same way).  The FINAL survivors are the values inside the LAST computed bounds
    // [lo_last, hi_last] applied to all data (astropy sigma_clipping.py:356-358: a value clipped by an earlier, tighter
    // pass can come back).  Bounds are float64 in astropy and applied to float32 data: lo <= (double)x <= hi is the
    // same set as ceil32(lo) <= x <= floor32(hi).  Non-finite values fail lo <= x <= hi from the first pass on
    // (+-inf only while the bounds are still infinite: excluded explicitly).
    float lo_run = -3.4028234663852886e38f, hi_run = 3.4028234663852886e38f, lo_last = lo_run, hi_last = hi_run;
    double med = __builtin_nan(""), sd = __builtin_nan("");
    int n = 0, n_prev = -1, n_unmasked = -1;
    unsigned guess0 = 0;                                    // first-level digit of the previous iteration's median
    for (int pass = 0;; pass++) {
        const bool final_pass = pass >= maxiters || n_prev == -2;
        const float lo = final_pass ? lo_last : lo_run, hi = final_pass ? hi_last : hi_run;
        unsigned prefix, kk;
        if (pass == 0 || RES) {
            // first iteration (and every iteration of an LDS-resident box, which is bound by its LDS atomics and gains nothing
            // from fewer reads): count + sum, then spread + first select level, then the second level (3 passes)
            double cnt = 0.0, sum = 0.0;
            for_each([&](float x) {
                if (x >= lo && x <= hi) {
                    cnt += 1.0;
                    sum += (double)x;
                }
            });
            n = (int)block_sum<NT>(cnt, scratch);
            const double total = block_sum<NT>(sum, scratch);
            if (n_unmasked < 0) n_unmasked = n;
            if (n == 0) {
                if (final_pass || pass == 0) {
                    med = sd = __builtin_nan("");
                    break;
                }
                // a pass before maxiters removed everything: astropy's next pass divides 0 by 0, its bounds are NaN, no comparison
                // with them masks anything - every unmasked finite value of the box survives (golden group G15 holds such boxes)
                lo_last = -3.4028234663852886e38f;
                hi_last = 3.4028234663852886e38f;
                n_prev = -2;
                continue;
            }
            if (!final_pass && n == n_prev) {               // the last bounds removed nothing: converged, evaluate the survivors
                n_prev = -2;
                continue;
            }
            const double mean = total / (double)n;
            const unsigned k = (unsigned)(n >> 1);          // upper middle element (the median itself for odd n)
            // spread + leading 11 key bits.  The sky values of a box share their leading digits: run-length coded per
            // thread before they reach the LDS histogram.
            zero_hist();
            double ss = 0.0;
            unsigned cur_d = kNoDigit, cur_n = 0;
            for_each([&](float x) {
                if (x >= lo && x <= hi) {
                    const double d = mean - (double)x;
                    ss += d * d;
                    const unsigned dg = OrderKey<float>::to(x) >> (32 - kBoxDigit);
                    if (dg != cur_d) {
                        if (cur_d != kNoDigit) atomicAdd(&hist[cur_d], cur_n);
                        cur_d = dg;
                        cur_n = 0;
                    }
                    cur_n++;
                }
            });
            if (cur_d != kNoDigit) atomicAdd(&hist[cur_d], cur_n);
            sd = sqrt(block_sum<NT>(ss, scratch) / (double)n);   // (its barriers also close the histogram)
            DigitPick pk = pick_digit(hist, k, &s_pick);
            prefix = (unsigned)pk.digit;
            kk = k - pk.cum;
            guess0 = prefix;
            zero_hist();
            for_each([&](float x) {
                if (x >= lo && x <= hi) {
                    const unsigned key = OrderKey<float>::to(x);
                    if ((key >> 21) == prefix) atomicAdd(&hist[(key >> 10) & (kBoxBins - 1)], 1u);
                }
            });
            __syncthreads();
            pk = pick_digit(hist, kk, &s_pick);
            prefix = (prefix << kBoxDigit) | (unsigned)pk.digit;
            kk -= pk.cum;
        } else {
            // later iterations: ONE pass for count, moments about the previous median (S1 = sum(x - p), S2 = sum((x - p)^2):
            // mean = p + S1 / n, n var = S2 - S1^2 / n - p sits inside the survivors, so nothing cancels), the first select
            // level, and the second level speculated on the first level's digit of the previous iteration (the median hardly
            // moves); a wrong guess costs the separate second-level pass.
            const double p = med;
            zero_hist();
            const unsigned g0 = guess0;
            for (int t = threadIdx.x; t < kBoxBins; t += NT) hist2[t] = 0;
            __syncthreads();
            double cnt = 0.0, s1 = 0.0, s2 = 0.0;
            unsigned cur_d = kNoDigit, cur_n = 0;
            for_each([&](float x) {
                if (x >= lo && x <= hi) {
                    cnt += 1.0;
                    const double d = (double)x - p;
                    s1 += d;
                    s2 = fma(d, d, s2);
                    const unsigned key = OrderKey<float>::to(x);
                    const unsigned dg = key >> (32 - kBoxDigit);
                    if (dg != cur_d) {
                        if (cur_d != kNoDigit) atomicAdd(&hist[cur_d], cur_n);
                        cur_d = dg;
                        cur_n = 0;
                    }
                    cur_n++;
                    if (dg == g0) atomicAdd(&hist2[(key >> 10) & (kBoxBins - 1)], 1u);
                }
            });
            if (cur_d != kNoDigit) atomicAdd(&hist[cur_d], cur_n);
            n = (int)block_sum<NT>(cnt, scratch);
            const double S1 = block_sum<NT>(s1, scratch), S2 = block_sum<NT>(s2, scratch);
            if (n == 0) {
                if (final_pass || pass == 0) {
                    med = sd = __builtin_nan("");
                    break;
                }
                // a pass before maxiters removed everything: astropy's next pass divides 0 by 0, its bounds are NaN, no comparison
                // with them masks anything - every unmasked finite value of the box survives (golden group G15 holds such boxes)
                lo_last = -3.4028234663852886e38f;
                hi_last = 3.4028234663852886e38f;
                n_prev = -2;
                continue;
            }
            if (!final_pass && n == n_prev) {               // the last bounds removed nothing: converged, evaluate the survivors
                n_prev = -2;
                continue;
            }
            const double nv = S2 - S1 * S1 / (double)n;
            sd = sqrt((nv > 0.0 ? nv : 0.0) / (double)n);
            const unsigned k = (unsigned)(n >> 1);
            DigitPick pk = pick_digit(hist, k, &s_pick);
            prefix = (unsigned)pk.digit;
            kk = k - pk.cum;
            if (prefix == g0) {
                pk = pick_digit(hist2, kk, &s_pick);
            } else {
                guess0 = prefix;
                zero_hist();
                for_each([&](float x) {
                    if (x >= lo && x <= hi) {
                        const unsigned key = OrderKey<float>::to(x);
                        if ((key >> 21) == prefix) atomicAdd(&hist[(key >> 10) & (kBoxBins - 1)], 1u);
                    }
                });
                __syncthreads();
                pk = pick_digit(hist, kk, &s_pick);
            }
            prefix = (prefix << kBoxDigit) | (unsigned)pk.digit;
            kk -= pk.cum;
        }
        // (d) last 10 bits + the largest survivor key below the 22-bit prefix
        zero_hist();
        unsigned below = 0;
        for_each([&](float x) {
            if (x >= lo && x <= hi) {
                const unsigned key = OrderKey<float>::to(x);
                const unsigned top = key >> 10;
                if (top == prefix) atomicAdd(&hist[key & 1023u], 1u);
                else if (top < prefix) below = key > below ? key : below;
            }
        });
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const unsigned o = __shfl_down(below, d);
            below = o > below ? o : below;
        }
        if (lane == 0) s_below[wave] = below;
        __syncthreads();
        const DigitPick pk = pick_digit(hist, kk, &s_pick);
        const unsigned key2 = (prefix << 10) | (unsigned)pk.digit;
        unsigned key1 = key2;
        if ((n & 1) == 0 && kk - pk.cum == 0) {             // rank k is the first of its key: the lower neighbour is another key
            if (pk.dlow >= 0) key1 = (prefix << 10) | (unsigned)pk.dlow;
            else {
                unsigned mx = 0;
                for (int w = 0; w < NT / kWave; w++) mx = s_below[w] > mx ? s_below[w] : mx;
                key1 = mx;
            }
        }
        med = ((double)OrderKey<float>::from(key1) + (double)OrderKey<float>::from(key2)) / 2.0;
        if (final_pass) break;
        const double lo64 = med - sigma * sd, hi64 = med + sigma * sd;
        float lof = (float)lo64, hif = (float)hi64;
        if ((double)lof < lo64) lof = nextafterf(lof, __builtin_inff());
        if ((double)hif > hi64) hif = nextafterf(hif, -__builtin_inff());
        lo_last = lof;
        hi_last = hif;
        lo_run = fmaxf(lo_run, lof);
        hi_run = fminf(hi_run, hif);
        n_prev = n;
    }
    if constexpr (ORIGIN::kOrderedStd) {
        // np.nanstd of the final survivors with numpy's own roundings (the oracle's loop): the sum from +0 in the box's row-major
        // order, mean = sum / n, then the squares of x - mean added in the same order.  The final survivors are the values inside
        // the last bounds [lo_last, hi_last] (the loop left through its final pass).  A chain of at most 2 x 4225 dependent float64
        // additions by the one lane that writes the result: the passes above only feed the clip's bounds, where a tree sum serves.
        if (threadIdx.x == 0 && n > 0) {
            double sum = 0.0;
            for (int e = 0; e < npix; e++) {
                const float x = vals[e];
                if (x >= lo_last && x <= hi_last) sum = sum + (double)x;
            }
            const double mean = sum / (double)n;
            double q = 0.0;
            for (int e = 0; e < npix; e++) {
                const float x = vals[e];
                if (x >= lo_last && x <= hi_last) {
                    const double d = (double)x - mean;
                    q = q + d * d;
                }
            }
            sd = sqrt(q / (double)n);
        }
    }
    if (threadIdx.x == 0) {
        out[4 * box + 0] = med;
        out[4 * box + 1] = sd;
        out[4 * box + 2] = (double)n;
        out[4 * box + 3] = (double)(npix - (n_unmasked < 0 ? 0 : n_unmasked));
    }
}

}  // namespace apgpu
