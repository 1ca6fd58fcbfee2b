// stack_reject.h - what the rejection rules of the stack share (stack_reject.hip: Winsorized clipping and min/max rejection;
// stack_esd.hip: the generalized ESD test): the kernel arguments, the slot counts, the compact column and its squeeze through
// LDS, the rank selection on keys, numpy's sum as one pass, the per-frame and the local map, the kernel arguments filled from a
// call's.  The column load and the weighted walk are the fragments stack_reject_load.inc and stack_reject_walk.inc.  Everything
// is written once; both units include it.  No contraction: every multiply and add rounds on its own.
#pragma once
#include "stack_reduce.h"
#include "np_exact.h"

namespace {
using namespace apgpu;
using namespace apgpu_stack;

struct RejectParams {
    const void *frames;
    const float *bias, *dark, *nflat, *exp_ratio, *pedestal;
    const uint8_t *pixmask;
    float *mean, *std;
    int32_t *count;
    double *mean64, *std64;
    int64_t P, stride;
    double kl, kh;          // Winsorized: sigma_lower, sigma_upper
    int N, still_biased, maxiters;
    int minmax, nlow, nhigh;
    // APGPU_STACK_FRAME_LOCAL (behind everything older: the other instances' arguments keep their places)
    const float *lscale, *loffset, *lweight;                // meshes [N][ny][nx] (lscale may be NULL = 1), weights [N] or NULL = 1
    int64_t width, row0;                                     // pixel p is image row row0 + p / width, column p % width
    int bh, bw, ny, nx;                                      // box size, mesh shape
};

constexpr int kWinsorMaxInner = APGPU_STACK_WINSOR_MAX_INNER;

// THE SLOT COUNTS of the reject kernel, written once (multiples of 8).  A stack between two counts runs the next one: every
// loop over the column skips the blocks of 8 slots above the wavefront's largest n (a scalar branch per block - per SLOT it
// cost the float64 chains of neighbouring slots their overlap: 3 x the time), so unused slots cost registers, not time.
#define APGPU_REJECT_SLOTS(X) X(8) X(16) X(32) X(64) X(128)

__device__ __forceinline__ int wave_max_i(int x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int y = __shfl_xor(x, off, 64);
        x = y > x ? y : x;
    }
    return __builtin_amdgcn_readfirstlane(x);
}

// Squeezes the column: the elements keep(i) accepts, in order, to the front; NaN behind them.  Returns their number.
template <int NP, typename K>
__device__ __forceinline__ int compact(float (&v)[NP], float *col, int nmax, K keep)
{
    int pos = 0;
#pragma unroll
    for (int j = 0; j < NP; j += 8) {
        if (j >= nmax) continue;                             // (wave-uniform: whole blocks of 8 slots no lane uses are skipped)
#pragma unroll
        for (int i = j; i < j + 8; i++) {
            if (keep(i)) {
                col[pos * 64] = v[i];
                pos++;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NP; j += 8) {
        if (j >= nmax) continue;
#pragma unroll
        for (int i = j; i < j + 8; i++) {
            const float x = col[i * 64];
            v[i] = i < pos ? x : quiet_nan();
        }
    }
    return pos;
}

// The value of rank k (0-based, k < n) among v[0 .. n) in float order (-0 == +0; NaN slots never count): the largest key T with
// #(x < from(T)) <= k, built from the top bit down.  T stays below key(+inf) (that count is n > k), so from(T) is never a NaN.
template <int NP>
__device__ __forceinline__ float select_rank(const float (&v)[NP], int k, int nmax)
{
    unsigned T = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; bit--) {
        const unsigned cand = T | (1u << bit);
        const float c = OrderKey<float>::from(cand);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < NP; j += 8) {
            if (j >= nmax) continue;
#pragma unroll
            for (int i = j; i < j + 8; i++) cnt += v[i] < c ? 1 : 0;
        }
        T = cnt <= k ? cand : T;
    }
    return OrderKey<float>::from(T);
}

// the same on keys (u[i] = OrderKey of v[i]; the NaN slots' keys lie above key(+inf))
template <int NP>
__device__ __forceinline__ unsigned select_rank_key(const unsigned (&u)[NP], int k, int nmax)
{
    unsigned T = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; bit--) {
        const unsigned cand = T | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < NP; j += 8) {
            if (j >= nmax) continue;
#pragma unroll
            for (int i = j; i < j + 8; i++) cnt += u[i] < cand ? 1 : 0;
        }
        T = cnt <= k ? cand : T;
    }
    return T;
}

// np.median of v[0 .. n), n >= 1: the two middle values summed from +0 and halved
template <int NP>
__device__ __forceinline__ double median_of(const float (&v)[NP], int n, int nmax)
{
    const float m2 = select_rank<NP>(v, n >> 1, nmax);
    float m1 = m2;
    if (wave_any((n & 1) == 0)) {
        // the lower middle value (rank n / 2 - 1): the largest value below m2 when exactly n / 2 values are below it,
        // else m2 once more (a tie across the middle)
        int below = 0;
        float mx = -__builtin_inff();
#pragma unroll
        for (int j = 0; j < NP; j += 8) {
            if (j >= nmax) continue;
#pragma unroll
            for (int i = j; i < j + 8; i++) {
                const bool lt = v[i] < m2;
                below += lt ? 1 : 0;
                mx = lt ? __builtin_fmaxf(mx, v[i]) : mx;
            }
        }
        if ((n & 1) == 0 && below == (n >> 1)) m1 = mx;
    }
    return ((0.0 + (double)m1) + (double)m2) / 2.0;
}

// ONE numpy-ordered sum over the lane's column: term i = g(v[i]), g(x) = min(max(x, clo), chi) - m, squared if sq (wave-uniform).
// n8 = n - n % 8; nmin8 / nmax (wave-uniform): the smallest n8 and the largest n of the wavefront - below nmin8 every lane adds
// term i to accumulator i % 8, at or above nmax no lane has a term.  -0.0 is the identity of a rounded add (x + -0.0 == x for
// every x, zeros of both signs included), so an accumulator that starts there IS its first term, and a tail slot that holds it
// adds nothing.
template <int NP>
__device__ __forceinline__ double np_pass(const float (&v)[NP], int n, int nmin8, int nmax, double clo, double chi, double m, bool sq)
{
    const int n8 = n & ~7;
    double r[8], tl[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        r[k] = -0.0;
        tl[k] = -0.0;
    }
#pragma unroll
    for (int j = 0; j < NP; j += 8) {                        // a block = one term for each accumulator
        if (j >= nmax) continue;                             // (wave-uniform)
        double t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) t[k] = __builtin_fmin(__builtin_fmax(widen(v[j + k]), clo), chi) - m;
        if (sq) {                                            // (wave-uniform)
#pragma unroll
            for (int k = 0; k < 8; k++) t[k] = t[k] * t[k];
        }
        if (j + 8 <= nmin8) {                                // (wave-uniform) every lane's block of accumulator terms
#pragma unroll
            for (int k = 0; k < 8; k++) r[k] = r[k] + t[k];
        } else {
            const bool acc = j < n8, last = j == n8;         // n8 is a multiple of 8: a block is all accumulator terms, or the tail
#pragma unroll
            for (int k = 0; k < 8; k++) {
                r[k] = r[k] + (acc ? t[k] : -0.0);
                tl[k] = (last && j + k < n) ? t[k] : tl[k];
            }
        }
    }
    double res = n >= 8 ? ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])) : 0.0;
#pragma unroll
    for (int k = 0; k < 7; k++) res = res + tl[k];
    return 0.0 + res;                                        // np.add.reduce folds its pieces from +0: a sum of -0s is +0
}

// v = float32(float32(a x) + b): the map of APGPU_STACK_FRAME_PARAMS, each operation rounded on its own
__device__ __forceinline__ float frame_map(float x, float a, float b) { return __fadd_rn(__fmul_rn(a, x), b); }

// APGPU_STACK_FRAME_LOCAL: where a pixel coordinate c lies between the box centres (j + 0.5) b - 0.5 of a mesh axis of m cells:
// the lower cell j0, the upper one j1 (the same cell beyond the outer centres and on a one-cell axis) and the fraction t.  Whole
// numbers throughout (c < 2^30, b <= 32768: stack_dispatch has seen to it), one IEEE division of two exactly held values.
__device__ __forceinline__ void mesh_axis(int c, int b, int m, int &j0, int &j1, float &t)
{
    const int u = 2 * c + 1 - b, b2 = 2 * b;                 // u > -2 b: floor(u / 2b) is -1 for a negative u, clamped to 0
    const int top = m >= 2 ? m - 2 : 0;
    const int q = u < 0 ? 0 : u / b2;
    j0 = q < top ? q : top;
    j1 = j0 + 1 < m ? j0 + 1 : m - 1;
    int r = u - b2 * j0;
    r = r < 0 ? 0 : (r > b2 ? b2 : r);
    t = __fdiv_rn((float)r, (float)b2);
}

// a lane's place in the meshes: the four corners' indices inside a frame's [ny][nx] mesh and the two fractions
struct MeshCell {
    int i00, i01, i10, i11;
    float tx, ty;
};

// m(y, x) = top + ty (bot - top), top = M[j0][k0] + tx (M[j0][k1] - M[j0][k0]), bot the same on row j1: every operation rounds
__device__ __forceinline__ float mesh_value(const float *M, const MeshCell &c)
{
    const float m00 = M[c.i00], m01 = M[c.i01], m10 = M[c.i10], m11 = M[c.i11];
    const float top = __fadd_rn(m00, __fmul_rn(c.tx, __fsub_rn(m01, m00)));
    const float bot = __fadd_rn(m10, __fmul_rn(c.tx, __fsub_rn(m11, m10)));
    return __fadd_rn(top, __fmul_rn(c.ty, __fsub_rn(bot, top)));
}

// v = float32(float32(a(y,x) x) + b(y,x)) of frame f; without a scale mesh v = float32(x + b), the bits a mesh of ones gives.
// The one place the local map is formed: the first load and the weighted walk both come through here.
__device__ __forceinline__ float local_map(float x, const float *lscale, const float *loffset, int64_t cells, int f, const MeshCell &c)
{
    const float b = mesh_value(loffset + f * cells, c);
    if (lscale) x = __fmul_rn(mesh_value(lscale + f * cells, c), x);      // (wave-uniform)
    return __fadd_rn(x, b);
}

// The kernel arguments from the call's (stack_dispatch has checked them); loc: the descriptor of APGPU_STACK_FRAME_LOCAL or NULL.
// The rule's own parameters (kl / kh / maxiters, minmax / nlow / nhigh) are the caller's to fill.
inline RejectParams reject_params(const apgpu_stack_args *args, const apgpu_stack_local *loc)
{
    RejectParams prm{};
    prm.frames = args->frames;
    prm.bias = args->bias;
    prm.dark = args->dark;
    prm.nflat = args->nflat;
    prm.exp_ratio = args->exp_ratio;
    prm.pedestal = args->pedestal;
    prm.pixmask = args->pixmask;
    prm.mean = args->mean;
    prm.std = args->std;
    prm.count = args->count;
    prm.mean64 = args->mean_f64;
    prm.std64 = args->std_f64;
    prm.P = args->n_pixels;
    prm.stride = args->frame_stride > 0 ? args->frame_stride : args->n_pixels;
    prm.N = args->n_frames;
    prm.still_biased = args->dark_still_biased;
    if (loc) {
        prm.lscale = loc->scale;
        prm.loffset = loc->offset;
        prm.lweight = loc->weight;
        prm.width = loc->width;
        prm.row0 = loc->row0;
        prm.bh = loc->box_height;
        prm.bw = loc->box_width;
        prm.ny = loc->ny;
        prm.nx = loc->nx;
    }
    return prm;
}

}  // namespace
