// stack_reject.hip - the two rejection rules of small stacks (5 .. 30 registered light frames, where an outlier inflates the
// very standard deviation a sigma clip judges it by): Winsorized sigma clipping and min/max rejection.  Selected by
// APGPU_STACK_REJECT_WINSORIZED / APGPU_STACK_REJECT_MINMAX in apgpu_stack_args.flags; one launch, float64 arithmetic, no
// workspace.  No contraction: every multiply and add below rounds on its own (-ffp-contract=off).
//
// THE DEFINITION (include/apgpu.h; restated for NumPy in tests/stack_reject_model.py).  Per pixel, S = the finite values of
// the column after the optional calibration (a float32 value as stack_calibrate.h forms it), widened to float64, in frame
// order.  A masked pixel or an empty S gives NaN (0x7fc00000) and count 0.
//   Winsorized (kl = sigma_lower, kh = sigma_upper; maxiters rounds, < 0: until a round removes nothing):
//     round:  n = len(S); if n < 3: stop
//             med = np.median(S); sig = np.std(S)                   (ddof 0, numpy's summation order: np_exact.h)
//             repeat at most APGPU_STACK_WINSOR_MAX_INNER = 16 times:
//                 W  = min(max(S, med - 1.5 sig), med + 1.5 sig)    (clamped from S each time, never from the previous W)
//                 s0 = sig; sig = 1.134 np.std(W)
//                 if |sig - s0| <= 0.0005 s0: break
//             keep x with med - kl sig <= x <= med + kh sig         (inclusive)
//             if nothing was removed: stop;  S = the kept values, still in frame order
//   Min/max (nlow = sigma_lower, nhigh = sigma_upper, whole numbers): order S by (OrderKey of the value, frame index), drop the
//     first nlow and the last nhigh; n <= nlow + nhigh leaves nothing.
//   Outputs over the survivors in frame order: count = m, mean_f64 = np.add.reduce(surv) / m, std_f64 = np.std(surv), mean and
//   std those values rounded once to float32.
//   APGPU_STACK_FRAME_PARAMS (exp_ratio = float32 [3][N]: scale a, offset b, weight w; no calibration): the column is
//   v = float32(float32(a_i x) + b_i), the rule runs on the finite v, count and std_f64 as above (unweighted), and
//   mean_f64 = num / den, num += double(w_k) double(v_k), den += double(w_k) over the survivors in frame order from +0.0.
//   APGPU_STACK_FRAME_LOCAL (workspace = a host apgpu_stack_local; no calibration, no exp_ratio): a and b are per-frame MESHES, one
//   value per box, read off bilinearly at the pixel (mesh_axis, mesh_value, local_map below); everything behind v is as above.
//
// THE KERNEL.  One pixel per lane, one wavefront per workgroup, the column v[NP] in VGPRs IN FRAME ORDER and COMPACT: v[0 .. n)
// are the lane's current S, v[n .. NP) are NaN.  numpy's sum of n <= 128 terms puts term i into accumulator i % 8 (i < n - n % 8)
// or adds it to the folded accumulators as one of the n % 8 last terms - with a compact column both places are known from the
// static index i and the lane's n, so a lane whose n differs from its neighbours' needs selects, not a different instruction
// stream.  What a round rejects is squeezed out through LDS (NP x 64 floats: row i = element i of every lane, a lane only ever
// touches its own column, so there is no barrier): written at the lane's running count, read back by static index.
// Every sum of the rule - S, (S - mean)^2, W, (W - mean)^2 and the final statistics - is ONE pass (np_pass: clamp, subtract,
// optionally square, add in numpy's order) at ONE site inside a rolled loop over a wave-uniform step, so the NP-times unrolled
// body exists once per kernel.  Lanes that have finished a loop ride along: their state is not updated.  The wavefront leaves
// the inner loop when its last lane has converged and a round when no lane removed anything - that divergence is what the
// kernel's time depends on.  The median is a bisection over the 32 key bits on float compares (two instructions
// per value and bit, no second copy of the column); min/max selects its two bounds the same way on the keys themselves, where
// -0 sorts below +0 as the definition wants.
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

// FP: APGPU_STACK_FRAME_PARAMS - prm.exp_ratio is float32 [3][N] = scale a, offset b, weight w of every frame; the column is
// v = a x + b (two roundings) and the mean is the weighted mean of the survivors (see the end).  No calibration then.
// LOC: APGPU_STACK_FRAME_LOCAL - a and b are read off per-frame meshes at the lane's pixel (local_map), the weights are
// prm.lweight; everything behind the map is FP's.
template <int NP, typename RawT, bool CALIB, bool FP = false, bool LOC = false>
__global__ __launch_bounds__(64) void stack_reject_kernel(const RejectParams prm)
{
    static_assert(!(CALIB && FP), "fused calibration and frame parameters exclude each other");
    static_assert(!(LOC && (CALIB || FP)), "the local map excludes the fused calibration and the per-frame parameters");
    constexpr bool WT = FP || LOC;                           // the mean is the weighted mean of the survivors
    __shared__ float cols[NP * 64];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * 64;
    const int64_t p = base + lane;
    const bool valid = p < prm.P;
    float *const col = cols + lane;
    const int N = prm.N;
    const double inf = __builtin_inf();
    float v[NP];
    MeshCell cell{};
    int64_t cells = 0;
    if constexpr (LOC) {                                     // (a lane behind the last pixel takes the block's first one)
        const int64_t q = base + (valid ? lane : 0);
        const int64_t row = q / prm.width;
        const int y = (int)(prm.row0 + row), x = (int)(q - row * prm.width);
        int j0, j1, k0, k1;
        mesh_axis(y, prm.bh, prm.ny, j0, j1, cell.ty);
        mesh_axis(x, prm.bw, prm.nx, k0, k1, cell.tx);
        cell.i00 = j0 * prm.nx + k0; cell.i01 = j0 * prm.nx + k1;
        cell.i10 = j1 * prm.nx + k0; cell.i11 = j1 * prm.nx + k1;
        cells = (int64_t)prm.ny * prm.nx;
    }

    // ---- the column: load, calibrate (stack_calibrate.h, load_column_exact: IEEE division, one value at a time) ----
    {
        const int off = valid ? lane : 0;
        float b = 0.f, D = 0.f, nf = 1.f;
        bool dodiv = false;
        if constexpr (CALIB) {
            b = prm.bias[base + off];
            const float d = prm.dark[base + off];
            D = prm.still_biased ? d - b : d;                // ApCalibrate.py:440-445
            if (prm.nflat) {
                nf = prm.nflat[base + off];
                dodiv = (nf != 0.f);                         // ApCalibrate.py:462 (NaN != 0 is True)
            }
        }
        const RawT *const fb = static_cast<const RawT *>(prm.frames) + base + off;
#pragma unroll
        for (int j = 0; j < NP; j += 8) {                    // blocks of 8 frames: eight loads in flight, one branch
            if (j >= N) {                                    // (wave-uniform)
#pragma unroll
                for (int k = 0; k < 8; k++) v[j + k] = quiet_nan();
                continue;
            }
            RawT raw[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int f = j + k < N ? j + k : N - 1;     // slots behind the last frame re-read it and are then dropped
                raw[k] = fb[(int64_t)f * prm.stride];
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int f = j + k < N ? j + k : N - 1;
                float x = to_f32(raw[k]);
                if constexpr (CALIB) {
                    const float e = prm.exp_ratio[f];
                    const float ped = prm.pedestal ? prm.pedestal[f] : 0.f;
                    if (ped != 0.f) x = x + ped;             // ApCalibrate.py:318-326
                    x = x - b;                               // :439
                    const float ds = e * D;                  // :450
                    x = x - ds;                              // :451
                    if (dodiv) x = __fdiv_rn(x, nf);         // :463
                }
                if constexpr (FP) x = frame_map(x, prm.exp_ratio[f], prm.exp_ratio[N + f]);
                if constexpr (LOC) x = local_map(x, prm.lscale, prm.loffset, cells, f, cell);
                v[j + k] = j + k < N ? x : quiet_nan();
            }
        }
    }
    const bool skip = !valid || (prm.pixmask && prm.pixmask[p]);
    int n;
    {
        int nfin = 0;
#pragma unroll
        for (int i = 0; i < NP; i++) nfin += is_finite(v[i]) ? 1 : 0;      // (slots from N on hold NaN)
        n = skip ? 0 : nfin;
        if (wave_any(n != N)) n = compact<NP>(v, col, N, [&](int i) { return !skip && is_finite(v[i]); });
    }

    // ---- min/max: the bounds are the keys of rank nlow - 1 and n - nhigh; equal keys go by frame index ----
    // (FP) the membership test of the rule, kept for the weighted walk over the frames at the end: min/max - the two key bounds
    // and the tie counts; Winsorized - the intersection [Lo, Hi] of the rounds' intervals
    unsigned mm_klo = 0, mm_khi = 0xffffffffu;               // (an end the rule does not trim: bounds and counts no value fails)
    int mm_dlo = 0, mm_keephi = NP + 1;
    bool mm_some = true;
    double Lo = -inf, Hi = inf;
    if (prm.minmax) {
        const int nlow = prm.nlow, nhigh = prm.nhigh;
        const int nmax = wave_max_i(n);
        if (nlow + nhigh > 0 && nmax > 0) {
            unsigned u[NP];
#pragma unroll
            for (int i = 0; i < NP; i++) u[i] = OrderKey<float>::to(v[i]);
            const bool some = n > nlow + nhigh;
            // (lanes with nothing to select pass rank 0: their result is not used)
            const unsigned klo = select_rank_key<NP>(u, (some && nlow > 0) ? nlow - 1 : 0, nmax);
            const unsigned khi = select_rank_key<NP>(u, (some && nhigh > 0) ? n - nhigh : 0, nmax);
            int lt = 0, gt = 0, eqhi = 0;
#pragma unroll
            for (int j = 0; j < NP; j += 8) {
                if (j >= nmax) continue;
#pragma unroll
                for (int i = j; i < j + 8; i++) {
                    const bool in = i < n;
                    lt += (in && u[i] < klo) ? 1 : 0;
                    gt += (in && u[i] > khi) ? 1 : 0;
                    eqhi += (in && u[i] == khi) ? 1 : 0;
                }
            }
            // of the values equal to the low bound the first dlo go, of those equal to the high bound the last nhigh - gt
            const int dlo = nlow > 0 ? nlow - lt : 0;
            const int keephi = nhigh > 0 ? eqhi - (nhigh - gt) : NP + 1;
            const bool uselo = nlow > 0, usehi = nhigh > 0;
            if constexpr (WT) {
                mm_klo = uselo ? klo : 0u; mm_khi = usehi ? khi : 0xffffffffu;
                mm_dlo = dlo; mm_keephi = keephi; mm_some = some;
            }
            int seenlo = 0, seenhi = 0;
            const int nn = n;
            n = compact<NP>(v, col, nmax, [&](int i) {
                const unsigned k = u[i];
                bool ok = some && i < nn;
                if (uselo) {
                    const bool e = k == klo;
                    ok = ok && k >= klo && (!e || seenlo >= dlo);
                    seenlo += (e && i < nn) ? 1 : 0;
                }
                if (usehi) {
                    const bool e = k == khi;
                    ok = ok && k <= khi && (!e || seenhi < keephi);
                    seenhi += (e && i < nn) ? 1 : 0;
                }
                return ok;
            });
        }
    }

    // ---- the rounds, the inner steps and the final statistics: one pass site, a wave-uniform step ----
    enum { kRound = 0, kSumS, kSqS, kSumW, kSqW, kFinalSum, kFinalSq };
    const double kl = prm.kl, kh = prm.kh;
    const int maxiters = prm.maxiters;
    bool active = !prm.minmax && n >= 3;                     // the lane has a round to run
    bool fresh = false;                                      // mean / sd are those of the lane's current S
    bool inner_active = false;
    int iters = 0, inner = 0;
    int step = kRound, nmax = 0, nmin8 = 0;
    double med = 0.0, sig = 0.0, mean = 0.0, sd = 0.0;
    double clo = -inf, chi = inf, m = 0.0;
    bool sq = false;
#pragma unroll 1
    for (;;) {
        if (step == kRound) {
            nmax = wave_max_i(n);
            nmin8 = -wave_max_i(-(n > 0 ? (n & ~7) : NP));      // (lanes without data ride along: their sums are not used)
            clo = -inf; chi = inf; m = 0.0; sq = false;
            if (wave_any(active)) {
                med = median_of<NP>(v, n > 0 ? n : 1, nmax);
                step = kSumS;
            } else {
                if (!wave_any(!fresh && n > 0)) break;
                step = kFinalSum;
            }
        }
        const double res = np_pass<NP>(v, n, nmin8, nmax, clo, chi, m, sq);
        const double nd = (double)n;
        if (step == kSumS || step == kFinalSum) {
            mean = res / nd;
            m = mean; sq = true;
            step = step == kSumS ? kSqS : kFinalSq;
        } else if (step == kSqS) {
            sd = sqrt(res / nd);
            fresh = true;
            sig = sd;
            inner = 0;
            inner_active = active;
            clo = med - 1.5 * sig; chi = med + 1.5 * sig; m = 0.0; sq = false;
            step = kSumW;
        } else if (step == kSumW) {
            m = res / nd; sq = true;
            step = kSqW;
        } else if (step == kSqW) {
            if (inner_active) {
                const double s0 = sig;
                sig = 1.134 * sqrt(res / nd);
                inner++;
                if (__builtin_fabs(sig - s0) <= 0.0005 * s0 || inner >= kWinsorMaxInner) inner_active = false;
            }
            if (wave_any(inner_active)) {
                clo = med - 1.5 * sig; chi = med + 1.5 * sig; m = 0.0; sq = false;
                step = kSumW;
            } else {
                // the clip of this round (lanes without a round keep everything)
                const double lo = active ? med - kl * sig : -inf, hi = active ? med + kh * sig : inf;
                if constexpr (WT) {                          // (a lane without a round has -inf / +inf: no change)
                    Lo = !(lo <= Lo) ? lo : Lo;              // (a NaN bound - sigma = inf on a constant column - keeps
                    Hi = !(hi >= Hi) ? hi : Hi;              //  nothing, here as in the round)
                }
                int kept = 0;
#pragma unroll
                for (int j = 0; j < NP; j += 8) {
                    if (j >= nmax) continue;
#pragma unroll
                    for (int i = j; i < j + 8; i++) {
                        const double x = widen(v[i]);
                        kept += (i < n && x >= lo && x <= hi) ? 1 : 0;
                    }
                }
                const bool removed = kept != n;
                if (wave_any(removed)) {
                    const int nn = n;
                    n = compact<NP>(v, col, nmax, [&](int i) {
                        const double x = widen(v[i]);
                        return i < nn && x >= lo && x <= hi;
                    });
                }
                if (removed) fresh = false;
                iters++;
                active = active && removed && n >= 3 && (maxiters < 0 || iters < maxiters);
                step = kRound;
            }
        } else {                                             // kFinalSq
            sd = sqrt(res / nd);
            fresh = true;
            break;
        }
    }

    // ---- (FP) the weighted mean.  The compact column has lost its frame indices, so the frames are walked once more from memory
    // (the kernel is bound by its arithmetic many times over): v is formed again, the rule's membership test is
    // repeated on it - Winsorized: finite and inside [Lo, Hi], for a removed value lies outside its round's interval and a kept one
    // inside every round's; min/max: the two key bounds and the tie counters over the finite values in frame order, as the
    // compaction above counted them - and num += double(w) double(v), den += double(w) run in frame order from +0.
    if constexpr (WT) {
        const int off = valid ? lane : 0;
        const RawT *const fb = static_cast<const RawT *>(prm.frames) + base + off;
        const bool mm = prm.minmax != 0;
        double num = 0.0, den = 0.0;
        int seenlo = 0, seenhi = 0;
        constexpr int B = 8;                                 // frames per block: eight loads in flight, as on the first load
#pragma unroll 1
        for (int j = 0; j < N; j += B) {
            RawT raw[B];
#pragma unroll
            for (int k = 0; k < B; k++) {
                const int f = j + k < N ? j + k : N - 1;
                raw[k] = fb[(int64_t)f * prm.stride];
            }
#pragma unroll
            for (int k = 0; k < B; k++) {
                const int f = j + k < N ? j + k : N - 1;
                float x, w;
                if constexpr (LOC) {
                    x = local_map(to_f32(raw[k]), prm.lscale, prm.loffset, cells, f, cell);
                    w = prm.lweight ? prm.lweight[f] : 1.f;
                } else {
                    x = frame_map(to_f32(raw[k]), prm.exp_ratio[f], prm.exp_ratio[N + f]);
                    w = prm.exp_ratio[2 * N + f];
                }
                const bool fin = j + k < N && is_finite(x);
                bool ok;
                if (mm) {                                    // (wave-uniform)
                    const unsigned key = OrderKey<float>::to(x);
                    const bool elo = key == mm_klo, ehi = key == mm_khi;
                    ok = fin && mm_some && key >= mm_klo && (!elo || seenlo >= mm_dlo) && key <= mm_khi && (!ehi || seenhi < mm_keephi);
                    seenlo += (elo && fin) ? 1 : 0;
                    seenhi += (ehi && fin) ? 1 : 0;
                } else {
                    const double xd = widen(x);
                    ok = fin && xd >= Lo && xd <= Hi;
                }
                const double wd = widen(w);
                const double t = wd * widen(x);              // (exact: two widened float32 values)
                num = ok ? num + t : num;
                den = ok ? den + wd : den;
            }
        }
        mean = num / den;
    }

    if (valid) {
        const bool any = n > 0;
        const double nan64 = __builtin_nan("");
        if (prm.mean) prm.mean[p] = any ? (float)mean : quiet_nan();
        if (prm.std) prm.std[p] = any ? (float)sd : quiet_nan();
        if (prm.count) prm.count[p] = n;
        if (prm.mean64) prm.mean64[p] = any ? mean : nan64;
        if (prm.std64) prm.std64[p] = any ? sd : nan64;
    }
}

template <int NP, typename RawT, bool CALIB, bool FP, bool LOC>
int launch_one(const RejectParams &prm, hipStream_t st, char *describe)
{
    if (describe) {
        if (LOC) snprintf(describe, 256, "stack_reject_kernel<%d, %s, false, false, true>", NP, sizeof(RawT) == 2 ? "unsigned short" : "float");
        else if (FP) snprintf(describe, 256, "stack_reject_kernel<%d, %s, false, true>", NP, sizeof(RawT) == 2 ? "unsigned short" : "float");
        else snprintf(describe, 256, "stack_reject_kernel<%d, %s, %s>", NP, sizeof(RawT) == 2 ? "unsigned short" : "float", CALIB ? "true" : "false");
        return APGPU_OK;
    }
    const int64_t grid = (prm.P + 63) / 64;
    if (grid > 0x7fffffff) return fail(APGPU_EUNSUPPORTED, "stack (reject): n_pixels = %lld is too many for one launch", (long long)prm.P);
    hipLaunchKernelGGL((stack_reject_kernel<NP, RawT, CALIB, FP, LOC>), dim3((unsigned)grid), dim3(64), 0, st, prm);
    return check_launch("stack kernel (reject)");
}

template <typename RawT, bool CALIB, bool FP = false, bool LOC = false>
int launch_slots(const RejectParams &prm, hipStream_t st, char *describe)
{
#define APGPU_REJECT_TRY(NP) if (prm.N <= NP) return launch_one<NP, RawT, CALIB, FP, LOC>(prm, st, describe);
    APGPU_REJECT_SLOTS(APGPU_REJECT_TRY)
#undef APGPU_REJECT_TRY
    return fail(APGPU_EUNSUPPORTED, "stack (reject): n_frames = %d exceeds APGPU_STACK_REJECT_MAX = %d", prm.N, APGPU_STACK_REJECT_MAX);
}

}  // namespace

namespace apgpu_stack {

// The arguments have been checked by stack_dispatch (stack.hip), which is the only caller.
int launch_reject(const apgpu_stack_args *args, hipStream_t st, char *describe)
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
    prm.maxiters = args->maxiters;
    prm.minmax = (args->flags & APGPU_STACK_REJECT_MINMAX) ? 1 : 0;
    if (prm.minmax) {
        prm.nlow = (int)args->sigma_lower;
        prm.nhigh = (int)args->sigma_upper;
    } else {
        prm.kl = args->sigma_lower;
        prm.kh = args->sigma_upper;
    }
    if (args->flags & APGPU_STACK_FRAME_LOCAL) {             // (the descriptor on the host: stack_dispatch has checked it)
        const apgpu_stack_local *loc = static_cast<const apgpu_stack_local *>(args->workspace);
        prm.lscale = loc->scale;
        prm.loffset = loc->offset;
        prm.lweight = loc->weight;
        prm.width = loc->width;
        prm.row0 = loc->row0;
        prm.bh = loc->box_height;
        prm.bw = loc->box_width;
        prm.ny = loc->ny;
        prm.nx = loc->nx;
        return args->dtype == APGPU_F32 ? launch_slots<float, false, false, true>(prm, st, describe)
                                        : launch_slots<uint16_t, false, false, true>(prm, st, describe);
    }
    if (args->flags & APGPU_STACK_FRAME_PARAMS)              // (no calibration planes: stack_dispatch has seen to it)
        return args->dtype == APGPU_F32 ? launch_slots<float, false, true>(prm, st, describe) : launch_slots<uint16_t, false, true>(prm, st, describe);
    const bool calib = args->bias != nullptr;
    if (args->dtype == APGPU_F32) return calib ? launch_slots<float, true>(prm, st, describe) : launch_slots<float, false>(prm, st, describe);
    return calib ? launch_slots<uint16_t, true>(prm, st, describe) : launch_slots<uint16_t, false>(prm, st, describe);
}

}  // namespace apgpu_stack
