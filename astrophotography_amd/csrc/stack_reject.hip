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
#include "stack_reject.h"

namespace {
using namespace apgpu;
using namespace apgpu_stack;

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
#include "stack_reject_load.inc"
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

#include "stack_reject_walk.inc"

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
    const apgpu_stack_local *loc = (args->flags & APGPU_STACK_FRAME_LOCAL) ? static_cast<const apgpu_stack_local *>(args->workspace) : nullptr;
    RejectParams prm = reject_params(args, loc);             // (the descriptor on the host: stack_dispatch has checked it)
    prm.maxiters = args->maxiters;
    prm.minmax = (args->flags & APGPU_STACK_REJECT_MINMAX) ? 1 : 0;
    if (prm.minmax) {
        prm.nlow = (int)args->sigma_lower;
        prm.nhigh = (int)args->sigma_upper;
    } else {
        prm.kl = args->sigma_lower;
        prm.kh = args->sigma_upper;
    }
    if (loc) {
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
