// stack_esd.hip - the generalized extreme Studentized deviate test (Rosner 1983) as a rejection rule of the stack.  Selected by
// APGPU_STACK_REJECT_ESD in apgpu_stack_args.flags; one launch, float64 arithmetic; `workspace` is a host apgpu_stack_esd (the
// table of critical values on the device, the mesh descriptor of APGPU_STACK_FRAME_LOCAL).  No contraction: every multiply and
// add below rounds on its own (-ffp-contract=off).
//
// THE DEFINITION (include/apgpu.h; restated for NumPy in tests/stack_esd_model.py).  Per pixel, S = the finite values of the
// column after the calibration or the frame map, widened to float64, n = len(S):
//     K = min(floor(frac * n), n - 3, max_outliers)                 (K <= 0: nothing is removed)
//     y = S ordered by (order key, frame index);  lo, hi = 0, n;  L = H = 0
//     for i in 0 .. K-1:
//         w = y[lo:hi];  m = hi - lo
//         mean = np.add.reduce(w) / m;  d = w - mean;  sd = sqrt(np.add.reduce(d * d) / (m - 1))
//         if not (sd > 0): break
//         dl = (mean - w[0]) / relax;  dh = w[m-1] - mean
//         if dh >= dl: R = dh / sd; hi -= 1     else: R = dl / sd; lo += 1
//         if R > lambda[n][i]: L, H = lo, n - hi
//     survivors = the min/max rule with nlow = L, nhigh = H on S (same ties); outputs as for min/max.
//
// THE KERNEL.  One pixel per lane, one wavefront per workgroup, as stack_reject_kernel, whose pieces (stack_reject.h) it is built
// from.  The lane holds its column twice: v[NP] in FRAME ORDER and compact (what the final statistics are summed from), and
// s[NP], the test's window w in VALUE order - the keys sorted once by a network (stack_sort.h's Batcher list on unsigned
// minima / maxima, NaN slots' keys last), turned back into floats, and parked in LDS (row i = y[i] of every lane; a lane only
// touches its own column: no barrier), where the window's upper end is one read by a per-lane index.  Removing the highest
// value only lowers m; removing the lowest re-reads the window from LDS one row further up.  Every sum - the window's, its
// squared deviations', and the two of the final statistics - is np_pass at ONE site in a rolled loop over a wave-uniform trip
// count (two passes per step, the wavefront's largest K steps, two passes more for the survivors).  Before the final passes
// the lane's (L, H) becomes min/max's membership test: the keys of the last value taken from either end are the two bounds,
// the tie counts come from one walk over v, and `compact` squeezes the survivors, in frame order, into s.  With
// APGPU_STACK_FRAME_PARAMS / APGPU_STACK_FRAME_LOCAL the weighted walk repeats that test on the frames.
//
// The unit is compiled once per raw dtype (-DAPGPU_ESD_RAW=float / uint16_t, -DAPGPU_ESD_ENTRY=launch_esd_f32 / _u16: _build.py),
// so that the two halves of its instances build side by side.
#include "stack_reject.h"

#if !defined(APGPU_ESD_RAW) || !defined(APGPU_ESD_ENTRY)
#error "stack_esd.hip is compiled with -DAPGPU_ESD_RAW=<raw type> -DAPGPU_ESD_ENTRY=<name of its launcher>"
#endif

namespace {
using namespace apgpu;
using namespace apgpu_stack;

struct EsdParams {
    RejectParams r;
    const double *lambda;   // device [N + 1][maxout]
    double frac, relax;
    int maxout;
};

__device__ __forceinline__ void cmpx_key(unsigned &x, unsigned &y)
{
    const unsigned lo = x < y ? x : y, hi = x < y ? y : x;
    x = lo;
    y = hi;
}

template <int NP, int BASE, int... I>
__device__ __forceinline__ void key_net_chunk(unsigned (&u)[NP], std::integer_sequence<int, I...>)
{
    constexpr Net<NP> net = make_net<NP, 1>();
    (cmpx_key(u[net.ce[BASE + I].a], u[net.ce[BASE + I].b]), ...);
}

// Batcher's network (stack_sort.h) on the keys: ascending, the NaN slots' keys (above key(+inf)) last
template <int NP, int BASE = 0>
__device__ __forceinline__ void sort_keys(unsigned (&u)[NP])
{
    constexpr int total = make_net<NP, 1>().n;
    constexpr int CH = 64;
    if constexpr (BASE < total) {
        constexpr int len = (total - BASE < CH) ? total - BASE : CH;
        key_net_chunk<NP, BASE>(u, std::make_integer_sequence<int, len>{});
        sort_keys<NP, BASE + len>(u);
    }
}

template <int NP, typename RawT, bool CALIB, bool FP = false, bool LOC = false>
__global__ __launch_bounds__(64) void stack_esd_kernel(const EsdParams ep)
{
    static_assert(!(CALIB && FP), "fused calibration and frame parameters exclude each other");
    static_assert(!(LOC && (CALIB || FP)), "the local map excludes the fused calibration and the per-frame parameters");
    constexpr bool WT = FP || LOC;                           // the mean is the weighted mean of the survivors
    const RejectParams &prm = ep.r;
    __shared__ float cols[NP * 64];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * 64;
    const int64_t p = base + lane;
    const bool valid = p < prm.P;
    float *const col = cols + lane;
    const int N = prm.N;
    const double inf = __builtin_inf();
    float v[NP], s[NP];
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

    // ---- the test's steps: K of this lane, the wavefront's largest ----
    int K = (int)floor(ep.frac * (double)n);
    K = K < n - 3 ? K : n - 3;
    K = K < ep.maxout ? K : ep.maxout;
    K = K > 0 ? K : 0;
    const int Kmax = wave_max_i(K);
    const int n0max = wave_max_i(n);
    if (Kmax > 0) {                                          // (wave-uniform) the window: sorted once, parked in LDS
        unsigned u[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) u[i] = OrderKey<float>::to(v[i]);
        sort_keys<NP>(u);
#pragma unroll
        for (int i = 0; i < NP; i++) {
            s[i] = i < n ? OrderKey<float>::from(u[i]) : quiet_nan();
            col[i * 64] = s[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < NP; i++) s[i] = v[i];
    }

    const double *const lam = ep.lambda + (int64_t)n * ep.maxout;
    const double relax = ep.relax;
    int lo = 0, m = n;                                       // the window is y[lo .. lo + m), held in s[0 .. m)
    int L = 0, H = 0;                                        // the significant prefix of removals
    unsigned cur_klo = 0, cur_khi = 0xffffffffu;             // keys of the last value taken from either end ...
    unsigned klo = 0, khi = 0xffffffffu;                     // ... as they were at the last significant step
    bool going = K > 0;
    double mean = 0.0, sd = 0.0;
    int nmax = n0max, nmin8 = 0;
    // (FP / LOC) the survivors' membership test as min/max words it, for the weighted walk
    unsigned mm_klo = 0, mm_khi = 0xffffffffu;
    int mm_dlo = 0, mm_keephi = NP + 1;
    bool mm_some = true;
    const double Lo = -inf, Hi = inf;                        // (Winsorized's interval: not used, prm.minmax is set)
    const int trips = 2 * Kmax + 2;                          // two passes per step, two for the survivors
#pragma unroll 1
    for (int t = 0; t < trips; t++) {
        const bool sq = (t & 1) != 0;
        const bool fin = t >= 2 * Kmax;
        if (t == 2 * Kmax) {
            // ---- the survivors: min/max with this lane's (L, H), squeezed into s in frame order ----
            const bool some = n > L + H;                     // (always: K <= n - 3)
            const bool uselo = L > 0, usehi = H > 0;
            int lt = 0, gt = 0, eqhi = 0;
#pragma unroll
            for (int j = 0; j < NP; j += 8) {
                if (j >= n0max) continue;                    // (wave-uniform)
#pragma unroll
                for (int i = j; i < j + 8; i++) {
                    // (v does not change inside the loop: without the barrier its NP keys are formed in front of the loop and
                    // held in registers across it)
                    const unsigned k = OrderKey<float>::to(park_in_vgpr(v[i]));
                    const bool in = i < n;
                    lt += (in && k < klo) ? 1 : 0;
                    gt += (in && k > khi) ? 1 : 0;
                    eqhi += (in && k == khi) ? 1 : 0;
                }
            }
            // of the values equal to the low bound the first dlo go, of those equal to the high bound the last H - gt
            const int dlo = uselo ? L - lt : 0;
            const int keephi = usehi ? eqhi - (H - gt) : NP + 1;
            if (!uselo) klo = 0u;
            if (!usehi) khi = 0xffffffffu;
#pragma unroll
            for (int i = 0; i < NP; i++) s[i] = v[i];
            if (wave_any(L + H > 0)) {
                int seenlo = 0, seenhi = 0;
                const int nn = n;
                m = compact<NP>(s, col, n0max, [&](int i) {
                    const unsigned k = OrderKey<float>::to(s[i]);
                    bool ok = some && i < nn;
                    const bool el = k == klo && uselo, eh = k == khi && usehi;
                    ok = ok && k >= klo && (!el || seenlo >= dlo) && k <= khi && (!eh || seenhi < keephi);
                    seenlo += (el && i < nn) ? 1 : 0;
                    seenhi += (eh && i < nn) ? 1 : 0;
                    return ok;
                });
            } else {
                m = n;
            }
            if constexpr (WT) {                              // (kept for the walk behind the loop)
                mm_klo = klo; mm_khi = khi; mm_dlo = dlo; mm_keephi = keephi; mm_some = some;
            }
        }
        if (!sq) {
            nmax = wave_max_i(m);
            nmin8 = -wave_max_i(-(m > 0 ? (m & ~7) : NP));  // (lanes without data ride along: their sums are not used)
        }
        const double res = np_pass<NP>(s, m, nmin8, nmax, -inf, inf, sq ? mean : 0.0, sq);
        if (!sq) {
            mean = res / (double)m;
            continue;
        }
        if (fin) {
            sd = sqrt(res / (double)m);
            break;
        }
        // ---- one step of the test ----
        const int i = t >> 1;
        const double sdev = sqrt(res / (double)(m - 1));
        const bool mine = going && i < K;
        const bool act = mine && sdev > 0.0;
        if (mine && !act) going = false;
        const float w0 = s[0];
        int top = lo + m - 1;
        top = top < 0 ? 0 : (top > NP - 1 ? NP - 1 : top);
        const float w1 = col[top * 64];
        const double dl = (mean - widen(w0)) / relax, dh = widen(w1) - mean;
        const bool high = dh >= dl;
        const double R = (high ? dh : dl) / sdev;
        const double crit = act ? lam[i] : inf;
        if (act) {
            m -= 1;
            if (high) {
                cur_khi = OrderKey<float>::to(w1);
            } else {
                cur_klo = OrderKey<float>::to(w0);
                lo += 1;
            }
            if (R > crit) {
                L = lo; H = n - (lo + m);
                klo = cur_klo; khi = cur_khi;
            }
        }
        if (wave_any(act && !high)) {                        // a lane's window moved up: read it again from its new start
            const int nm = wave_max_i(m);
#pragma unroll
            for (int j = 0; j < NP; j += 8) {
                if (j >= nm) continue;                       // (wave-uniform)
#pragma unroll
                for (int k = j; k < j + 8; k++) {
                    int r = lo + k;
                    r = r > NP - 1 ? NP - 1 : r;
                    const float x = col[r * 64];
                    s[k] = k < m ? x : quiet_nan();
                }
            }
        }
    }
    n = m;                                                   // the survivors' count

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
int launch_one(const EsdParams &ep, hipStream_t st, char *describe)
{
    if (describe) {
        if (LOC) snprintf(describe, 256, "stack_esd_kernel<%d, %s, false, false, true>", NP, sizeof(RawT) == 2 ? "unsigned short" : "float");
        else if (FP) snprintf(describe, 256, "stack_esd_kernel<%d, %s, false, true>", NP, sizeof(RawT) == 2 ? "unsigned short" : "float");
        else snprintf(describe, 256, "stack_esd_kernel<%d, %s, %s>", NP, sizeof(RawT) == 2 ? "unsigned short" : "float", CALIB ? "true" : "false");
        return APGPU_OK;
    }
    const int64_t grid = (ep.r.P + 63) / 64;
    if (grid > 0x7fffffff) return fail(APGPU_EUNSUPPORTED, "stack (reject): n_pixels = %lld is too many for one launch", (long long)ep.r.P);
    hipLaunchKernelGGL((stack_esd_kernel<NP, RawT, CALIB, FP, LOC>), dim3((unsigned)grid), dim3(64), 0, st, ep);
    return check_launch("stack kernel (esd)");
}

template <typename RawT, bool CALIB, bool FP = false, bool LOC = false>
int launch_slots(const EsdParams &ep, hipStream_t st, char *describe)
{
#define APGPU_ESD_TRY(NP) if (ep.r.N <= NP) return launch_one<NP, RawT, CALIB, FP, LOC>(ep, st, describe);
    APGPU_REJECT_SLOTS(APGPU_ESD_TRY)
#undef APGPU_ESD_TRY
    return fail(APGPU_EUNSUPPORTED, "stack (reject): n_frames = %d exceeds APGPU_STACK_REJECT_MAX = %d", ep.r.N, APGPU_STACK_REJECT_MAX);
}

}  // namespace

namespace apgpu_stack {

// The arguments and the descriptor have been checked by stack_dispatch (stack.hip), which is the only caller and has looked at
// the dtype.
int APGPU_ESD_ENTRY(const apgpu_stack_args *args, hipStream_t st, char *describe)
{
    using RawT = APGPU_ESD_RAW;
    const apgpu_stack_esd *esd = static_cast<const apgpu_stack_esd *>(args->workspace);
    EsdParams ep{};
    ep.r = reject_params(args, esd->local);
    ep.r.minmax = 1;                                         // (the weighted walk's membership test is min/max's)
    ep.lambda = esd->lambda;
    ep.maxout = esd->max_outliers;
    ep.frac = args->sigma_lower;
    ep.relax = args->sigma_upper;
    if (esd->local) return launch_slots<RawT, false, false, true>(ep, st, describe);
    if (args->flags & APGPU_STACK_FRAME_PARAMS) return launch_slots<RawT, false, true>(ep, st, describe);      // (no calibration planes)
    return args->bias != nullptr ? launch_slots<RawT, true>(ep, st, describe) : launch_slots<RawT, false>(ep, st, describe);
}

}  // namespace apgpu_stack
