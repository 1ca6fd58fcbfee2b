// F8: star-list frame registration (include/apgpu.h F8; restated in tests/register_model.py).
//   triangle_build_kernel  the similarity invariants of every triple among the K brightest stars of each frame
//   triangle_vote_kernel   reference x frame triangle pairs within eps -> votes for their three vertex pairs
//   nearest_match_kernel   nearest neighbour under a per-frame map (an affine, or the polynomial of DESIGN 4.3e'), both directions
// All float64, no contraction (-ffp-contract=off): every expression rounds as the NumPy model's does.
#include "common.h"
#include "distortion_core.h"

namespace apgpu {
namespace {

constexpr int kRegMaxK = APGPU_REGISTER_MAX_K;
constexpr int kRegMaxStars = APGPU_REGISTER_MAX_STARS;
constexpr int kRegBlock = 256;

__device__ __forceinline__ double dist2(double2 a, double2 b)
{
    const double dx = a.x - b.x, dy = a.y - b.y;
    return dx * dx + dy * dy;
}

// One thread per (i, j, k) of the K^3 cube; the threads with i < j < k < n hold a triangle.  The kept ones go through a per-frame
// counter into a list in no particular order.  A triangle's packed word: v0 | v1 << 8 | v2 << 16 | (orientation + 1) << 24.
__global__ __launch_bounds__(kRegBlock) void triangle_build_kernel(const double *__restrict__ xy, const int *__restrict__ count, int M,
                                                                   int K, int tcap, double min_side2, double *__restrict__ tri_xy,
                                                                   int *__restrict__ tri_v, int *__restrict__ ntri)
{
    const int f = blockIdx.y;
    const int n = min(min(count[f], K), M);
    const int t = blockIdx.x * kRegBlock + threadIdx.x;
    const int i = t / (K * K), j = (t / K) % K, k = t % K;
    if (!(i < j && j < k && k < n)) return;
    const double2 *p = reinterpret_cast<const double2 *>(xy) + (size_t)f * M;
    const double2 pi = p[i], pj = p[j], pk = p[k];
    // the side opposite each vertex, in vertex order; a stable descending sort (a swap only on strictly less)
    double s0 = dist2(pj, pk), s1 = dist2(pi, pk), s2 = dist2(pi, pj), ts;
    int o0 = i, o1 = j, o2 = k, to;
    if (s0 < s1) { ts = s0; s0 = s1; s1 = ts; to = o0; o0 = o1; o1 = to; }
    if (s1 < s2) { ts = s1; s1 = s2; s2 = ts; to = o1; o1 = o2; o2 = to; }
    if (s0 < s1) { ts = s0; s0 = s1; s1 = ts; to = o0; o0 = o1; o1 = to; }
    const double a2 = s0, b2 = s1, c2 = s2;
    const int v2 = o0, v1 = o1, v0 = o2;                    // opposite the longest, the middle and the shortest side
    const double x = sqrt(b2 / a2), y = sqrt(c2 / a2);
    if (!(c2 >= min_side2 && y >= 0.1 && x <= 0.98 && y <= 0.98 * x)) return;
    const double2 q0 = v0 == i ? pi : (v0 == j ? pj : pk);
    const double2 q1 = v1 == i ? pi : (v1 == j ? pj : pk);
    const double2 q2 = v2 == i ? pi : (v2 == j ? pj : pk);
    const double cross = (q1.x - q0.x) * (q2.y - q0.y) - (q1.y - q0.y) * (q2.x - q0.x);
    const int orient = cross > 0.0 ? 1 : (cross < 0.0 ? -1 : 0);
    const int slot = atomicAdd(&ntri[f], 1);
    if (slot < tcap) {
        const size_t o = (size_t)f * tcap + slot;
        reinterpret_cast<double2 *>(tri_xy)[o] = make_double2(x, y);
        tri_v[o] = v0 | (v1 << 8) | (v2 << 16) | ((orient + 1) << 24);
    }
}

constexpr int kVoteTPL = 2;                                 // target triangles per lane, in registers
constexpr int kVoteTile = kRegBlock * kVoteTPL;             // ... per block
constexpr int kVoteChunk = 512;                             // reference triangles per LDS chunk

// Block (bx, by, bz): target triangles [bx * kVoteTile, + kVoteTile) of frame bz + 1 against the by-th share of the reference's
// chunks.  Every lane reads the same reference triangle (an LDS broadcast) and compares it with its own targets; a match adds
// to the block's K x K vote matrix in LDS, which is flushed with integer atomic adds - exact in any order.
__global__ __launch_bounds__(kRegBlock) void triangle_vote_kernel(const double *__restrict__ tri_xy, const int *__restrict__ tri_v,
                                                                  const int *__restrict__ ntri, int tcap, int K, double eps,
                                                                  int allow_mirror, int *__restrict__ votes)
{
    __shared__ double2 s_xy[kVoteChunk];
    __shared__ int s_v[kVoteChunk];
    __shared__ int s_votes[kRegMaxK * kRegMaxK];
    const int tid = threadIdx.x;
    const int f = blockIdx.z + 1;
    const int nr = min(ntri[0], tcap), nt = min(ntri[f], tcap);
    const int t0 = blockIdx.x * kVoteTile;
    if (t0 >= nt || nr <= 0) return;
    const int nchunks = (nr + kVoteChunk - 1) / kVoteChunk;
    const int per = (nchunks + (int)gridDim.y - 1) / (int)gridDim.y;
    const int c0 = blockIdx.y * per, c1 = min(c0 + per, nchunks);
    if (c0 >= c1) return;
    for (int e = tid; e < K * K; e += kRegBlock) s_votes[e] = 0;

    const double2 *ref_xy = reinterpret_cast<const double2 *>(tri_xy);
    const double2 *tgt_xy = ref_xy + (size_t)f * tcap;
    const int *tgt_v = tri_v + (size_t)f * tcap;
    double tx[kVoteTPL], ty[kVoteTPL];
    int tv[kVoteTPL];
#pragma unroll
    for (int u = 0; u < kVoteTPL; ++u) {
        const int t = t0 + u * kRegBlock + tid;
        const bool valid = t < nt;
        const double2 q = valid ? tgt_xy[t] : make_double2(__builtin_nan(""), __builtin_nan(""));    // NaN matches nothing
        tx[u] = q.x;
        ty[u] = q.y;
        tv[u] = valid ? tgt_v[t] : 0;
    }
    for (int c = c0; c < c1; ++c) {
        __syncthreads();
        const int base = c * kVoteChunk, m = min(kVoteChunk, nr - base);
        for (int r = tid; r < m; r += kRegBlock) {
            s_xy[r] = ref_xy[base + r];
            s_v[r] = tri_v[base + r];
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < m; ++r) {
            const double2 q = s_xy[r];
#pragma unroll
            for (int u = 0; u < kVoteTPL; ++u) {
                if (fabs(q.x - tx[u]) <= eps && fabs(q.y - ty[u]) <= eps) {
                    const int rv = s_v[r];
                    if (allow_mirror || (rv >> 24) == (tv[u] >> 24)) {
#pragma unroll
                        for (int s = 0; s < 24; s += 8) {
                            const int a = (rv >> s) & 0xff, b = (tv[u] >> s) & 0xff;
                            if (a < K && b < K) atomicAdd(&s_votes[a * K + b], 1);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    int *out = votes + (size_t)f * K * K;
    for (int e = tid; e < K * K; e += kRegBlock) {
        const int v = s_votes[e];
        if (v) atomicAdd(&out[e], v);
    }
}

constexpr int kNearChunk = 1024;                            // stars of the scanned list per LDS chunk

// The map of a frame, reference -> frame, as the kernel's template parameter: the 2x3 affine of apgpu_nearest_match ...
struct AffineMap {
    const double *transforms;                               // [F][6]
    struct Frame {
        double A[6];
        __device__ __forceinline__ double2 operator()(double2 r) const
        {
            return make_double2((A[0] * r.x + A[1] * r.y) + A[2], (A[3] * r.x + A[4] * r.y) + A[5]);
        }
    };
    __device__ __forceinline__ Frame frame(int f) const
    {
        Frame T;
#pragma unroll
        for (int i = 0; i < 6; ++i) T.A[i] = transforms[6 * f + i];
        return T;
    }
};

// ... or the polynomial of degree D of apgpu_nearest_match_poly (distortion_core.h); a frame's coefficients are read at a
// wave-uniform address wherever the map is evaluated.
template <int D>
struct PolyMap {
    const double *coef;                                     // [F][2][ncoef]
    PolyFrame fr;
    struct Frame {
        const double *c;
        PolyFrame fr;
        __device__ __forceinline__ double2 operator()(double2 r) const
        {
            double X, Y;
            poly_eval<D>(c, fr, r.x, r.y, X, Y);
            return make_double2(X, Y);
        }
    };
    __device__ __forceinline__ Frame frame(int f) const { return Frame{coef + (size_t)f * 2 * poly_ncoef(D), fr}; }
};

// Block (bx, f, dir).  dir 0: query = T_f(reference star), scanned list = the stars of frame f.  dir 1: query = a star of frame
// f, scanned list = T_f(reference stars).  The scan runs in ascending index and replaces on strictly smaller d2 only: the
// lexicographic (d2, index) minimum.
template <class Map>
__global__ __launch_bounds__(kRegBlock) void nearest_match_kernel(const double *__restrict__ xy, const int *__restrict__ count, const Map map,
                                                                  int M, double radius2,
                                                                  int *__restrict__ fwd_idx, double *__restrict__ fwd_d2,
                                                                  int *__restrict__ bwd_idx, double *__restrict__ bwd_d2)
{
    __shared__ double2 s[kNearChunk];
    const int tid = threadIdx.x;
    const int f = blockIdx.y, dir = blockIdx.z;
    const int n0 = max(0, min(count[0], M)), nf = max(0, min(count[f], M));
    const int nq = dir == 0 ? n0 : nf, ns = dir == 0 ? nf : n0;
    const double2 *ref = reinterpret_cast<const double2 *>(xy);
    const double2 *frm = ref + (size_t)f * M;
    const typename Map::Frame T = map.frame(f);
    const int q = blockIdx.x * kRegBlock + tid;
    int *out_idx = (dir == 0 ? fwd_idx : bwd_idx) + (size_t)f * M;
    double *out_d2 = (dir == 0 ? fwd_d2 : bwd_d2) + (size_t)f * M;
    int best = -1;
    double best_d2 = __builtin_inf();
    if ((int)(blockIdx.x * kRegBlock) < nq) {               // (the same for the whole block)
        double2 p = make_double2(0.0, 0.0);
        if (q < nq) p = dir == 0 ? T(ref[q]) : frm[q];
        for (int base = 0; base < ns; base += kNearChunk) {
            const int m = min(kNearChunk, ns - base);
            __syncthreads();
            for (int r = tid; r < m; r += kRegBlock) s[r] = dir == 0 ? frm[base + r] : T(ref[base + r]);
            __syncthreads();
            if (q < nq) {
#pragma unroll 4
                for (int r = 0; r < m; ++r) {
                    const double d2 = dist2(s[r], p);
                    if (d2 < best_d2) {
                        best_d2 = d2;
                        best = base + r;
                    }
                }
            }
        }
    }
    if (q < M) {
        const bool ok = q < nq && best >= 0 && best_d2 <= radius2;
        out_idx[q] = ok ? best : -1;
        out_d2[q] = ok ? best_d2 : __builtin_inf();
    }
}

long long n_triples(int k) { return (long long)k * (k - 1) * (k - 2) / 6; }

int nearest_match_check(const char *what, const double *xy, const int32_t *count, const double *map, int32_t n_frames, int32_t max_stars,
                        double radius, int32_t *fwd_idx, double *fwd_d2, int32_t *bwd_idx, double *bwd_d2)
{
    if (n_frames < 1 || n_frames > 65535) return fail(APGPU_EINVAL, "%s: %d frames (1 .. 65535)", what, n_frames);
    if (max_stars < 1 || max_stars > kRegMaxStars)
        return fail(APGPU_EINVAL, "%s: list length %d is outside 1 .. %d", what, max_stars, kRegMaxStars);
    if (!(radius >= 0.0)) return fail(APGPU_EINVAL, "%s: radius %g is negative or NaN", what, radius);
    if (!xy || !count || !map || !fwd_idx || !fwd_d2 || !bwd_idx || !bwd_d2) return fail(APGPU_EINVAL, "%s: NULL pointer argument", what);
    return APGPU_OK;
}

template <class Map>
int nearest_match_launch(const char *what, const Map &map, const double *xy, const int32_t *count, int32_t n_frames, int32_t max_stars,
                         double radius, int32_t *fwd_idx, double *fwd_d2, int32_t *bwd_idx, double *bwd_d2, void *stream)
{
    const unsigned blocks = (unsigned)((max_stars + kRegBlock - 1) / kRegBlock);
    hipLaunchKernelGGL(nearest_match_kernel<Map>, dim3(blocks, (unsigned)n_frames, 2u), dim3(kRegBlock), 0, as_stream(stream), xy, count, map,
                       (int)max_stars, radius * radius, fwd_idx, fwd_d2, bwd_idx, bwd_d2);
    return check_launch(what);
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_triangle_build(const double *xy, const int32_t *count, int32_t n_frames, int32_t max_stars, int32_t k,
                                    double min_side, int32_t tri_capacity, double *tri_xy, int32_t *tri_v, int32_t *tri_count,
                                    void *stream)
{
    if (n_frames < 1 || n_frames > 65535) return fail(APGPU_EINVAL, "triangle_build: %d frames (1 .. 65535)", n_frames);
    if (k < 3 || k > kRegMaxK) return fail(APGPU_EINVAL, "triangle_build: K = %d is outside 3 .. %d", k, kRegMaxK);
    if (max_stars < 1) return fail(APGPU_EINVAL, "triangle_build: list length %d", max_stars);
    if (!(min_side >= 0.0)) return fail(APGPU_EINVAL, "triangle_build: min_side %g is negative or NaN", min_side);
    if (tri_capacity < n_triples(k))
        return fail(APGPU_EINVAL, "triangle_build: a list of %d triangles cannot hold the %lld triples of K = %d", tri_capacity,
                    n_triples(k), k);
    if (!xy || !count || !tri_xy || !tri_v || !tri_count) return fail(APGPU_EINVAL, "triangle_build: NULL pointer argument");
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(tri_count, 0, sizeof(int32_t) * n_frames, st) != hipSuccess)
        return fail(APGPU_ELAUNCH, "triangle_build: hipMemsetAsync failed");
    const unsigned blocks = (unsigned)((k * k * k + kRegBlock - 1) / kRegBlock);
    hipLaunchKernelGGL(triangle_build_kernel, dim3(blocks, (unsigned)n_frames), dim3(kRegBlock), 0, st, xy, count, (int)max_stars,
                       (int)k, (int)tri_capacity, min_side * min_side, tri_xy, tri_v, tri_count);
    return check_launch("triangle_build");
}

extern "C" int apgpu_triangle_vote(const double *tri_xy, const int32_t *tri_v, const int32_t *tri_count, int32_t n_frames,
                                   int32_t tri_capacity, int32_t k, double eps, int32_t allow_mirror, int32_t *votes, void *stream)
{
    if (n_frames < 1 || n_frames > 65535) return fail(APGPU_EINVAL, "triangle_vote: %d frames (1 .. 65535)", n_frames);
    if (k < 3 || k > kRegMaxK) return fail(APGPU_EINVAL, "triangle_vote: K = %d is outside 3 .. %d", k, kRegMaxK);
    if (tri_capacity < 1) return fail(APGPU_EINVAL, "triangle_vote: list capacity %d", tri_capacity);
    if (!(eps >= 0.0)) return fail(APGPU_EINVAL, "triangle_vote: eps %g is negative or NaN", eps);
    if (!tri_xy || !tri_v || !tri_count || !votes) return fail(APGPU_EINVAL, "triangle_vote: NULL pointer argument");
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(votes, 0, sizeof(int32_t) * (size_t)n_frames * k * k, st) != hipSuccess)
        return fail(APGPU_ELAUNCH, "triangle_vote: hipMemsetAsync failed");
    if (n_frames == 1) return APGPU_OK;
    // enough blocks to fill the device: the reference's chunks are shared out over grid.y when tiles x frames are few
    const int tiles = (tri_capacity + kVoteTile - 1) / kVoteTile, chunks = (tri_capacity + kVoteChunk - 1) / kVoteChunk;
    const int want = 8 * kNumCU, have = tiles * (n_frames - 1);
    int split = (want + have - 1) / have;
    split = split < 1 ? 1 : (split > chunks ? chunks : split);
    hipLaunchKernelGGL(triangle_vote_kernel, dim3((unsigned)tiles, (unsigned)split, (unsigned)(n_frames - 1)), dim3(kRegBlock), 0, st,
                       tri_xy, tri_v, tri_count, (int)tri_capacity, (int)k, eps, (int)(allow_mirror != 0), votes);
    return check_launch("triangle_vote");
}

extern "C" int apgpu_nearest_match(const double *xy, const int32_t *count, const double *transforms, int32_t n_frames,
                                   int32_t max_stars, double radius, int32_t *fwd_idx, double *fwd_d2, int32_t *bwd_idx,
                                   double *bwd_d2, void *stream)
{
    if (int rc = nearest_match_check("nearest_match", xy, count, transforms, n_frames, max_stars, radius, fwd_idx, fwd_d2, bwd_idx, bwd_d2))
        return rc;
    return nearest_match_launch("nearest_match", AffineMap{transforms}, xy, count, n_frames, max_stars, radius, fwd_idx, fwd_d2, bwd_idx,
                                bwd_d2, stream);
}

extern "C" int apgpu_nearest_match_poly(const double *xy, const int32_t *count, const double *coef, int32_t degree, double x0, double y0,
                                        double scale_l, int32_t n_frames, int32_t max_stars, double radius, int32_t *fwd_idx,
                                        double *fwd_d2, int32_t *bwd_idx, double *bwd_d2, void *stream)
{
    const char *what = "nearest_match_poly";
    if (int rc = nearest_match_check(what, xy, count, coef, n_frames, max_stars, radius, fwd_idx, fwd_d2, bwd_idx, bwd_d2)) return rc;
    if (degree < 1 || degree > kPolyMaxDegree) return fail(APGPU_EINVAL, "%s: degree %d is outside 1 .. %d", what, degree, kPolyMaxDegree);
    if (!(is_finite(x0) && is_finite(y0) && is_finite(scale_l) && scale_l > 0.0))
        return fail(APGPU_EINVAL, "%s: origin (%g, %g) must be finite and L = %g finite and positive", what, x0, y0, scale_l);
    const PolyFrame fr{x0, y0, scale_l};
#define APGPU_NEAREST_POLY(D) \
    case D: return nearest_match_launch(what, PolyMap<D>{coef, fr}, xy, count, n_frames, max_stars, radius, fwd_idx, fwd_d2, bwd_idx, bwd_d2, stream)
    switch (degree) {
        APGPU_NEAREST_POLY(1);
        APGPU_NEAREST_POLY(2);
        APGPU_NEAREST_POLY(3);
        APGPU_NEAREST_POLY(4);
    default:
        APGPU_NEAREST_POLY(5);
    }
#undef APGPU_NEAREST_POLY
}
