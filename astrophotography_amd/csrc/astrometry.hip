// astrometry.hip - F21: the catalogue side of the offline plate solver on gfx950 (include/apgpu.h F21; restated in
// tests/astrometry_model.py).  All float64, no contraction: every expression rounds as the NumPy model's does.
//
//   sky_project  the gnomonic projection of every catalogue star about the hint centre, one lane per star: 16 bytes read, 17 written
//   cell_select  per search cell the first `capacity` stars, in the list's order, inside a closed square: an ordered stream compaction.
//                A workgroup of four wavefronts owns a cell and walks the list 1024 stars at a trip (four ballots per wavefront); a lane's
//                slot is the cell's running count + the stars of earlier sub-chunks and wavefronts of the trip (sixteen counts passed
//                through LDS, double-buffered: one barrier per trip) + the set bits below it in its ballot.  No atomics: the list is the
//                same on every run.  The walk ends once a trip leaves the count above `capacity`.
#include "common.h"

namespace apgpu {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kSub = 4;                                     // ballots per wavefront and trip
constexpr double kD2R = 3.14159265358979323846 / 180.0;

__global__ __launch_bounds__(kBlock) void sky_project_kernel(const double *__restrict__ ra, const double *__restrict__ dec, long long n, double a0,
                                                            double sd0, double cd0, double cos_rc, double *__restrict__ xi,
                                                            double *__restrict__ eta, uint8_t *__restrict__ keep)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double r = ra[i], q = dec[i];
    const double a = r * kD2R, d = q * kD2R;
    const double da = a - a0;
    const double sd = sin(d), cd = cos(d), sda = sin(da), cda = cos(da);
    const double cosc = sd0 * sd + (cd0 * cd) * cda;
    const bool front = cosc > 0.0;                          // false for NaN: a non-finite input lands here
    const double nan = __builtin_nan("");
    xi[i] = front ? ((cd * sda) / cosc) / kD2R : nan;
    eta[i] = front ? ((cd0 * sd - (sd0 * cd) * cda) / cosc) / kD2R : nan;
    if (keep) keep[i] = (front && cosc >= cos_rc && __builtin_isfinite(r) && __builtin_isfinite(q)) ? 1 : 0;
}

__device__ __forceinline__ int lanes_below(unsigned long long ballot)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

__global__ __launch_bounds__(kBlock) void cell_select_kernel(const double *__restrict__ x, const double *__restrict__ y, long long n,
                                                            const double *__restrict__ cells, int capacity, int *__restrict__ idx,
                                                            int *__restrict__ count, int *__restrict__ inside)
{
    __shared__ int part[2][kSub][kWaves];
    const size_t c = blockIdx.x;
    const double cx = cells[3 * c], cy = cells[3 * c + 1], half = cells[3 * c + 2];
    const int wave = threadIdx.x / kWave;
    int *list = idx + c * (size_t)capacity;
    int run = 0, buf = 0;                                   // run: the stars found so far, the same in every lane
    for (long long base = 0; base < n && run <= capacity; base += kBlock * kSub, buf ^= 1) {
        bool in[kSub];
        unsigned long long ballot[kSub];
#pragma unroll
        for (int j = 0; j < kSub; j++) {
            const long long i = base + j * kBlock + threadIdx.x;
            in[j] = i < n && fabs(x[i] - cx) <= half && fabs(y[i] - cy) <= half;
            ballot[j] = __ballot(in[j]);
        }
        if (threadIdx.x % kWave == 0) {
#pragma unroll
            for (int j = 0; j < kSub; j++) part[buf][j][wave] = __popcll(ballot[j]);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kSub; j++) {
            int mine = run;
#pragma unroll
            for (int w = 0; w < kWaves; w++) {
                const int v = part[buf][j][w];
                if (w < wave) mine += v;
                run += v;
            }
            const int slot = mine + lanes_below(ballot[j]);
            if (in[j] && slot < capacity) list[slot] = (int)(base + j * kBlock + threadIdx.x);
        }
    }
    for (int p = min(run, capacity) + (int)threadIdx.x; p < capacity; p += kBlock) list[p] = -1;
    if (threadIdx.x == 0) {
        count[c] = min(run, capacity);
        inside[c] = run;
    }
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_sky_project(const double *ra, const double *dec, int64_t n, double ra0, double dec0, double cos_rc, double *xi, double *eta,
                                 uint8_t *keep, void *stream)
{
    if (n < 0 || n > 0x7fffffffLL) return fail(APGPU_EINVAL, "sky_project: %lld stars, at most 2^31 - 1", (long long)n);
    if (!__builtin_isfinite(ra0) || !__builtin_isfinite(dec0) || !(dec0 >= -90.0 && dec0 <= 90.0))
        return fail(APGPU_EINVAL, "sky_project: centre (%g, %g)", ra0, dec0);
    if (!(cos_rc >= -1.0 && cos_rc <= 1.0)) return fail(APGPU_EINVAL, "sky_project: cos_rc %g outside -1 .. 1", cos_rc);
    if (n == 0) return APGPU_OK;
    if (!ra || !dec || !xi || !eta) return fail(APGPU_EINVAL, "sky_project: NULL pointer argument");
    if (!aligned(ra, 8) || !aligned(dec, 8) || !aligned(xi, 8) || !aligned(eta, 8)) return fail(APGPU_EINVAL, "sky_project: the arrays must be 8-byte aligned");
    const double a0 = ra0 * kD2R, d0 = dec0 * kD2R;
    hipLaunchKernelGGL(sky_project_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream), ra, dec, (long long)n, a0,
                       sin(d0), cos(d0), cos_rc, xi, eta, keep);
    return check_launch("sky_project");
}

extern "C" int apgpu_cell_select(const double *x, const double *y, int64_t n, const double *cells, int64_t n_cells, int32_t capacity, int32_t *idx,
                                 int32_t *count, int32_t *inside, void *stream)
{
    if (n < 0 || n > 0x7fffffffLL) return fail(APGPU_EINVAL, "cell_select: %lld stars, at most 2^31 - 1", (long long)n);
    if (n_cells < 0 || n_cells > 0x7fffffffLL) return fail(APGPU_EINVAL, "cell_select: %lld cells, at most 2^31 - 1", (long long)n_cells);
    if (capacity < 1 || capacity > APGPU_CELL_MAX_CAPACITY)
        return fail(APGPU_EINVAL, "cell_select: capacity %d outside 1 .. %d", capacity, APGPU_CELL_MAX_CAPACITY);
    if (n_cells * (int64_t)capacity > 0x7fffffffLL) return fail(APGPU_EINVAL, "cell_select: %lld cells of %d slots", (long long)n_cells, capacity);
    if (n_cells == 0) return APGPU_OK;
    if (!cells || !idx || !count || !inside || (n > 0 && (!x || !y))) return fail(APGPU_EINVAL, "cell_select: NULL pointer argument");
    if (!aligned(x, 8) || !aligned(y, 8) || !aligned(cells, 8) || !aligned(idx, 4) || !aligned(count, 4) || !aligned(inside, 4))
        return fail(APGPU_EINVAL, "cell_select: the coordinates and cells must be 8-byte, the lists 4-byte aligned");
    hipLaunchKernelGGL(cell_select_kernel, dim3((unsigned)n_cells), dim3(kBlock), 0, as_stream(stream), x, y, (long long)n, cells, (int)capacity, idx,
                       count, inside);
    return check_launch("cell_select");
}
