// F22 ApEmpiricalPsf: the effective PSF of Anderson & King (2000) on an oversampled grid, PSF-fitting photometry
// with it, and the model / residual image.  The definition is the project's own, restated in tests/epsf_model.py.
//
// The grid (float32, at most 257 x 257 = 258 KiB) is read from global memory through the caches: the largest grid does not fit
// the 160 KiB of LDS, the usual one (o = 4, R = 12: 37 KiB) sits in L2 from its first use, and every evaluation touches one 4 x 4
// patch whose place differs from lane to lane (a star's sub-pixel phase), which LDS would serve with bank conflicts.
//
//   accumulate  one wavefront per node, lanes striding the stars; each round of the clip streams the stars again
//   update      one thread per node: add the mean residual, 5 x 5 smoothing with the caller's taps
//   shift       one thread per node: the grid evaluated at its own nodes plus an offset, times a scale
//   fit         one wavefront per star: damped Gauss-Newton in float64 after measurestars.hip (butterfly sums, a Cholesky
//               solution per lane, uniform control flow); the star's data are staged in LDS as float64
//   render      one workgroup per 32 x 32 tile: each thread sums its tile's stars in list order
// All arithmetic is float64 and every operation rounds on its own (-ffp-contract=off).
#include "common.h"
#include "epsf_core.h"
#include "np_exact.h"

#include <cmath>

namespace apgpu {
namespace {

constexpr int kRec = APGPU_EPSF_REC;
constexpr int kTile = APGPU_EPSF_TILE;
constexpr int kMaxFitHalf = APGPU_EPSF_MAX_RADIUS;

struct Taps {
    double w[25];
};

// ---- accumulate ---------------------------------------------------------------------------------------------------------------
struct Sampler {
    const float *img;
    long long H, W;
    const double *stars;     // [n][4] f, x, y, sky
    EpsfGrid g;
    int ki, kj;              // the node, relative to the grid's centre

    // the residual of star s at this node, if it has one
    __device__ bool operator()(int s, double &r) const
    {
        const double f = stars[4LL * s], x = stars[4LL * s + 1], y = stars[4LL * s + 2], sky = stars[4LL * s + 3];
        if (!epsf_star_usable(f, x, y, sky)) return false;
        long long px, py;
        if (!epsf_pixel_of(ki, x, g.o, &px) || !epsf_pixel_of(kj, y, g.o, &py)) return false;
        if (px < 0 || px >= W || py < 0 || py >= H) return false;
        const double d = (double)img[py * W + px];
        if (!(fabs(d) < INFINITY)) return false;
        r = (d - sky) / f - epsf_eval<false>(g, (double)px - x, (double)py - y, nullptr, nullptr);
        return fabs(r) < INFINITY;
    }
};

__global__ void __launch_bounds__(kWave) epsf_accumulate_kernel(Sampler sm, int n, double sigma, int maxiters,
                                                                double *__restrict__ mean_out, int32_t *__restrict__ count_out)
{
    const int node = blockIdx.x, lane = threadIdx.x;
    const int G = sm.g.G, half = sm.g.o * sm.g.R;
    sm.kj = node / G - half;
    sm.ki = node % G - half;
    double lo = -INFINITY, hi = INFINITY, mean = 0.0, kept = 0.0, prev = -1.0;
    for (int round = 0; round <= maxiters; ++round) {
        double c = 0.0, s1 = 0.0;
        for (int s = lane; s < n; s += kWave) {
            double r;
            if (sm(s, r) && r >= lo && r <= hi) {
                c += 1.0;
                s1 += r;
            }
        }
        c = wave_sum(c);
        s1 = wave_sum(s1);
        if (c == prev) break;                               // the round removed nothing
        kept = c;
        if (c == 0.0) {
            mean = 0.0;
            break;
        }
        mean = s1 / c;
        if (round == maxiters) break;
        double s2 = 0.0;
        for (int s = lane; s < n; s += kWave) {
            double r;
            if (sm(s, r) && r >= lo && r <= hi) s2 += (r - mean) * (r - mean);
        }
        s2 = wave_sum(s2);
        const double sd = sqrt(s2 / c);
        lo = mean - sigma * sd;
        hi = mean + sigma * sd;
        prev = c;
    }
    if (lane == 0) {
        mean_out[node] = mean;
        count_out[node] = (int32_t)kept;
    }
}

// ---- update, shift ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) epsf_update_kernel(const float *__restrict__ E, const double *__restrict__ mean,
                                                          const int32_t *__restrict__ count, int G, int min_count, Taps taps,
                                                          float *__restrict__ out)
{
    const int i = blockIdx.x * 16 + threadIdx.x % 16, j = blockIdx.y * 16 + threadIdx.x / 16;
    if (i >= G || j >= G) return;
    double acc = 0.0;
    for (int a = 0; a < 5; ++a) {
        const int jj = epsf_clamp(j + a - 2, G);
        for (int b = 0; b < 5; ++b) {
            const int q = jj * G + epsf_clamp(i + b - 2, G);
            const double e = (double)E[q];
            const double t = count[q] >= min_count ? e + mean[q] : e;
            acc = acc + taps.w[a * 5 + b] * t;
        }
    }
    out[j * G + i] = (float)acc;
}

__global__ void __launch_bounds__(256) epsf_shift_kernel(EpsfGrid g, double dx, double dy, double scale, float *__restrict__ out)
{
    const int i = blockIdx.x * 16 + threadIdx.x % 16, j = blockIdx.y * 16 + threadIdx.x / 16;
    if (i >= g.G || j >= g.G) return;
    const int half = g.o * g.R;
    const double x = (double)(i - half) / (double)g.o + dx, y = (double)(j - half) / (double)g.o + dy;
    out[j * g.G + i] = (float)(epsf_eval<false>(g, x, y, nullptr, nullptr) * scale);
}

// ---- fit ----------------------------------------------------------------------------------------------------------------------
struct FitBox {
    const double *d;         // LDS: the datum of every pixel of the box, NaN where the pixel is not used
    long long x0, y0;        // the box's first pixel
    int wb, nbox, lane;
    EpsfGrid g;
    double rn2, inv_gain;    // weights 1 / (rn2 + max(model, 0) inv_gain); inv_gain == 0 and rn2 == 1: uniform
};

// One pass over the pixels at p = (f, x, y, sky): J^T W J (upper triangle, row-major), J^T W r and chi^2 of r = model - datum over
// the first NF parameters; the sums are the same in every lane.  FROZEN: the weights are those of the model at pw, not at p.
template <int NF, bool FROZEN>
__device__ void fit_pass(const FitBox &bx, const double (&p)[4], const double (&pw)[4], double (&JtJ)[NF * (NF + 1) / 2], double (&Jtr)[NF],
                         double &chi2)
{
#pragma unroll
    for (int i = 0; i < NF * (NF + 1) / 2; ++i) JtJ[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NF; ++i) Jtr[i] = 0.0;
    double c2 = 0.0;
    for (int k = bx.lane; k < bx.nbox; k += kWave) {
        const double d = bx.d[k];
        if (d != d) continue;
        const int row = k / bx.wb, col = k - row * bx.wb;
        double ex, ey;
        const double e = epsf_eval<true>(bx.g, (double)(bx.x0 + col) - p[1], (double)(bx.y0 + row) - p[2], &ex, &ey);
        const double m = p[0] * e + p[3];
        double mw = m;
        if (FROZEN)
            mw = pw[0] * epsf_eval<false>(bx.g, (double)(bx.x0 + col) - pw[1], (double)(bx.y0 + row) - pw[2], nullptr, nullptr) + pw[3];
        const double w = 1.0 / (bx.rn2 + fmax(mw, 0.0) * bx.inv_gain);
        const double r = m - d;
        double J[4];
        J[0] = e;
        J[1] = -(p[0] * ex);
        J[2] = -(p[0] * ey);
        J[3] = 1.0;
        c2 += w * (r * r);
        int q = 0;
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const double wi = w * J[i];
            Jtr[i] += wi * r;
#pragma unroll
            for (int j = i; j < NF; ++j) JtJ[q++] += wi * J[j];
        }
    }
#pragma unroll
    for (int i = 0; i < NF * (NF + 1) / 2; ++i) JtJ[i] = wave_sum(JtJ[i]);
#pragma unroll
    for (int i = 0; i < NF; ++i) Jtr[i] = wave_sum(Jtr[i]);
    chi2 = wave_sum(c2);
}

// M = D^-1 JtJ D^-1 with D = sqrt(diag(JtJ)) and 1 + lambda on the diagonal; false if a diagonal element is not positive and finite.
template <int NF>
__device__ bool fit_matrix(const double (&JtJ)[NF * (NF + 1) / 2], double lambda, double (&D)[NF], double (&M)[NF][NF])
{
    bool ok = true;
    int q = 0;
#pragma unroll
    for (int i = 0; i < NF; ++i) {
#pragma unroll
        for (int j = i; j < NF; ++j) {
            M[i][j] = JtJ[q];
            M[j][i] = JtJ[q];
            ++q;
        }
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        ok = ok && (M[i][i] > 0.0) && (M[i][i] < 1e300);
        D[i] = sqrt(M[i][i]);
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
#pragma unroll
        for (int j = 0; j < NF; ++j) M[i][j] = (i == j) ? 1.0 + lambda : M[i][j] / (D[i] * D[j]);
    }
    return ok;
}

// Cholesky factor (lower, in place); false if M is not positive definite.
template <int NF>
__device__ bool fit_cholesky(double (&M)[NF][NF])
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        double s = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= M[j][k] * M[j][k];
        ok = ok && (s > 0.0) && (s < 1e300);
        const double l = sqrt(s);
        M[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < NF; ++i) {
            double t = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= M[i][k] * M[j][k];
            M[i][j] = t / l;
        }
    }
    return ok;
}

template <int NF>
__device__ void fit_solve(const double (&L)[NF][NF], double (&x)[NF])
{
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        double t = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= L[i][k] * x[k];
        x[i] = t / L[i][i];
    }
#pragma unroll
    for (int i = NF - 1; i >= 0; --i) {
        double t = x[i];
#pragma unroll
        for (int k = i + 1; k < NF; ++k) t -= L[k][i] * x[k];
        x[i] = t / L[i][i];
    }
}

// Damped Gauss-Newton over the first NF of (f, x, y, sky).  It ends when a step with damping <= 1 has |dx|, |dy| < 1e-7 and
// |df| <= 1e-9 |f|, or after max_iter iterations; false on a system that is not positive definite or a non-finite chi^2.
// With the noise model's weights a trial step is judged with the weights of the point it starts from (they are frozen over the
// step, or chi^2 would compare two different sums), and an accepted point gets its sums again with its own weights.
template <int NF>
__device__ bool fit_run(const FitBox &bx, double (&p)[4], double &chi2, int max_iter, int &iters)
{
    double JtJ[NF * (NF + 1) / 2], Jtr[NF], JtJt[NF * (NF + 1) / 2], Jtrt[NF], D[NF], M[NF][NF], u[NF];
    const bool weighted = bx.inv_gain != 0.0;
    fit_pass<NF, false>(bx, p, p, JtJ, Jtr, chi2);
    iters = 0;
    if (!(chi2 < 1e300)) return false;
    double lambda = 1e-3, nu = 2.0;
    for (int it = 1; it <= max_iter; ++it) {
        iters = it;
        if (!fit_matrix<NF>(JtJ, lambda, D, M)) return false;
        if (!fit_cholesky<NF>(M)) {
            lambda *= nu;
            nu *= 2.0;
            if (lambda > 1e30) return false;
            continue;
        }
        double gs[NF], step[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            gs[i] = Jtr[i] / D[i];
            u[i] = -gs[i];
        }
        fit_solve<NF>(M, u);
        double pt[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) pt[i] = p[i];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            step[i] = u[i] / D[i];
            pt[i] = p[i] + step[i];
        }
        const bool small = lambda <= 1.0 && fabs(step[1]) < 1e-7 && fabs(step[2]) < 1e-7 && fabs(step[0]) <= 1e-9 * fabs(p[0]);
        double chi2t;
        if (weighted)
            fit_pass<NF, true>(bx, pt, p, JtJt, Jtrt, chi2t);
        else
            fit_pass<NF, false>(bx, pt, pt, JtJt, Jtrt, chi2t);
        // a rise within the rounding noise of chi^2 is accepted (measurestars.hip); false for NaN
        if (chi2t <= chi2 * (1.0 + 1e-14)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) p[i] = pt[i];
#pragma unroll
            for (int i = 0; i < NF * (NF + 1) / 2; ++i) JtJ[i] = JtJt[i];
#pragma unroll
            for (int i = 0; i < NF; ++i) Jtr[i] = Jtrt[i];
            double pred = 0.0;
#pragma unroll
            for (int i = 0; i < NF; ++i) pred += u[i] * (lambda * u[i] - gs[i]);
            const double rho = pred > 1e-12 * chi2 ? (chi2 - chi2t) / pred : 1.0;
            const double t = 2.0 * rho - 1.0;
            chi2 = chi2t;
            lambda = fmax(lambda * fmax(1.0 / 3.0, 1.0 - t * t * t), 1e-15);
            nu = 2.0;
            if (weighted) {
                fit_pass<NF, false>(bx, p, p, JtJ, Jtr, chi2);
                if (!(chi2 < 1e300)) return false;
            }
        } else {
            lambda *= nu;
            nu *= 2.0;
            if (lambda > 1e30) return false;
        }
        if (small) break;
    }
    return true;
}

__global__ void __launch_bounds__(kWave) epsf_fit_kernel(const float *__restrict__ img, long long H, long long W,
                                                         const double *__restrict__ init, const double *__restrict__ prev, int n,
                                                         EpsfGrid g, double r_fit, int half, int fit_sky, double rn2, double inv_gain,
                                                         int max_iter, double *__restrict__ rec)
{
    extern __shared__ double epsf_lds[];
    const int star = blockIdx.x, lane = threadIdx.x;
    if (star >= n) return;
    double p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = init[4LL * star + i];
    const double f_in = p[0], x_in = p[1], y_in = p[2], sky_in = p[3];
    double *out = rec + (long long)star * kRec;
    bool ok = fabs(f_in) < INFINITY && fabs(sky_in) < INFINITY && fabs(x_in) <= 1e9 && fabs(y_in) <= 1e9;
    double f0 = 0.0, x0 = 0.0, y0 = 0.0;
    if (prev) {
        f0 = prev[3LL * star];
        x0 = prev[3LL * star + 1];
        y0 = prev[3LL * star + 2];
        ok = ok && fabs(f0) < INFINITY && fabs(x0) <= 1e9 && fabs(y0) <= 1e9;
    }
    const int wb = 2 * half + 1, nbox = wb * wb;
    double cnt = 0.0, chi2 = nan("");
    int iters = 0;
    if (ok) {                                                    // (uniform: the same star in every lane)
        const long long cx = (long long)rint(x_in), cy = (long long)rint(y_in);
        const double r2 = r_fit * r_fit;
        for (int k = lane; k < nbox; k += kWave) {
            const int row = k / wb, col = k - row * wb;
            const long long px = cx - half + col, py = cy - half + row;
            const double ddx = (double)(col - half), ddy = (double)(row - half);
            double d = nan("");
            if (ddx * ddx + ddy * ddy <= r2 && px >= 0 && px < W && py >= 0 && py < H) {
                d = (double)img[py * W + px];
                if (prev) d = d + f0 * epsf_eval<false>(g, (double)px - x0, (double)py - y0, nullptr, nullptr);
                if (!(fabs(d) < INFINITY)) d = nan("");
            }
            epsf_lds[k] = d;
            if (d == d) cnt += 1.0;
        }
        cnt = wave_sum(cnt);
        __syncthreads();
        FitBox bx{epsf_lds, cx - half, cy - half, wb, nbox, lane, g, rn2, inv_gain};
        ok = cnt >= 6.0;
        if (ok) ok = fit_sky ? fit_run<4>(bx, p, chi2, max_iter, iters) : fit_run<3>(bx, p, chi2, max_iter, iters);
        ok = ok && fabs(p[0]) < INFINITY && fabs(p[1]) < INFINITY && fabs(p[2]) < INFINITY && fabs(p[3]) < INFINITY && chi2 < INFINITY;
    }
    if (lane == 0) {
        out[0] = ok ? p[0] : f_in;
        out[1] = ok ? p[1] : x_in;
        out[2] = ok ? p[2] : y_in;
        out[3] = ok ? p[3] : sky_in;
        out[4] = ok ? chi2 : nan("");
        out[5] = cnt;
        out[6] = (double)iters;
        out[7] = ok ? 1.0 : 0.0;
    }
}

// ---- render -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) epsf_render_kernel(const float *__restrict__ img, long long H, long long W,
                                                          const double *__restrict__ stars, int n, const int32_t *__restrict__ offsets,
                                                          const int32_t *__restrict__ list, int n_entries, EpsfGrid g,
                                                          float *__restrict__ model, float *__restrict__ resid)
{
    const long long tiles_x = (W + kTile - 1) / kTile;
    const long long tile = (long long)blockIdx.y * tiles_x + blockIdx.x;
    int first = offsets[tile], last = offsets[tile + 1];
    first = first < 0 ? 0 : first;
    last = last > n_entries ? n_entries : last;
    const long long px = (long long)blockIdx.x * kTile + threadIdx.x % kTile;
    for (int rr = threadIdx.x / kTile; rr < kTile; rr += 256 / kTile) {
        const long long py = (long long)blockIdx.y * kTile + rr;
        if (px >= W || py >= H) continue;
        double sum = 0.0;
        for (int e = first; e < last; ++e) {
            const int s = list[e];
            if (s < 0 || s >= n) continue;
            const double f = stars[3LL * s], x = stars[3LL * s + 1], y = stars[3LL * s + 2];
            if (!(fabs(f) < INFINITY)) continue;
            sum = sum + f * epsf_eval<false>(g, (double)px - x, (double)py - y, nullptr, nullptr);
        }
        if (model) model[py * W + px] = (float)sum;
        if (resid) resid[py * W + px] = (float)((double)img[py * W + px] - sum);
    }
}

int check_grid(const char *what, const float *grid, int32_t o, int32_t R, EpsfGrid *g)
{
    if (o < 1 || o > APGPU_EPSF_MAX_OVERSAMPLING) return fail(APGPU_EINVAL, "%s: oversampling %d is outside 1 .. %d", what, o, APGPU_EPSF_MAX_OVERSAMPLING);
    if (R < 2 || R > APGPU_EPSF_MAX_RADIUS) return fail(APGPU_EINVAL, "%s: radius %d is outside 2 .. %d", what, R, APGPU_EPSF_MAX_RADIUS);
    if (!grid || !aligned(grid, 4)) return fail(APGPU_EINVAL, "%s: the grid is NULL or misaligned", what);
    *g = EpsfGrid{grid, 2 * o * R + 1, o, R};
    return APGPU_OK;
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_epsf_accumulate_f32(const float *image, int64_t height, int64_t width, const double *stars, int32_t n_stars,
                                         const float *grid, int32_t oversampling, int32_t radius, double sigma, int32_t maxiters,
                                         double *mean_out, int32_t *count_out, void *stream)
{
    EpsfGrid g;
    if (int rc = check_plane("epsf_accumulate", image, height, width)) return rc;
    if (int rc = check_grid("epsf_accumulate", grid, oversampling, radius, &g)) return rc;
    if (n_stars < 0) return fail(APGPU_EINVAL, "epsf_accumulate: negative star count %d", n_stars);
    if (!(sigma > 0.0) || maxiters < 0) return fail(APGPU_EINVAL, "epsf_accumulate: sigma %g or maxiters %d is not valid", sigma, maxiters);
    if (!mean_out || !count_out || (n_stars > 0 && !stars) || !aligned(mean_out, 8) || !aligned(count_out, 4) || !aligned(stars, 8))
        return fail(APGPU_EINVAL, "epsf_accumulate: NULL or misaligned pointer argument");
    Sampler sm{image, (long long)height, (long long)width, stars, g, 0, 0};
    hipLaunchKernelGGL(epsf_accumulate_kernel, dim3((unsigned)(g.G * g.G)), dim3(kWave), 0, as_stream(stream), sm, (int)n_stars, sigma,
                       (int)maxiters, mean_out, count_out);
    return check_launch("epsf_accumulate");
}

extern "C" int apgpu_epsf_update_f32(const float *grid, const double *mean, const int32_t *count, int32_t oversampling, int32_t radius,
                                     int32_t min_count, const double *taps, float *out, void *stream)
{
    EpsfGrid g;
    if (int rc = check_grid("epsf_update", grid, oversampling, radius, &g)) return rc;
    if (!mean || !count || !taps || !out || !aligned(mean, 8) || !aligned(count, 4) || !aligned(out, 4))
        return fail(APGPU_EINVAL, "epsf_update: NULL or misaligned pointer argument");
    if (out == grid) return fail(APGPU_EINVAL, "epsf_update: out must not be the grid");
    Taps t;
    for (int i = 0; i < 25; ++i) {
        if (!(fabs(taps[i]) < INFINITY)) return fail(APGPU_EINVAL, "epsf_update: tap %d is not finite", i);
        t.w[i] = taps[i];
    }
    const unsigned nb = (unsigned)((g.G + 15) / 16);
    hipLaunchKernelGGL(epsf_update_kernel, dim3(nb, nb), dim3(256), 0, as_stream(stream), grid, mean, count, g.G, (int)min_count, t, out);
    return check_launch("epsf_update");
}

extern "C" int apgpu_epsf_shift_f32(const float *grid, int32_t oversampling, int32_t radius, double dx, double dy, double scale,
                                    float *out, void *stream)
{
    EpsfGrid g;
    if (int rc = check_grid("epsf_shift", grid, oversampling, radius, &g)) return rc;
    if (!out || !aligned(out, 4)) return fail(APGPU_EINVAL, "epsf_shift: NULL or misaligned pointer argument");
    if (out == grid) return fail(APGPU_EINVAL, "epsf_shift: out must not be the grid");
    if (!(fabs(dx) < INFINITY) || !(fabs(dy) < INFINITY) || !(fabs(scale) < INFINITY))
        return fail(APGPU_EINVAL, "epsf_shift: the offset (%g, %g) or the scale %g is not finite", dx, dy, scale);
    const unsigned nb = (unsigned)((g.G + 15) / 16);
    hipLaunchKernelGGL(epsf_shift_kernel, dim3(nb, nb), dim3(256), 0, as_stream(stream), g, dx, dy, scale, out);
    return check_launch("epsf_shift");
}

extern "C" int apgpu_epsf_fit_f32(const float *image, int64_t height, int64_t width, const double *init, const double *prev,
                                  int32_t n_stars, const float *grid, int32_t oversampling, int32_t radius, double r_fit, int32_t fit_sky,
                                  double gain, double readnoise, int32_t max_iter, double *rec_out, void *stream)
{
    EpsfGrid g;
    if (int rc = check_plane("epsf_fit", image, height, width)) return rc;
    if (int rc = check_grid("epsf_fit", grid, oversampling, radius, &g)) return rc;
    if (n_stars < 0) return fail(APGPU_EINVAL, "epsf_fit: negative star count %d", n_stars);
    if (!(r_fit >= 1.0) || !(r_fit <= (double)kMaxFitHalf)) return fail(APGPU_EINVAL, "epsf_fit: r_fit %g is outside 1 .. %d", r_fit, kMaxFitHalf);
    if (max_iter < 1) return fail(APGPU_EINVAL, "epsf_fit: max_iter %d is below 1", max_iter);
    if (!(gain >= 0.0) || !(gain < INFINITY) || !(readnoise >= 0.0) || !(readnoise < INFINITY))
        return fail(APGPU_EINVAL, "epsf_fit: gain %g or readnoise %g is not valid", gain, readnoise);
    if (n_stars == 0) return APGPU_OK;
    if (!init || !rec_out || !aligned(init, 8) || !aligned(prev, 8) || !aligned(rec_out, 8))
        return fail(APGPU_EINVAL, "epsf_fit: NULL or misaligned pointer argument");
    const int half = (int)floor(r_fit);
    const size_t lds_bytes = (size_t)(2 * half + 1) * (2 * half + 1) * sizeof(double);
    const bool weighted = gain > 0.0;
    hipLaunchKernelGGL(epsf_fit_kernel, dim3((unsigned)n_stars), dim3(kWave), lds_bytes, as_stream(stream), image, (long long)height,
                       (long long)width, init, prev, (int)n_stars, g, r_fit, half, (int)(fit_sky != 0), weighted ? readnoise * readnoise : 1.0,
                       weighted ? 1.0 / gain : 0.0, (int)max_iter, rec_out);
    return check_launch("epsf_fit");
}

extern "C" int apgpu_epsf_render_f32(const float *image, int64_t height, int64_t width, const double *stars, int32_t n_stars,
                                     const int32_t *tile_offsets, const int32_t *tile_stars, int32_t n_entries, const float *grid,
                                     int32_t oversampling, int32_t radius, float *model_out, float *residual_out, void *stream)
{
    EpsfGrid g;
    if (height <= 0 || width <= 0) return fail(APGPU_EINVAL, "epsf_render: image of %lld x %lld", (long long)height, (long long)width);
    if (int rc = check_grid("epsf_render", grid, oversampling, radius, &g)) return rc;
    if (n_stars < 0 || n_entries < 0) return fail(APGPU_EINVAL, "epsf_render: negative star count %d or list length %d", n_stars, n_entries);
    if (!model_out && !residual_out) return fail(APGPU_EINVAL, "epsf_render: neither a model nor a residual plane");
    if ((residual_out && !image) || !tile_offsets || (n_entries > 0 && (!tile_stars || !stars)) || !aligned(image, 4) ||
        !aligned(model_out, 4) || !aligned(residual_out, 4) || !aligned(stars, 8) || !aligned(tile_offsets, 4) || !aligned(tile_stars, 4))
        return fail(APGPU_EINVAL, "epsf_render: NULL or misaligned pointer argument");
    if ((model_out && (model_out == residual_out || model_out == image)) || (residual_out && residual_out == image))
        return fail(APGPU_EINVAL, "epsf_render: the model and the residual must be planes of their own");
    dim3 grid_dim;
    if (int rc = tile_grid("epsf_render", height, width, kTile, kTile, &grid_dim)) return rc;
    hipLaunchKernelGGL(epsf_render_kernel, grid_dim, dim3(256), 0, as_stream(stream), image, (long long)height, (long long)width, stars,
                       (int)n_stars, tile_offsets, tile_stars, (int)n_entries, g, model_out, residual_out);
    return check_launch("epsf_render");
}
