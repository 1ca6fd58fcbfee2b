// ApMeasureStars: weighted least-squares fits of a 2-D Gaussian plus a constant to star cut-outs (reference:
// core/ApMeasureStars.py:223-430, astropy.modeling Gaussian2D + Const2D under LevMarLSQFitter).
//
// One wavefront per star, everything in float64 (plain C++, no contraction).  The cut-out and its standard deviations sit in
// LDS (float32 each, as the reference holds them); every Levenberg-Marquardt iteration is one pass of the 64 lanes over the
// Wb^2 pixels that accumulates J^T W J (upper triangle), J^T W r and chi^2, a butterfly of shuffles that leaves the same sums
// in every lane, and a Cholesky solution (<= 7 x 7) of the damped, diagonally scaled normal equations that every lane
// computes for itself: the control flow is uniform.  The three stages of the reference (4, 5, 7 free parameters) are three
// instantiations of one template, so every small array is indexed by constants and stays in registers.
//
// Parameter order inside this file: A, sigma_x, sigma_y, theta, B, x_mean, y_mean - a stage frees the first NF of them.
// The model's "x" is the FIRST axis of the cut-out (np.mgrid), the row: a quirk of the reference that is kept.
#include "common.h"
#include "np_exact.h"

#include <cmath>

namespace apgpu {
namespace {

constexpr int kFitMaxBox = APGPU_GAUSS2D_MAX_BOX;   // 2 * 76^2 floats = 46208 bytes of LDS
constexpr int kRec = APGPU_GAUSS2D_REC;

struct Box {
    const float *d;      // the cut-out, row-major [Wb, Wb]
    const float *sd;     // its standard deviations (float32, as the reference's std_arr)
    int Wb, npix, lane;
};

// One pass over the pixels at parameters p: JtJ (upper triangle, row-major), Jtr and chi^2 of the weighted residuals
// w (model - d), w = float32(1 / sd): the sums are the same in every lane.
template <int NF>
__device__ void accumulate(const Box &bx, const double (&p)[7], double (&JtJ)[NF * (NF + 1) / 2], double (&Jtr)[NF], double &chi2)
{
    const double A = p[0], sx = p[1], sy = p[2], th = p[3], B = p[4], xm = p[5], ym = p[6];
    double st, ct;
    sincos(th, &st, &ct);
    const double cost2 = ct * ct, sint2 = st * st, sin2t = sin(2.0 * th), cos2t = cos(2.0 * th);
    const double xs2 = sx * sx, ys2 = sy * sy;
    const double a = 0.5 * ((cost2 / xs2) + (sint2 / ys2));
    const double b = 0.5 * ((sin2t / xs2) - (sin2t / ys2));
    const double c = 0.5 * ((sint2 / xs2) + (cost2 / ys2));
    const double xs3 = xs2 * sx, ys3 = ys2 * sy, dbt = cos2t * (1.0 / xs2 - 1.0 / ys2);
#pragma unroll
    for (int i = 0; i < NF * (NF + 1) / 2; ++i) JtJ[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NF; ++i) Jtr[i] = 0.0;
    double c2 = 0.0;
    for (int k = bx.lane; k < bx.npix; k += kWave) {
        const int row = k / bx.Wb, col = k - row * bx.Wb;
        const double dx = (double)row - xm, dy = (double)col - ym;
        const double dx2 = dx * dx, dxy = dx * dy, dy2 = dy * dy;
        const double E = exp(-((a * dx2) + (b * dxy) + (c * dy2)));
        const double g = A * E;
        const double w = (double)(1.0f / bx.sd[k]);
        const double r = w * ((g + B) - (double)bx.d[k]);
        double J[7];
        J[0] = E;
        J[1] = g * (cost2 * dx2 + sin2t * dxy + sint2 * dy2) / xs3;
        J[2] = g * (sint2 * dx2 - sin2t * dxy + cost2 * dy2) / ys3;
        J[3] = -g * (dbt * dxy + b * (dy2 - dx2));
        J[4] = 1.0;
        J[5] = g * (2.0 * a * dx + b * dy);
        J[6] = g * (b * dx + 2.0 * c * dy);
        c2 += r * r;
        int q = 0;
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const double wi = w * J[i];
            Jtr[i] += wi * r;
#pragma unroll
            for (int j = i; j < NF; ++j) JtJ[q++] += wi * (w * J[j]);
        }
    }
#pragma unroll
    for (int i = 0; i < NF * (NF + 1) / 2; ++i) JtJ[i] = wave_sum(JtJ[i]);
#pragma unroll
    for (int i = 0; i < NF; ++i) Jtr[i] = wave_sum(Jtr[i]);
    chi2 = wave_sum(c2);
}

// Cholesky factor (lower, in place) of the scaled matrix M; false if it is not positive definite.
template <int NF>
__device__ bool cholesky(double (&M)[NF][NF])
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
__device__ void chol_solve(const double (&L)[NF][NF], double (&x)[NF])
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

// M = D^-1 (JtJ + lambda diag(JtJ)) D^-1 with D = sqrt(diag(JtJ)): unit diagonal plus lambda.  False if a diagonal
// element is not positive and finite.
template <int NF>
__device__ bool scaled_matrix(const double (&JtJ)[NF * (NF + 1) / 2], double lambda, double (&D)[NF], double (&M)[NF][NF])
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

// One stage: Levenberg-Marquardt over the first NF parameters.  Ends ok when every step, in the scaled variables
// u_i = p_i D_i, is <= 1e-10 max(|u_i|, 1) with a damping factor <= 1; on that the standard errors
// sqrt(diag(JtJ^-1) chi^2 / err_dof) are written to err[0..NF).
template <int NF>
__device__ bool run_stage(const Box &bx, double (&p)[7], double (&err)[7], double &chi2, int max_iter, int err_dof, int &iters)
{
    double JtJ[NF * (NF + 1) / 2], Jtr[NF], JtJt[NF * (NF + 1) / 2], Jtrt[NF], D[NF], M[NF][NF], u[NF];
    accumulate<NF>(bx, p, JtJ, Jtr, chi2);
    iters = 0;
    if (!(chi2 < 1e300)) return false;                     // NaN or infinite
    // the damping follows the gain ratio (Nielsen's update: Madsen, Nielsen, Tingleff, Methods for non-linear least squares
    // problems, 2004): it crosses the flat valleys of a sub-pixel spike several times faster than a fixed x 10 / x 0.1 rule
    double lambda = 1e-3, nu = 2.0;
    bool converged = false;
    for (int it = 1; it <= max_iter; ++it) {
        iters = it;
        bool ok = scaled_matrix<NF>(JtJ, lambda, D, M);
        if (!ok) return false;
        ok = cholesky<NF>(M);
        if (!ok) {
            lambda *= nu;
            nu *= 2.0;
            if (lambda > 1e30) return false;
            continue;
        }
        double gs[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            gs[i] = Jtr[i] / D[i];
            u[i] = -gs[i];
        }
        chol_solve<NF>(M, u);
        double pt[7];
        bool small = lambda <= 1.0;
#pragma unroll
        for (int i = 0; i < 7; ++i) pt[i] = p[i];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            pt[i] = p[i] + u[i] / D[i];
            small = small && (fabs(u[i]) <= 1e-10 * fmax(fabs(p[i] * D[i]), 1.0));
        }
        double chi2t;
        accumulate<NF>(bx, pt, JtJt, Jtrt, chi2t);
        // near the minimum chi^2 no longer resolves a step (a step of u sigma changes it by u^2 / 2): a rise within its
        // rounding noise is accepted, or the last decades of the contraction would be rejected one by one (false for NaN)
        if (chi2t <= chi2 * (1.0 + 1e-14)) {
#pragma unroll
            for (int i = 0; i < 7; ++i) p[i] = pt[i];
#pragma unroll
            for (int i = 0; i < NF * (NF + 1) / 2; ++i) JtJ[i] = JtJt[i];
#pragma unroll
            for (int i = 0; i < NF; ++i) Jtr[i] = Jtrt[i];
            // gain ratio = actual / predicted decrease of chi^2; a predicted decrease within the rounding noise of chi^2
            // says nothing: the step counts as a full success
            double pred = 0.0;
#pragma unroll
            for (int i = 0; i < NF; ++i) pred += u[i] * (lambda * u[i] - gs[i]);
            const double rho = pred > 1e-12 * chi2 ? (chi2 - chi2t) / pred : 1.0;
            const double t = 2.0 * rho - 1.0;
            chi2 = chi2t;
            lambda = fmax(lambda * fmax(1.0 / 3.0, 1.0 - t * t * t), 1e-15);
            nu = 2.0;
        } else {
            lambda *= nu;
            nu *= 2.0;
            if (lambda > 1e30) return false;
        }
        if (small) {
            converged = true;
            break;
        }
    }
    if (!converged) return false;
    // the covariance: diag((D M D)^-1) with the undamped M
    if (!scaled_matrix<NF>(JtJ, 0.0, D, M)) return false;
    if (!cholesky<NF>(M)) return false;
    const double scale = chi2 / (double)err_dof;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        double e[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i) e[i] = (i == k) ? 1.0 : 0.0;
        chol_solve<NF>(M, e);
        err[k] = sqrt(e[k] / (D[k] * D[k]) * scale);
    }
#pragma unroll
    for (int k = NF; k < 7; ++k) err[k] = 0.0;
    return true;
}

__global__ void __launch_bounds__(kWave) gauss2d_fit_kernel(const float *__restrict__ img, long long H, long long W,
                                                            const int32_t *__restrict__ box_y, const int32_t *__restrict__ box_x,
                                                            const double *__restrict__ init, int n, int Wb, int max_iter,
                                                            double *__restrict__ rec, int32_t *__restrict__ okflag)
{
    extern __shared__ float lds[];
    __shared__ NpSumStack<float> pw_stack;
    __shared__ float mean_sh;
    const int star = blockIdx.x, lane = threadIdx.x;
    if (star >= n) return;
    const int npix = Wb * Wb;
    float *d = lds, *sd = lds + npix;
    double *out = rec + (long long)star * kRec;
    const long long y0 = box_y[star], x0 = box_x[star];
    double p[7], err[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        p[i] = init[(long long)star * 7 + i];
        err[i] = 0.0;
    }
    if (y0 < 0 || x0 < 0 || y0 + Wb > H || x0 + Wb > W) {        // a box outside the image: flagged, nothing is read
        if (lane == 0) {
            for (int i = 0; i < kRec; ++i) out[i] = i < 7 ? p[i] : 0.0;
            okflag[star] = -1;
        }
        return;
    }
    // the cut-out, and the values v != 1 of v = d > 0 ? d : 1 in pixel order (in sd's place, for their mean)
    int cnt = 0;
    for (int base = 0; base < npix; base += kWave) {
        const int k = base + lane;
        bool sel = false;
        float v = 1.f;
        if (k < npix) {
            const int row = k / Wb, col = k - row * Wb;
            const float x = img[(y0 + row) * W + (x0 + col)];
            d[k] = x;
            v = x > 0.f ? x : 1.f;
            sel = v != 1.f;
        }
        const unsigned long long m = __ballot(sel);
        if (sel) sd[cnt + __popcll(m & ((1ull << lane) - 1ull))] = v;
        cnt += __popcll(m);
    }
    __syncthreads();
    // np.mean of a contiguous float32 array: numpy's pairwise sum (np_exact.h; cnt <= 5776 is one piece), by one lane
    if (lane == 0) mean_sh = cnt > 0 ? np_pairwise_sum<float>(cnt, [&](int i) { return sd[i]; }, pw_stack) / (float)cnt : nanf("");
    __syncthreads();
    const float mean32 = mean_sh;
    const float rms32 = (float)sqrt((double)mean32);
    for (int k = lane; k < npix; k += kWave) {
        const float x = d[k];
        const float v = x > 0.f ? x : 1.f;
        sd[k] = v != 1.f ? sqrtf(v) : rms32;
    }
    __syncthreads();

    Box bx{d, sd, Wb, npix, lane};
    int it1 = 0, it2 = 0, it3 = 0, nfree = 4;
    double chi2 = nan("");
    bool ok = mean32 == mean32;                                  // an empty set: the mean is NaN, nothing is fitted
    if (ok) {
        // astropy scales the covariance by chi^2 / (len(y) - n_free) and len(y) of the 2-D grid is its row count
        ok = run_stage<4>(bx, p, err, chi2, max_iter, Wb - 4, it1);
        if (ok) {
            nfree = 5;
            ok = run_stage<5>(bx, p, err, chi2, max_iter, Wb - 5, it2);
        }
        if (ok) {
            nfree = 7;
            ok = run_stage<7>(bx, p, err, chi2, max_iter, Wb - 7, it3);
        }
        // the reduced chi^2 of the reference: deviations divided by the float32 standard deviations
        double c2 = 0.0;
        {
            const double A = p[0], sx = p[1], sy = p[2], th = p[3], B = p[4], xm = p[5], ym = p[6];
            double st, ct;
            sincos(th, &st, &ct);
            const double cost2 = ct * ct, sint2 = st * st, sin2t = sin(2.0 * th), xs2 = sx * sx, ys2 = sy * sy;
            const double a = 0.5 * ((cost2 / xs2) + (sint2 / ys2));
            const double b = 0.5 * ((sin2t / xs2) - (sin2t / ys2));
            const double c = 0.5 * ((sint2 / xs2) + (cost2 / ys2));
            for (int k = lane; k < npix; k += kWave) {
                const int row = k / Wb, col = k - row * Wb;
                const double dx = (double)row - xm, dy = (double)col - ym;
                const double m = A * exp(-((a * dx * dx) + (b * dx * dy) + (c * dy * dy))) + B;
                const double dev = ((double)d[k] - m) / (double)sd[k];
                c2 += dev * dev;
            }
        }
        chi2 = wave_sum(c2);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            out[i] = p[i];
            out[7 + i] = ok ? err[i] : 0.0;
        }
        out[14] = chi2 / (double)(npix - nfree);
        out[15] = chi2;
        out[16] = (double)it1;
        out[17] = (double)it2;
        out[18] = (double)it3;
        out[19] = (double)nfree;
        okflag[star] = ok ? 1 : 0;
    }
}

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_gauss2d_fit_f32(const float *img, int64_t height, int64_t width, const int32_t *box_y, const int32_t *box_x,
                                     const double *init, int32_t n, int32_t box_width, int32_t max_iter, double *out_rec,
                                     int32_t *out_ok, void *stream)
{
    if (n < 0) return fail(APGPU_EINVAL, "gauss2d_fit: negative star count %d", n);
    if (box_width < 12 || (box_width & 1)) return fail(APGPU_EINVAL, "gauss2d_fit: box width %d is odd or below 12", box_width);
    if (max_iter < 1) return fail(APGPU_EINVAL, "gauss2d_fit: max_iter %d is below 1", max_iter);
    if (height <= 0 || width <= 0) return fail(APGPU_EINVAL, "gauss2d_fit: bad shape [%lld, %lld]", (long long)height, (long long)width);
    if (box_width > kFitMaxBox)
        return fail(APGPU_EUNSUPPORTED, "gauss2d_fit: box width %d is above %d (initial FWHM too large)", box_width, kFitMaxBox);
    if (box_width > height || box_width > width)
        return fail(APGPU_EINVAL, "gauss2d_fit: box width %d does not fit a [%lld, %lld] image", box_width, (long long)height,
                    (long long)width);
    if (n == 0) return APGPU_OK;
    if (!img || !box_y || !box_x || !init || !out_rec || !out_ok) return fail(APGPU_EINVAL, "gauss2d_fit: NULL pointer argument");
    const size_t lds_bytes = (size_t)2 * box_width * box_width * sizeof(float);
    hipLaunchKernelGGL(gauss2d_fit_kernel, dim3((unsigned)n), dim3(kWave), lds_bytes, as_stream(stream), img, (long long)height,
                       (long long)width, box_y, box_x, init, (int)n, (int)box_width, (int)max_iter, out_rec, out_ok);
    return check_launch("gauss2d_fit");
}
