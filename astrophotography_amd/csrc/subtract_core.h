// The kernel basis and the spatial polynomials of the optimal image subtraction (F23) as functions: plain C++ (float64,
// every operation rounds on its own) that compiles for the host and the device.  apgpu_subtract_basis_f64 builds the basis with
// them on the host, the apply kernel evaluates the spatial terms with them per pixel; tests/subtract_model.py states the same
// expressions in the same order (tools/subtract_core_check.cpp runs this header under the host sanitizers).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIP__)
#define APGPU_SUBTRACT_FN __host__ __device__ inline
#else
#define APGPU_SUBTRACT_FN inline
#endif

namespace apgpu {

constexpr int kSubMaxRadius = 15;          // APGPU_SUBTRACT_MAX_RADIUS
constexpr int kSubMaxBasis = 64;           // APGPU_SUBTRACT_MAX_BASIS
constexpr int kSubMaxDegree = 3;           // APGPU_SUBTRACT_MAX_DEGREE: of the spatial polynomials
constexpr int kSubMaxTerms = 10;           // (3 + 1)(3 + 2) / 2

// ---- the spatial terms ------------------------------------------------------------------------------------------------------
// The number of terms X^i Y^j with i + j <= d.
APGPU_SUBTRACT_FN int subtract_poly_count(int d) { return (d + 1) * (d + 2) / 2; }

// The normalised coordinate of pixel p on an axis of n pixels: (2 p - (n - 1)) / max(n - 1, 1), -1 .. 1 over the axis.
APGPU_SUBTRACT_FN double subtract_norm_coord(long long p, long long n)
{
    const long long m = n - 1 > 1 ? n - 1 : 1;
    return (double)(2 * p - (n - 1)) / (double)m;
}

// x^k by repeated multiplication from 1 (k multiplications; x^0 = 1).
APGPU_SUBTRACT_FN double subtract_ipow(double x, int k)
{
    double p = 1.0;
    for (int q = 0; q < k; ++q) p = p * x;
    return p;
}

// out[t] = X^i Y^j for i + j <= d, i then j ascending: (0,0), (0,1), .., (0,d), (1,0), ..  Returns the number of terms.
APGPU_SUBTRACT_FN int subtract_poly_terms(int d, double X, double Y, double *out)
{
    int t = 0;
    for (int i = 0; i <= d; ++i)
        for (int j = 0; i + j <= d; ++j) out[t++] = subtract_ipow(X, i) * subtract_ipow(Y, j);
    return t;
}

// ---- the kernel basis -------------------------------------------------------------------------------------------------------
// The number of functions of a basis of ng Gaussians with the polynomial degrees deg[g], or -1 if a degree is negative or the
// count passes kSubMaxBasis.
APGPU_SUBTRACT_FN int subtract_basis_count(int ng, const int32_t *deg)
{
    long long n = 0;
    for (int g = 0; g < ng; ++g) {
        if (deg[g] < 0 || deg[g] > kSubMaxBasis) return -1;
        n += (long long)(deg[g] + 1) * (deg[g] + 2) / 2;
        if (n > kSubMaxBasis) return -1;
    }
    return (int)n;
}

// One tap of a 1-D filter: exp(-u^2 / (2 sigma^2)) u^power.
APGPU_SUBTRACT_FN double subtract_filter_tap(double sigma, int power, int u)
{
    const double du = (double)u;
    return exp(-(du * du) / (2.0 * (sigma * sigma))) * subtract_ipow(du, power);
}

// The separable form of the basis.  Functions are ordered g, then i, then j ascending (i + j <= deg[g]); the 1-D filters g, then
// power ascending, filter f of Gaussian g and power p being filters[f][u + r] = subtract_filter_tap(sigma[g], p, u).  Function n =
// (g, i, j) is b(u, v) = filters[row[n]][u + r] filters[col[n]][v + r]: row[n] is the filter of (g, i) along x, col[n] that of
// (g, j) along y.  even[n] = 1 where i and j are both even; then scale[n] = 1 / sum b (the sum over v ascending of the sums over u
// ascending, from +0), else scale[n] = 1.  The basis function is B_n = scale[n] b_n, minus B_0 where even[n] and n > 0.
// Returns the number of functions (the caller has checked subtract_basis_count), *n_filters the number of filters.
inline int subtract_basis_build(int ng, const double *sigma, const int32_t *deg, int r, double *filters, int32_t *row, int32_t *col,
                                double *scale, int32_t *even, int *n_filters)
{
    const int kw = 2 * r + 1;
    int n = 0, f0 = 0;
    for (int g = 0; g < ng; ++g) {
        for (int p = 0; p <= deg[g]; ++p)
            for (int u = -r; u <= r; ++u) filters[(size_t)(f0 + p) * kw + (u + r)] = subtract_filter_tap(sigma[g], p, u);
        for (int i = 0; i <= deg[g]; ++i)
            for (int j = 0; i + j <= deg[g]; ++j) {
                row[n] = f0 + i;
                col[n] = f0 + j;
                even[n] = (i % 2 == 0 && j % 2 == 0) ? 1 : 0;
                scale[n] = 1.0;
                if (even[n]) {
                    double tot = 0.0;
                    for (int v = 0; v < kw; ++v) {
                        double line = 0.0;
                        for (int u = 0; u < kw; ++u) line = line + filters[(size_t)row[n] * kw + u] * filters[(size_t)col[n] * kw + v];
                        tot = tot + line;
                    }
                    scale[n] = 1.0 / tot;
                }
                ++n;
            }
        f0 += deg[g] + 1;
    }
    *n_filters = f0;
    return n;
}

// The dense basis function n at (u, v) from the separable form (what the fit's composite kernels are built from).
inline double subtract_basis_value(const double *filters, const int32_t *row, const int32_t *col, const double *scale, const int32_t *even,
                                   int r, int n, int u, int v)
{
    const int kw = 2 * r + 1;
    double b = scale[n] * (filters[(size_t)row[n] * kw + (u + r)] * filters[(size_t)col[n] * kw + (v + r)]);
    if (n > 0 && even[n]) b = b - scale[0] * (filters[(size_t)row[0] * kw + (u + r)] * filters[(size_t)col[0] * kw + (v + r)]);
    return b;
}

}  // namespace apgpu
