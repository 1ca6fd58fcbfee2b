// The effective PSF (F22) as a function: the separable Keys cubic convolution (a = -0.5) of an oversampled grid, with
// its analytic gradient, and the sample -> node rule.  Every kernel of epsf.hip evaluates the ePSF through this one function; it is
// plain C++ (float64, every operation rounds on its own) and compiles for the host as well.  tests/epsf_model.py states the same
// expressions in the same order.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIP__)
#define APGPU_EPSF_FN __host__ __device__ inline
#else
#define APGPU_EPSF_FN inline
#endif

namespace apgpu {

// The grid: float32 [G][G], G = 2 o R + 1; node (j, i) is the offset ((i - oR) / o, (j - oR) / o) pixels (x = column).
struct EpsfGrid {
    const float *E;
    int G, o, R;
};

// Keys' weights of the four nodes around a position t in [0, 1) past the second of them, and their derivatives in t.
APGPU_EPSF_FN void epsf_keys(double t, double (&w)[4], double (&d)[4])
{
    w[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    w[1] = (1.5 * t - 2.5) * t * t + 1.0;
    w[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    w[3] = (0.5 * t - 0.5) * t * t;
    d[0] = (-1.5 * t + 2.0) * t - 0.5;
    d[1] = (4.5 * t - 5.0) * t;
    d[2] = (-4.5 * t + 4.0) * t + 0.5;
    d[3] = (1.5 * t - 1.0) * t;
}

APGPU_EPSF_FN int epsf_clamp(int k, int G) { return k < 0 ? 0 : (k > G - 1 ? G - 1 : k); }

// E(dx, dy) and, with GRAD, dE/ddx and dE/ddy (per pixel).  0 (and a zero gradient) where |dx| <= R and |dy| <= R do not both
// hold, a NaN offset included.  Node indices are clamped to the grid's edge.
template <bool GRAD>
APGPU_EPSF_FN double epsf_eval(const EpsfGrid &g, double dx, double dy, double *gx, double *gy)
{
    const double Rr = (double)g.R;
    if (!(fabs(dx) <= Rr) || !(fabs(dy) <= Rr)) {
        if (GRAD) {
            *gx = 0.0;
            *gy = 0.0;
        }
        return 0.0;
    }
    const double oo = (double)g.o, c = (double)(g.o * g.R);
    const double u = dx * oo + c, v = dy * oo + c;
    const double fu = floor(u), fv = floor(v);
    const int iu = (int)fu, iv = (int)fv;
    double wx[4], dwx[4], wy[4], dwy[4];
    epsf_keys(u - fu, wx, dwx);
    epsf_keys(v - fv, wy, dwy);
    int xi[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) xi[b] = epsf_clamp(iu - 1 + b, g.G);
    double row[4], drow[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float *r = g.E + (long long)epsf_clamp(iv - 1 + a, g.G) * g.G;
        const double e0 = (double)r[xi[0]], e1 = (double)r[xi[1]], e2 = (double)r[xi[2]], e3 = (double)r[xi[3]];
        row[a] = ((wx[0] * e0 + wx[1] * e1) + wx[2] * e2) + wx[3] * e3;
        if (GRAD) drow[a] = ((dwx[0] * e0 + dwx[1] * e1) + dwx[2] * e2) + dwx[3] * e3;
    }
    if (GRAD) {
        *gx = (((wy[0] * drow[0] + wy[1] * drow[1]) + wy[2] * drow[2]) + wy[3] * drow[3]) * oo;
        *gy = (((dwy[0] * row[0] + dwy[1] * row[1]) + dwy[2] * row[2]) + dwy[3] * row[3]) * oo;
    }
    return ((wy[0] * row[0] + wy[1] * row[1]) + wy[2] * row[2]) + wy[3] * row[3];
}

// The node of pixel p on an axis for a star at x, less the grid's centre: floor((p - x) o + 0.5).
APGPU_EPSF_FN double epsf_node_of(long long p, double x, int o) { return floor(((double)p - x) * (double)o + 0.5); }

// The gather form of that rule: the one pixel p whose node is k (k relative to the centre, |x| <= 1e9).  The interval of p is
// 1 / o <= 1 wide, so at most one integer lies in it; its neighbours are tried as well and each is confirmed with the forward
// expression, so rounding in the inverse never decides.
APGPU_EPSF_FN bool epsf_pixel_of(int k, double x, int o, long long *p)
{
    const long long p0 = (long long)ceil(x + ((double)k - 0.5) / (double)o);
    for (long long q = p0 - 1; q <= p0 + 1; ++q) {
        if (epsf_node_of(q, x, o) == (double)k) {
            *p = q;
            return true;
        }
    }
    return false;
}

// A star that takes part in the accumulation: finite positive flux, finite sky, a centre within +-1e9 pixels (NaN: no).
APGPU_EPSF_FN bool epsf_star_usable(double f, double x, double y, double sky)
{
    return f > 0.0 && f < INFINITY && fabs(sky) < INFINITY && fabs(x) <= 1e9 && fabs(y) <= 1e9;
}

}  // namespace apgpu
