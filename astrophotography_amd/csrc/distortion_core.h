// distortion_core.h - the polynomial distortion map of DESIGN 4.3e' for ONE point, stated once (include/apgpu.h F19; the host states
// it in astrophotography_amd/distortion.py, the model in tests/distortion_model.py).  Everything here is __host__ __device__ and
// compiles as plain C++.  No contraction: the units that include this are compiled with -ffp-contract=off.
//
//   X = Px(u, v), Y = Py(u, v), u = (x - x0) / L, v = (y - y0) / L; coefficient k of an axis belongs to u^i v^j, the monomials
//   running by total degree t = 0 .. D and within t by j = 0 .. t, i = t - j.  Powers by repeated multiplication, the sum from +0
//   in coefficient order: s = s + c[k] * (up[i] * vp[j]).  A first derivative likewise from (i * c[k]) * (up[i-1] * vp[j]) over the
//   terms with i >= 1, then divided by L.
//
// The degree is a template parameter: every loop unrolls, the powers stay in registers and the coefficient indices are constants.
#pragma once
#include "apgpu.h"
#include "np_exact.h"

namespace apgpu {

constexpr int kPolyMaxDegree = APGPU_POLY_MAX_DEGREE;

constexpr int poly_ncoef(int degree) { return (degree + 1) * (degree + 2) / 2; }

struct PolyFrame {                         // where the maps of one call live
    double x0, y0, L;
};

template <int D>
APGPU_HD inline void poly_powers(double u, double (&p)[D + 1])
{
    p[0] = 1.0;
#pragma unroll
    for (int i = 1; i <= D; ++i) p[i] = p[i - 1] * u;
}

// The (DU, DV)-th derivative with respect to (u, v), DU + DV <= 1.
template <int D, int DU, int DV>
APGPU_HD inline double poly_sum(const double *__restrict__ c, const double (&up)[D + 1], const double (&vp)[D + 1])
{
    double s = 0.0;
    int k = 0;
#pragma unroll
    for (int t = 0; t <= D; ++t) {
#pragma unroll
        for (int j = 0; j <= t; ++j, ++k) {
            const int i = t - j;
            if (i < DU || j < DV) continue;
            const double ck = DU ? (double)i * c[k] : (DV ? (double)j * c[k] : c[k]);
            s = s + ck * (up[i - DU] * vp[j - DV]);
        }
    }
    return s;
}

// c: one frame's [2][ncoef].
template <int D>
APGPU_HD inline void poly_eval(const double *__restrict__ c, const PolyFrame &fr, double x, double y, double &X, double &Y)
{
    double up[D + 1], vp[D + 1];
    poly_powers<D>((x - fr.x0) / fr.L, up);
    poly_powers<D>((y - fr.y0) / fr.L, vp);
    X = poly_sum<D, 0, 0>(c, up, vp);
    Y = poly_sum<D, 0, 0>(c + poly_ncoef(D), up, vp);
}

// ... and with it J = (dX/dx, dX/dy, dY/dx, dY/dy).
template <int D>
APGPU_HD inline void poly_eval_jacobian(const double *__restrict__ c, const PolyFrame &fr, double x, double y, double &X, double &Y,
                                        double (&J)[4])
{
    double up[D + 1], vp[D + 1];
    poly_powers<D>((x - fr.x0) / fr.L, up);
    poly_powers<D>((y - fr.y0) / fr.L, vp);
    const double *cy = c + poly_ncoef(D);
    X = poly_sum<D, 0, 0>(c, up, vp);
    Y = poly_sum<D, 0, 0>(cy, up, vp);
    J[0] = poly_sum<D, 1, 0>(c, up, vp) / fr.L;
    J[1] = poly_sum<D, 0, 1>(c, up, vp) / fr.L;
    J[2] = poly_sum<D, 1, 0>(cy, up, vp) / fr.L;
    J[3] = poly_sum<D, 0, 1>(cy, up, vp) / fr.L;
}

// The affine of one output tile (ops.poly_tile_affines): the map and its Jacobian at the reference image of the tile centre (xc, yc)
// of a grid with s output pixels per reference pixel, reference coordinate (xc + 0.5) / s - 0.5.  composed: the affine takes OUTPUT
// pixels (the Jacobian composed with the grid's scaling); otherwise it takes reference pixels, valid about that tile.
template <int D>
APGPU_HD inline void poly_tile_affine(const double *__restrict__ c, const PolyFrame &fr, double xc, double yc, double s, bool composed,
                                      double (&A)[6])
{
    const double xr = (xc + 0.5) / s - 0.5, yr = (yc + 0.5) / s - 0.5;
    double X, Y, J[4];
    poly_eval_jacobian<D>(c, fr, xr, yr, X, Y, J);
    const double px = composed ? xc : xr, py = composed ? yc : yr;
    A[0] = composed ? J[0] / s : J[0];
    A[1] = composed ? J[1] / s : J[1];
    A[2] = (X - A[0] * px) - A[1] * py;
    A[3] = composed ? J[2] / s : J[2];
    A[4] = composed ? J[3] / s : J[3];
    A[5] = (Y - A[3] * px) - A[4] * py;
}

}  // namespace apgpu
