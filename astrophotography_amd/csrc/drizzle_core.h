// drizzle_core.h - the arithmetic of F14 for ONE output pixel (drizzle) and ONE input pixel (blot-and-compare rejection), stated
// once.  Everything here is __host__ __device__ and compiles as plain C++; csrc/drizzle.hip wraps it in the two kernels.  The
// definition is include/apgpu.h F14 / DESIGN 4.3k, restated in tests/drizzle_model.py.  No contraction: the units that include
// this are compiled with -ffp-contract=off; the one fma below adds an exact product, so it equals the multiply and the add.
#pragma once
#include <cmath>
#include <cstdint>

#include "np_exact.h"

namespace apgpu {

constexpr int kDrizzleFrameDoubles = 10;   // A0 .. A5, hx, hy, w, g
constexpr int kRejectFrameDoubles = 8;     // B0 .. B5, g, sigma

struct DrizzleImage {
    const float *frames;                   // [N][H][W]
    const uint8_t *mask;                   // [H][W] or NULL
    const uint8_t *frame_masks;            // [N][H][W] or NULL
    long long H, W;
    float hp;                              // pixfrac / 2
    float q;                               // float32(1 / pixfrac^2)
    unsigned cfa;                          // bit (j & 1) 2 + (i & 1) set: that cell position feeds this plane (0xf: no CFA)
};

// Overlaps of the footprint [l0, l1] with the four drops t - hp .. t + hp, t = 0 .. 3, in window coordinates, float32.
APGPU_HD inline void drizzle_overlaps(float l0, float l1, float hp, float o[4])
{
    for (int t = 0; t < 4; t++) {
        const float lo = fmaxf(l0, (float)t - hp), hi = fminf(l1, (float)t + hp);
        o[t] = fmaxf(0.0f, hi - lo);
    }
}

// How many taps along one axis can overlap a footprint of full width l = 2 h: the open interval of overlapping pixel centres is
// l + p long, so ceil(l + p) of them, and one more for the rounding of the window origin.  The taps behind it have a == 0.
APGPU_HD inline int drizzle_taps(double h, float hp)
{
    const double n = ceil(2.0 * h + 2.0 * (double)hp) + 1.0;
    return n < 4.0 ? (int)n : 4;           // (a NaN gives 4)
}

// Adds frame f's share of output pixel (u, v) to (num, den).  P: the frame's ten float64 parameters.
APGPU_HD inline void drizzle_frame(const DrizzleImage &im, long long f, const double *P, double u, double v, double &num, double &den)
{
    const double hx = P[6], hy = P[7];
    const float w = (float)P[8], g = (float)P[9];
    const double xc = (P[0] * u + P[1] * v) + P[2], yc = (P[3] * u + P[4] * v) + P[5];
    const double x0 = xc - hx, y0 = yc - hy;
    const double i0d = ceil(x0 - (double)im.hp), j0d = ceil(y0 - (double)im.hp);
    if (!(i0d >= -3.0 && i0d <= (double)(im.W - 1) && j0d >= -3.0 && j0d <= (double)(im.H - 1))) return;   // no tap on the frame (NaN too)
    float ox[4], oy[4];
    drizzle_overlaps((float)(x0 - i0d), (float)((xc + hx) - i0d), im.hp, ox);
    drizzle_overlaps((float)(y0 - j0d), (float)((yc + hy) - j0d), im.hp, oy);
    const long long i0 = (long long)i0d, j0 = (long long)j0d;
    const int ntx = drizzle_taps(hx, im.hp), nty = drizzle_taps(hy, im.hp);
    const size_t base = (size_t)f * (size_t)im.H * (size_t)im.W;
    for (int tj = 0; tj < nty; tj++) {
        const long long j = j0 + tj;
        if (j < 0 || j >= im.H) continue;
        for (int ti = 0; ti < ntx; ti++) {
            const long long i = i0 + ti;
            const float a = (ox[ti] * oy[tj]) * im.q;
            if (a == 0.0f || i < 0 || i >= im.W) continue;
            if (!((im.cfa >> (((int)j & 1) * 2 + ((int)i & 1))) & 1u)) continue;
            const size_t off = (size_t)j * (size_t)im.W + (size_t)i;
            if (im.mask && im.mask[off]) continue;
            if (im.frame_masks && im.frame_masks[base + off]) continue;
            const float val = im.frames[base + off];
            if (!is_finite(val)) continue;
            const float aw = a * w, gv = g * val;
            den = den + (double)aw;
            num = fma((double)aw, (double)gv, num);          // float32 x float32 is exact in float64
        }
    }
}

APGPU_HD inline void drizzle_finish(double num, double den, float &image, float &weight)
{
    image = den == 0.0 ? quiet_nan() : (float)(num / den);
    weight = (float)den;
}

// 1 when input pixel (c, r) of a frame, value val, is an outlier against the reference image.  P: the frame's eight parameters.
APGPU_HD inline uint8_t drizzle_reject_pixel(const float *ref, long long hr, long long wr, const double *P, double c, double r, float val,
                                             float k, float grow)
{
    const double xr = (P[0] * c + P[1] * r) + P[2], yr = (P[3] * c + P[4] * r) + P[5];
    const double x0d = floor(xr), y0d = floor(yr);
    if (!(x0d >= 0.0 && x0d <= (double)(wr - 2) && y0d >= 0.0 && y0d <= (double)(hr - 2))) return 0;       // a corner outside (NaN too)
    const float fx = (float)(xr - x0d), fy = (float)(yr - y0d);
    const float *p = ref + ((size_t)(long long)y0d * (size_t)wr + (size_t)(long long)x0d);
    const float p00 = p[0], p01 = p[1], p10 = p[wr], p11 = p[wr + 1];
    if (!(is_finite(p00) && is_finite(p01) && is_finite(p10) && is_finite(p11) && is_finite(val))) return 0;
    const float top = p00 + fx * (p01 - p00), bot = p10 + fx * (p11 - p10);
    const float b = top + fy * (bot - top);
    const float d = fmaxf(fmaxf(p00, p01), fmaxf(p10, p11)) - fminf(fminf(p00, p01), fminf(p10, p11));
    const float g = (float)P[6], sigma = (float)P[7];
    return fabsf(g * val - b) > k * sigma + grow * d ? 1 : 0;
}

}  // namespace apgpu
