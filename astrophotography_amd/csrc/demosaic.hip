// demosaic.hip - F10: Bayer demosaic, white-balance scaling and the per-colour sums behind the white balance, on gfx950.
//
// The reference hands the interpolation to LibRaw (core/RawConv.py:401-587), which is not part of its tree, so the arithmetic is
// this project's own definition, restated in tests/demosaic_model.py.  Everything is float32, one rounding per
// operation, in the stated order, no contraction.
//
//   sample     s(r, c) = float32(max(raw - black[k], 0)) gain[k], k = pattern[(r & 1) 2 + (c & 1)] (R 0, G1 1, B 2, G2 3).
//              uint16: the subtraction is integer; float32: d = raw - black[k], d < 0 -> 0 (NaN stays NaN).
//   borders    the index is reflected about the edge sample (-1 -> 1, H -> H - 2), period 2 (H - 1): a tap keeps its colour.
//   taps       C centre; N S W E the edge neighbours; NW NE SW SE the diagonals; N2 S2 W2 E2 at distance 2 on the axes.
//              ns = N + S, we = W + E, d4 = (NW + NE) + (SW + SE), ns2 = N2 + S2, we2 = W2 + E2, e4 = ns + we, a4 = ns2 + we2
//   BILINEAR   at R/B: G = e4 0.25, other = d4 0.25; at G: colour of the row = we 0.5, colour of the column = ns 0.5
//   MHC        (sixteenths)   at R/B: G = ((8 C + 4 e4) - 2 a4) / 16, other = ((12 C + 4 d4) - 3 a4) / 16
//              at G: colour of the row    = (((10 C + 8 we) + ns2) - 2 (d4 + we2)) / 16
//                    colour of the column = (((10 C + 8 ns) + we2) - 2 (d4 + ns2)) / 16
//   SUPERPIXEL one pixel per 2 x 2 cell: R = s_R, G = (s_G1 + s_G2) 0.5, B = s_B
//   RCD        ratio-corrected, edge-directed (modelled on RCD 2.x, PARITY UNPINNED; tests/demosaic_rcd_model.py).  IEEE division;
//              eps = 2^-10, epssq = 2^-20; s folded to all positions, every plane outside the image computed on that extension.
//              t(n) the plane n steps along the direction; pair(g1, e1, g2, e2) = (g2 e1 + g1 e2) / (g1 + g2)
//              1 all sites, along V and H: h = (((t(-3) + t(3)) - (t(-1) + t(1))) - 3 (t(-2) + t(2))) + 6 s, q = h h,
//                stat = (q(-1) + q(+1)) + q(0), stat < epssq -> epssq (NaN stays); VH = V / (V + H);
//                vd = |0.5 - VH| < |0.5 - vn| ? vn : VH, vn = 0.25 d4(VH)
//              2 R/B sites: lpf = (s + 0.5 (ns + we)) + 0.25 d4(s)
//              3 G at R/B sites, towards N, S, W, E: grad = (((eps + |t(1) - t(-1)|) + |s - t(2)|) + |t(1) - t(3)|) + |t(2) - t(4)|,
//                est = t(1) (1 + (lpf - lpf(2)) / ((eps + lpf) + lpf(2))); V_est = pair(gN, eN, gS, eS), H_est = pair(gW, eW, gE, eE);
//                G = vd H_est + (1 - vd) V_est
//              4 R/B sites: P, Q the stat of step 1 along NW-SE, NE-SW; D = (P - Q) / (P + Q)   (= 2 PQ - 1: exactly odd in P, Q)
//              5 other of R/B at R/B sites: dd = |D| < |dn| ? dn : D, dn = 0.25 d4(D); towards each diagonal d:
//                grad = ((eps + |s(d) - s(-d)|) + |s(d) - s(3d)|) + |G - G(2d)|, est = s(d) - G(d);
//                P_est = pair(gNW, eNW, gSE, eSE), Q_est = pair(gNE, eNE, gSW, eSW); O = G + ((0.5 (1 - dd)) P_est + (0.5 (1 + dd)) Q_est)
//              6 R, B at G sites, X the colour at the R/B sites (s where native, else O), towards N, S, W, E:
//                grad = ((eps + |G - G(2)|) + |X(1) - X(-1)|) + |X(1) - X(3)|, est = X(1) - G(1); value = G + ((1 - vd) V_est + vd H_est)
//   outputs    RGB_F32; RGB_U16 =(uint16)(v > 0 ? (v < 65535 ? v : 65535) : 0); GREY_F32 = (0.299f R + 0.587f G) + 0.114f B;
//              DIRECT_F32 = s
//
// The stencil kernel: a workgroup of 256 lanes owns a tile of 16 rows x 256 columns.  It stages the scaled samples of the tile and
// a halo (2 rows above and below, 4 columns left and right: 2 are used, 4 keep the float4 reads aligned) in LDS: 20 x 264 floats.
// Wavefront w then produces rows 4 w .. 4 w + 3 of the tile, lane l the columns 4 l .. 4 l + 3: it reads its 8 x 8 window once
// (per row a float2, a float4 and a float2) and writes, per row and plane, one 16-byte store where the destination is aligned
// and the run is whole, single values otherwise.  The tile origin is even in both directions, so after unrolling the cell
// position of every pixel of a lane is a compile-time constant; whether position 0 is green is a template parameter and where
// red sits is a uniform kernel argument.
#include "common.h"

namespace apgpu {
namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 256, kTileH = 16;
constexpr int kPadX = 4, kPadY = 2;
constexpr int kLdsW = kTileW + 2 * kPadX;          // 264
constexpr int kLdsH = kTileH + 2 * kPadY;          // 20
constexpr int kRowsPerWave = kTileH / (kBlock / kWave);     // 4
constexpr int kWin = kRowsPerWave + 4;             // 8 window rows, 8 window columns
static_assert(kRowsPerWave == 4 && kTileW == 4 * kWave, "a lane owns a 4 x 4 block of the tile");

struct BayerArgs {         // everything by cell position p = (r & 1) 2 + (c & 1)
    int pattern[4];         // the colour of the position
    int black_i[4];         // black level and gain of that colour
    float black_f[4];
    float gain[4];
    int rpos;               // the position of red
};

// v[i] for a run-time i without an indexed (scratch) copy of v
template <typename T>
__device__ __forceinline__ T sel4(const T (&v)[4], int i)
{
    return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}

__device__ __forceinline__ float scaled_sample(uint16_t raw, int black_i, float, float gain)
{
    int v = (int)raw - black_i;
    v = v < 0 ? 0 : v;
    return (float)v * gain;
}

__device__ __forceinline__ float scaled_sample(float raw, int, float black_f, float gain)
{
    float d = raw - black_f;
    d = d < 0.0f ? 0.0f : d;
    return d * gain;
}

// Reflection about the edge sample, exact for -2 <= i <= n + 1 (n >= 2); anything further out is clamped (never used).
__device__ __forceinline__ long long reflect(long long i, long long n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    i = i < 0 ? -i : i;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

__device__ __forceinline__ uint16_t to_u16(float v)
{
    const float c = v > 0.0f ? (v < 65535.0f ? v : 65535.0f) : 0.0f;       // NaN -> 0
    return (uint16_t)(unsigned)c;
}

__device__ __forceinline__ float luma(float r, float g, float b) { return (0.299f * r + 0.587f * g) + 0.114f * b; }

// Writes n <= 4 consecutive values of one row: whole and aligned runs in one store.
__device__ __forceinline__ void store_run(float *dst, const float (&v)[4], int n)
{
    if (n == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < n; j++) dst[j] = v[j];
    }
}

__device__ __forceinline__ void store_run(uint16_t *dst, const float (&v)[4], int n)
{
    if (n == 4 && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
        uint2 w;
        w.x = (unsigned)to_u16(v[0]) | ((unsigned)to_u16(v[1]) << 16);
        w.y = (unsigned)to_u16(v[2]) | ((unsigned)to_u16(v[3]) << 16);
        *reinterpret_cast<uint2 *>(dst) = w;
    } else {
        for (int j = 0; j < n; j++) dst[j] = to_u16(v[j]);
    }
}

// One pixel of the window: i, j the pixel's place in the lane's 4 x 4 block (its cell position is (i & 1) 2 + (j & 1)).
template <int METHOD, bool G0, int I, int J>
__device__ __forceinline__ void pixel_rgb(const float (&w)[kWin][kWin], int rpos, float &r, float &g, float &b)
{
    constexpr int pos = (I & 1) * 2 + (J & 1);
    constexpr bool green = (((I ^ J) & 1) == 0) == G0;
    constexpr int y = I + 2, x = J + 2;
    const float c = w[y][x];
    const float ns = w[y - 1][x] + w[y + 1][x];
    const float we = w[y][x - 1] + w[y][x + 1];
    const float d4 = (w[y - 1][x - 1] + w[y - 1][x + 1]) + (w[y + 1][x - 1] + w[y + 1][x + 1]);
    if (METHOD == APGPU_DEMOSAIC_BILINEAR) {
        if (green) {
            const float h = we * 0.5f, v = ns * 0.5f;
            const bool row_is_red = rpos == (pos ^ 1);
            r = row_is_red ? h : v;
            g = c;
            b = row_is_red ? v : h;
        } else {
            const float gg = (ns + we) * 0.25f, o = d4 * 0.25f;
            const bool is_red = rpos == pos;
            r = is_red ? c : o;
            g = gg;
            b = is_red ? o : c;
        }
    } else {
        const float ns2 = w[y - 2][x] + w[y + 2][x];
        const float we2 = w[y][x - 2] + w[y][x + 2];
        if (green) {
            const float c10 = 10.0f * c;
            const float h = (((c10 + 8.0f * we) + ns2) - 2.0f * (d4 + we2)) * 0.0625f;
            const float v = (((c10 + 8.0f * ns) + we2) - 2.0f * (d4 + ns2)) * 0.0625f;
            const bool row_is_red = rpos == (pos ^ 1);
            r = row_is_red ? h : v;
            g = c;
            b = row_is_red ? v : h;
        } else {
            const float a4 = ns2 + we2;
            const float gg = ((8.0f * c + 4.0f * (ns + we)) - 2.0f * a4) * 0.0625f;
            const float o = ((12.0f * c + 4.0f * d4) - 3.0f * a4) * 0.0625f;
            const bool is_red = rpos == pos;
            r = is_red ? c : o;
            g = gg;
            b = is_red ? o : c;
        }
    }
}

template <int METHOD, bool G0, int I, int OUTPUT, typename OutT>
__device__ __forceinline__ void row_out(const float (&w)[kWin][kWin], int rpos, OutT *dst, size_t plane, int n)
{
    float r[4], g[4], b[4];
    pixel_rgb<METHOD, G0, I, 0>(w, rpos, r[0], g[0], b[0]);
    pixel_rgb<METHOD, G0, I, 1>(w, rpos, r[1], g[1], b[1]);
    pixel_rgb<METHOD, G0, I, 2>(w, rpos, r[2], g[2], b[2]);
    pixel_rgb<METHOD, G0, I, 3>(w, rpos, r[3], g[3], b[3]);
    if (OUTPUT == APGPU_DEMOSAIC_GREY_F32) {
        float yv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) yv[j] = luma(r[j], g[j], b[j]);
        store_run(dst, yv, n);
    } else {
        store_run(dst, r, n);
        store_run(dst + plane, g, n);
        store_run(dst + 2 * plane, b, n);
    }
}

// BILINEAR and MHC.  grid = (tiles across, tiles down, frames).
template <typename InT, int METHOD, int OUTPUT, bool G0, typename OutT>
__global__ __launch_bounds__(kBlock) void demosaic_kernel(const InT *__restrict__ mosaic, long long H, long long W, const BayerArgs a,
                                                         OutT *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float tile[kLdsH][kLdsW];
    constexpr int kPlanes = OUTPUT == APGPU_DEMOSAIC_GREY_F32 ? 1 : 3;
    const size_t plane = (size_t)H * (size_t)W;
    const long long tx0 = (long long)blockIdx.x * kTileW, ty0 = (long long)blockIdx.y * kTileH;
    const InT *src = mosaic + (size_t)blockIdx.z * plane;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;

    // stage: wavefront w fills LDS rows w, w + 4, ...; a lane the columns lane, lane + 64, ...
    for (int lr = wave; lr < kLdsH; lr += kBlock / kWave) {
        const long long gr = reflect(ty0 + lr - kPadY, H);
        const InT *row = src + (size_t)gr * (size_t)W;
        const bool odd_row = (gr & 1) != 0;
        const int bi0 = odd_row ? a.black_i[2] : a.black_i[0], bi1 = odd_row ? a.black_i[3] : a.black_i[1];
        const float bf0 = odd_row ? a.black_f[2] : a.black_f[0], bf1 = odd_row ? a.black_f[3] : a.black_f[1];
        const float g0 = odd_row ? a.gain[2] : a.gain[0], g1 = odd_row ? a.gain[3] : a.gain[1];
        for (int lc = lane; lc < kLdsW; lc += kWave) {
            const long long gc = reflect(tx0 + lc - kPadX, W);
            const bool odd = (gc & 1) != 0;
            tile[lr][lc] = scaled_sample(row[gc], odd ? bi1 : bi0, odd ? bf1 : bf0, odd ? g1 : g0);
        }
    }
    __syncthreads();

    const long long y0 = ty0 + wave * kRowsPerWave, x0 = tx0 + lane * 4;
    if (y0 >= H || x0 >= W) return;
    const int n = (int)(W - x0 < 4 ? W - x0 : 4);
    float w[kWin][kWin];
#pragma unroll
    for (int i = 0; i < kWin; i++) {
        const float *p = &tile[wave * kRowsPerWave + i][lane * 4 + kPadX - 2];
        const float2 l = *reinterpret_cast<const float2 *>(p);
        const float4 m = *reinterpret_cast<const float4 *>(p + 2);
        const float2 r = *reinterpret_cast<const float2 *>(p + 6);
        w[i][0] = l.x; w[i][1] = l.y; w[i][2] = m.x; w[i][3] = m.y; w[i][4] = m.z; w[i][5] = m.w; w[i][6] = r.x; w[i][7] = r.y;
    }
    OutT *dst = out + (size_t)blockIdx.z * kPlanes * plane + (size_t)y0 * (size_t)W + (size_t)x0;
    const int rows = (int)(H - y0 < kRowsPerWave ? H - y0 : kRowsPerWave);
    row_out<METHOD, G0, 0, OUTPUT>(w, a.rpos, dst, plane, n);
    if (rows > 1) row_out<METHOD, G0, 1, OUTPUT>(w, a.rpos, dst + (size_t)W, plane, n);
    if (rows > 2) row_out<METHOD, G0, 2, OUTPUT>(w, a.rpos, dst + 2 * (size_t)W, plane, n);
    if (rows > 3) row_out<METHOD, G0, 3, OUTPUT>(w, a.rpos, dst + 3 * (size_t)W, plane, n);
}

// ---- RCD --------------------------------------------------------------------------------------------------------------------
// Margins of the planes around the tile, in pixels: a plane of margin m covers rows -m .. kRcdTileH + m - 1 and columns
// -m .. kRcdTileW + m - 1 of the tile.  Each follows from what reads it: the output reads O at distance 3 and VH at 1; O reads D at
// 1 and G at 2 (diagonally); G reads VH at 1, lpf at 2 and s at 4; VH and D read s at 4; lpf reads s at 1.
constexpr int kRcdTileH = APGPU_DEMOSAIC_RCD_TILE_H, kRcdTileW = APGPU_DEMOSAIC_RCD_TILE_W;
constexpr int kRcdMO = 3, kRcdMD = kRcdMO + 1, kRcdMG = kRcdMO + 2, kRcdMVH = kRcdMG + 1, kRcdMLpf = kRcdMG + 2, kRcdMS = kRcdMVH + 4;
static_assert(kRcdMS == APGPU_DEMOSAIC_RCD_HALO && kRcdMS >= kRcdMD + 4 && kRcdMS >= kRcdMLpf + 1, "the halo is the reach of the samples");
static_assert(kRcdTileH * kRcdTileW == 8 * kBlock && kRcdTileW % 4 == 0 && kRcdTileH % 2 == 0 && kRcdMS % 2 == 0,
              "a lane owns a 2 x 4 block of the tile; the tile origin and the halo are even");
constexpr int kRcdSW = kRcdTileW + 2 * kRcdMS, kRcdSH = kRcdTileH + 2 * kRcdMS;              // 84 x 52: the samples
constexpr int kRcdVW = kRcdTileW + 2 * kRcdMVH, kRcdVH = kRcdTileH + 2 * kRcdMVH;            // 76 x 44: VH, at all sites
// lpf, G, D and O live on the R/B sites alone: one column parity per row, kept at ((x + kRcdHalfX) >> 1)
constexpr int kRcdHalfX = 8, kRcdHalfW = (kRcdTileW + 2 * kRcdHalfX) / 2;                   // 40
static_assert(kRcdHalfX % 2 == 0 && kRcdHalfX >= kRcdMLpf, "the half planes start on an even column left of every margin");
constexpr int kRcdLdsFloats = kRcdSW * kRcdSH + kRcdVW * kRcdVH + kRcdHalfW * ((kRcdTileH + 2 * kRcdMLpf) + (kRcdTileH + 2 * kRcdMG) + (kRcdTileH + 2 * kRcdMO));
static_assert(kRcdLdsFloats * 4 <= 64 * 1024, "the planes fit a static LDS allocation");
constexpr float kRcdEps = 0x1p-10f, kRcdEpsSq = 0x1p-20f;

// The folded reflection at any distance: period 2 (n - 1), n >= 2.
__device__ __forceinline__ long long fold(long long i, long long n)
{
    if (i >= 0 && i < n) return i;
    const long long period = 2 * (n - 1);
    long long m = i % period;
    m = m < 0 ? m + period : m;
    return m < n ? m : period - m;
}

// Step 1 on nine samples along one direction (a[4] the site): h at the site and its two neighbours, squared and summed.
__device__ __forceinline__ float rcd_h(const float (&a)[9], int i)
{
    return (((a[i - 3] + a[i + 3]) - (a[i - 1] + a[i + 1])) - 3.0f * (a[i - 2] + a[i + 2])) + 6.0f * a[i];
}

__device__ __forceinline__ float rcd_stat(const float (&a)[9])
{
    const float hm = rcd_h(a, 3), h0 = rcd_h(a, 4), hp = rcd_h(a, 5);
    const float stat = (hm * hm + hp * hp) + h0 * h0;
    return stat < kRcdEpsSq ? kRcdEpsSq : stat;            // a NaN stays
}

__device__ __forceinline__ float rcd_d4(float nw, float ne, float sw, float se) { return (nw + ne) + (sw + se); }

// The value itself, or the mean of its four diagonal neighbours where that is farther from 0.5.
__device__ __forceinline__ float rcd_disc(float centre, float near)
{
    return fabsf(0.5f - centre) < fabsf(0.5f - near) ? near : centre;
}

// The estimates of two opposite directions, each weighted by the other's gradient.
__device__ __forceinline__ float rcd_pair(float g1, float e1, float g2, float e2) { return (g2 * e1 + g1 * e2) / (g1 + g2); }

// Step 3 towards one side of the nine samples a (SGN -1: towards a[0]): the gradient and the ratio-corrected estimate.
template <int SGN>
__device__ __forceinline__ void rcd_green_towards(const float (&a)[9], float lpf, float lpf2, float &grad, float &est)
{
    const float c = a[4], t1 = a[4 + SGN], tm1 = a[4 - SGN], t2 = a[4 + 2 * SGN], t3 = a[4 + 3 * SGN], t4 = a[4 + 4 * SGN];
    grad = (((kRcdEps + fabsf(t1 - tm1)) + fabsf(c - t2)) + fabsf(t1 - t3)) + fabsf(t2 - t4);
    est = t1 * (1.0f + (lpf - lpf2) / ((kRcdEps + lpf) + lpf2));
}

// Step 6 for one colour at a green site: g the green there, dg[d] = eps + |G - G(2)|, x1[d], x3[d] the colour one and three steps
// towards d = N, S, W, E, g1[d] the green one step that way.
__device__ __forceinline__ float rcd_at_green(float g, float vd, const float (&dg)[4], const float (&x1)[4], const float (&x3)[4],
                                              const float (&g1)[4])
{
    float grad[4], est[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        grad[d] = (dg[d] + fabsf(x1[d] - x1[d ^ 1])) + fabsf(x1[d] - x3[d]);
        est[d] = x1[d] - g1[d];
    }
    const float v_est = rcd_pair(grad[0], est[0], grad[1], est[1]);
    const float h_est = rcd_pair(grad[2], est[2], grad[3], est[3]);
    return g + ((1.0f - vd) * v_est + vd * h_est);
}

// RCD in one launch: a workgroup of 256 lanes owns a tile of 32 rows x 64 columns and keeps every intermediate plane in LDS.  It
// stages the scaled samples of the tile and a halo of 10 on every side, then runs the steps of the definition over regions that
// shrink by each step's reach, a barrier between them; D takes the place of lpf, which is dead after the green step.  Last, a lane
// produces a 2 x 4 block of the tile (all cell positions compile-time constants) and stores it like the stencil kernel does.
// grid = (tiles across, tiles down, frames).
template <typename InT, int OUTPUT, bool G0, typename OutT>
__global__ __launch_bounds__(kBlock) void rcd_kernel(const InT *__restrict__ mosaic, long long H, long long W, const BayerArgs a,
                                                    OutT *__restrict__ out)
{
    __shared__ float s_[kRcdSH * kRcdSW];
    __shared__ float vh_[kRcdVH * kRcdVW];
    __shared__ float lpf_[(kRcdTileH + 2 * kRcdMLpf) * kRcdHalfW];          // then D
    __shared__ float g_[(kRcdTileH + 2 * kRcdMG) * kRcdHalfW];
    __shared__ float o_[(kRcdTileH + 2 * kRcdMO) * kRcdHalfW];
    constexpr int kPlanes = OUTPUT == APGPU_DEMOSAIC_GREY_F32 ? 1 : 3;
    constexpr int NG = G0 ? 1 : 0;                       // an R/B site has (x + y) & 1 == NG
    const size_t plane = (size_t)H * (size_t)W;
    const long long tx0 = (long long)blockIdx.x * kRcdTileW, ty0 = (long long)blockIdx.y * kRcdTileH;
    const InT *src = mosaic + (size_t)blockIdx.z * plane;
    const int tid = threadIdx.x;
    auto S = [&](int y, int x) -> float & { return s_[(y + kRcdMS) * kRcdSW + (x + kRcdMS)]; };
    auto VH = [&](int y, int x) -> float & { return vh_[(y + kRcdMVH) * kRcdVW + (x + kRcdMVH)]; };
    auto LPF = [&](int y, int x) -> float & { return lpf_[(y + kRcdMLpf) * kRcdHalfW + ((x + kRcdHalfX) >> 1)]; };
    auto D = [&](int y, int x) -> float & { return lpf_[(y + kRcdMD) * kRcdHalfW + ((x + kRcdHalfX) >> 1)]; };
    auto G = [&](int y, int x) -> float & { return g_[(y + kRcdMG) * kRcdHalfW + ((x + kRcdHalfX) >> 1)]; };
    auto O = [&](int y, int x) -> float & { return o_[(y + kRcdMO) * kRcdHalfW + ((x + kRcdHalfX) >> 1)]; };

    // the samples, folded at any distance from the image
    for (int i = tid; i < kRcdSH * kRcdSW; i += kBlock) {
        const int yi = i / kRcdSW, xi = i - yi * kRcdSW;
        const long long gr = fold(ty0 + yi - kRcdMS, H), gc = fold(tx0 + xi - kRcdMS, W);
        const int p = (int)(gr & 1) * 2 + (int)(gc & 1);
        s_[i] = scaled_sample(src[(size_t)gr * (size_t)W + (size_t)gc], sel4(a.black_i, p), sel4(a.black_f, p), sel4(a.gain, p));
    }
    __syncthreads();

    // 1: VH at all sites of its margin
    for (int i = tid; i < kRcdVH * kRcdVW; i += kBlock) {
        const int yi = i / kRcdVW, y = yi - kRcdMVH, x = i - yi * kRcdVW - kRcdMVH;
        float col[9], row[9];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            col[k] = S(y + k - 4, x);
            row[k] = S(y, x + k - 4);
        }
        const float v = rcd_stat(col), h = rcd_stat(row);
        vh_[i] = v / (v + h);
    }
    // 2: lpf at the R/B sites of its margin
    {
        constexpr int m = kRcdMLpf, nh = (kRcdTileW + 2 * m) / 2, n = (kRcdTileH + 2 * m) * nh;
        for (int i = tid; i < n; i += kBlock) {
            const int yi = i / nh, y = yi - m, x = 2 * (i - yi * nh) - m + (((y - m) & 1) ^ NG);
            const float ns = S(y - 1, x) + S(y + 1, x), we = S(y, x - 1) + S(y, x + 1);
            LPF(y, x) = (S(y, x) + 0.5f * (ns + we)) + 0.25f * rcd_d4(S(y - 1, x - 1), S(y - 1, x + 1), S(y + 1, x - 1), S(y + 1, x + 1));
        }
    }
    __syncthreads();

    // 3: green at the R/B sites
    {
        constexpr int m = kRcdMG, nh = (kRcdTileW + 2 * m) / 2, n = (kRcdTileH + 2 * m) * nh;
        for (int i = tid; i < n; i += kBlock) {
            const int yi = i / nh, y = yi - m, x = 2 * (i - yi * nh) - m + (((y - m) & 1) ^ NG);
            float col[9], row[9];
#pragma unroll
            for (int k = 0; k < 9; k++) {
                col[k] = S(y + k - 4, x);
                row[k] = S(y, x + k - 4);
            }
            const float vd = rcd_disc(VH(y, x), 0.25f * rcd_d4(VH(y - 1, x - 1), VH(y - 1, x + 1), VH(y + 1, x - 1), VH(y + 1, x + 1)));
            const float lpf = LPF(y, x);
            float gn, gs, gw, ge, en, es, ew, ee;
            rcd_green_towards<-1>(col, lpf, LPF(y - 2, x), gn, en);
            rcd_green_towards<1>(col, lpf, LPF(y + 2, x), gs, es);
            rcd_green_towards<-1>(row, lpf, LPF(y, x - 2), gw, ew);
            rcd_green_towards<1>(row, lpf, LPF(y, x + 2), ge, ee);
            const float v_est = rcd_pair(gn, en, gs, es), h_est = rcd_pair(gw, ew, ge, ee);
            G(y, x) = vd * h_est + (1.0f - vd) * v_est;
        }
    }
    __syncthreads();

    // 4: D = (P - Q) / (P + Q) at the R/B sites, over lpf
    {
        constexpr int m = kRcdMD, nh = (kRcdTileW + 2 * m) / 2, n = (kRcdTileH + 2 * m) * nh;
        for (int i = tid; i < n; i += kBlock) {
            const int yi = i / nh, y = yi - m, x = 2 * (i - yi * nh) - m + (((y - m) & 1) ^ NG);
            float nwse[9], nesw[9];
#pragma unroll
            for (int k = 0; k < 9; k++) {
                nwse[k] = S(y + k - 4, x + k - 4);
                nesw[k] = S(y - k + 4, x + k - 4);
            }
            const float p = rcd_stat(nwse), q = rcd_stat(nesw);
            D(y, x) = (p - q) / (p + q);
        }
    }
    __syncthreads();

    // 5: the other of R/B at the R/B sites
    {
        constexpr int m = kRcdMO, nh = (kRcdTileW + 2 * m) / 2, n = (kRcdTileH + 2 * m) * nh;
        for (int i = tid; i < n; i += kBlock) {
            const int yi = i / nh, y = yi - m, x = 2 * (i - yi * nh) - m + (((y - m) & 1) ^ NG);
            const float g = G(y, x), dc = D(y, x);
            const float dn = 0.25f * rcd_d4(D(y - 1, x - 1), D(y - 1, x + 1), D(y + 1, x - 1), D(y + 1, x + 1));
            const float dd = fabsf(dc) < fabsf(dn) ? dn : dc;
            float grad[4], est[4];                        // NW, SE, NE, SW
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const int dy = (d == 0 || d == 2) ? -1 : 1, dx = (d == 0 || d == 3) ? -1 : 1;
                const float t1 = S(y + dy, x + dx);
                grad[d] = ((kRcdEps + fabsf(t1 - S(y - dy, x - dx))) + fabsf(t1 - S(y + 3 * dy, x + 3 * dx))) + fabsf(g - G(y + 2 * dy, x + 2 * dx));
                est[d] = t1 - G(y + dy, x + dx);
            }
            const float p_est = rcd_pair(grad[0], est[0], grad[1], est[1]), q_est = rcd_pair(grad[2], est[2], grad[3], est[3]);
            O(y, x) = g + ((0.5f * (1.0f - dd)) * p_est + (0.5f * (1.0f + dd)) * q_est);
        }
    }
    __syncthreads();

    // 6 and the output: lane t the rows 2 (t / 16), + 1 and the columns 4 (t % 16) .. + 3 of the tile
    const int ly = 2 * (tid / (kRcdTileW / 4)), lx = 4 * (tid % (kRcdTileW / 4));
    const long long y0 = ty0 + ly, x0 = tx0 + lx;
    if (y0 >= H || x0 >= W) return;
    const int n = (int)(W - x0 < 4 ? W - x0 : 4);
    OutT *dst = out + (size_t)blockIdx.z * kPlanes * plane + (size_t)y0 * (size_t)W + (size_t)x0;
#pragma unroll
    for (int I = 0; I < 2; I++) {
        if (y0 + I >= H) break;
        float r[4], g[4], b[4];
#pragma unroll
        for (int J = 0; J < 4; J++) {
            const int pos = (I & 1) * 2 + (J & 1);
            const bool green = (((I ^ J) & 1) == 0) == G0;
            const int y = ly + I, x = lx + J;
            const float c = S(y, x);
            if (green) {
                const float vd = rcd_disc(VH(y, x), 0.25f * rcd_d4(VH(y - 1, x - 1), VH(y - 1, x + 1), VH(y + 1, x - 1), VH(y + 1, x + 1)));
                const float dg[4] = {kRcdEps + fabsf(c - S(y - 2, x)), kRcdEps + fabsf(c - S(y + 2, x)), kRcdEps + fabsf(c - S(y, x - 2)),
                                     kRcdEps + fabsf(c - S(y, x + 2))};
                const float g1[4] = {G(y - 1, x), G(y + 1, x), G(y, x - 1), G(y, x + 1)};
                // the colour of the row is native left and right, that of the column above and below; O holds the other
                const float row1[4] = {O(y - 1, x), O(y + 1, x), S(y, x - 1), S(y, x + 1)};
                const float row3[4] = {O(y - 3, x), O(y + 3, x), S(y, x - 3), S(y, x + 3)};
                const float col1[4] = {S(y - 1, x), S(y + 1, x), O(y, x - 1), O(y, x + 1)};
                const float col3[4] = {S(y - 3, x), S(y + 3, x), O(y, x - 3), O(y, x + 3)};
                const float of_row = rcd_at_green(c, vd, dg, row1, row3, g1), of_col = rcd_at_green(c, vd, dg, col1, col3, g1);
                const bool row_is_red = a.rpos == (pos ^ 1);
                r[J] = row_is_red ? of_row : of_col;
                g[J] = c;
                b[J] = row_is_red ? of_col : of_row;
            } else {
                const float o = O(y, x);
                const bool is_red = a.rpos == pos;
                r[J] = is_red ? c : o;
                g[J] = G(y, x);
                b[J] = is_red ? o : c;
            }
        }
        OutT *row = dst + (size_t)I * (size_t)W;
        if (OUTPUT == APGPU_DEMOSAIC_GREY_F32) {
            float yv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) yv[j] = luma(r[j], g[j], b[j]);
            store_run(row, yv, n);
        } else {
            store_run(row, r, n);
            store_run(row + plane, g, n);
            store_run(row + 2 * plane, b, n);
        }
    }
}

// SUPERPIXEL: a lane owns four consecutive output pixels of one output row (8 x 2 samples).  grid.y = frames.
template <typename InT, int OUTPUT, typename OutT>
__global__ __launch_bounds__(kBlock) void superpixel_kernel(const InT *__restrict__ mosaic, long long H, long long W, const BayerArgs a,
                                                           OutT *__restrict__ out)
{
    constexpr int kPlanes = OUTPUT == APGPU_DEMOSAIC_GREY_F32 ? 1 : 3;
    const long long h = H / 2, w = W / 2;
    const long long groups_per_row = (w + 3) / 4;
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= groups_per_row * h) return;
    const long long r = gid / groups_per_row;
    const long long x0 = (gid - r * groups_per_row) * 4;
    const int n = (int)(w - x0 < 4 ? w - x0 : 4);
    const InT *src = mosaic + (size_t)blockIdx.y * (size_t)H * (size_t)W + (size_t)(2 * r) * (size_t)W + (size_t)(2 * x0);
    float rr[4], gg[4], bb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};          // by cell position
        if (j < n) {
#pragma unroll
            for (int p = 0; p < 4; p++)
                s[p] = scaled_sample(src[(size_t)(p >> 1) * (size_t)W + (size_t)(2 * j + (p & 1))], a.black_i[p], a.black_f[p], a.gain[p]);
        }
        const bool main_diag = a.rpos == 0 || a.rpos == 3;          // red and blue at positions 0 and 3: the greens at 1 and 2
        rr[j] = sel4(s, a.rpos);
        gg[j] = (main_diag ? s[1] + s[2] : s[0] + s[3]) * 0.5f;    // (float addition commutes: G1 + G2 either way round)
        bb[j] = sel4(s, a.rpos ^ 3);
    }
    const size_t plane = (size_t)h * (size_t)w;
    OutT *dst = out + (size_t)blockIdx.y * kPlanes * plane + (size_t)r * (size_t)w + (size_t)x0;
    if (OUTPUT == APGPU_DEMOSAIC_GREY_F32) {
        float yv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) yv[j] = luma(rr[j], gg[j], bb[j]);
        store_run(dst, yv, n);
    } else {
        store_run(dst, rr, n);
        store_run(dst + plane, gg, n);
        store_run(dst + 2 * plane, bb, n);
    }
}

// DIRECT_F32: the scaled sample itself.  A lane owns four consecutive pixels of one row.  grid.y = frames.
template <typename InT>
__global__ __launch_bounds__(kBlock) void direct_kernel(const InT *__restrict__ mosaic, long long H, long long W, const BayerArgs a,
                                                       float *__restrict__ out)
{
    const long long groups_per_row = (W + 3) / 4;
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= groups_per_row * H) return;
    const long long r = gid / groups_per_row;
    const long long x0 = (gid - r * groups_per_row) * 4;
    const int n = (int)(W - x0 < 4 ? W - x0 : 4);
    const size_t off = (size_t)blockIdx.y * (size_t)H * (size_t)W + (size_t)r * (size_t)W + (size_t)x0;
    const bool odd_row = (r & 1) != 0;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {                           // x0 is even: the column parity is that of j
        const int p0 = j & 1, p1 = 2 + (j & 1);
        v[j] = j < n ? scaled_sample(mosaic[off + j], odd_row ? a.black_i[p1] : a.black_i[p0], odd_row ? a.black_f[p1] : a.black_f[p0],
                                     odd_row ? a.gain[p1] : a.gain[p0])
                     : 0.0f;
    }
    store_run(out + off, v, n);
}

// The sums of the black-subtracted samples of each colour over the rows r0 .. r1 and columns c0 .. c1.  The column stride of a
// lane is even, so a lane meets one column parity; it keeps one accumulator per row parity.  Integer sums are exact in any order.
template <typename InT, typename SumT>
__global__ __launch_bounds__(kBlock) void channel_sums_kernel(const InT *__restrict__ mosaic, long long W, long long r0, long long r1,
                                                             long long c0, long long c1, const BayerArgs a, SumT *__restrict__ sums,
                                                             unsigned long long *__restrict__ counts)
{
    __shared__ SumT ssum[4];
    __shared__ unsigned long long scnt[4];
    if (threadIdx.x < 4) {
        ssum[threadIdx.x] = (SumT)0;
        scnt[threadIdx.x] = 0;
    }
    __syncthreads();
    SumT acc0 = (SumT)0, acc1 = (SumT)0;                   // even rows, odd rows
    unsigned long long cnt0 = 0, cnt1 = 0;
    const long long cfirst = c0 + (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long cstep = (long long)gridDim.x * kBlock;
    const int cp = (int)(cfirst & 1);
    for (long long r = r0 + blockIdx.y; r <= r1; r += gridDim.y) {
        const InT *row = mosaic + (size_t)r * (size_t)W;
        const bool odd_row = (r & 1) != 0;
        const int pos = (odd_row ? 2 : 0) + cp;
        const int black_i = sel4(a.black_i, pos);
        const float black_f = sel4(a.black_f, pos);
        SumT s = (SumT)0;
        unsigned long long m = 0;
        for (long long c = cfirst; c <= c1; c += cstep) {
            if (sizeof(InT) == 2) {
                int v = (int)row[c] - black_i;
                s += (SumT)(v < 0 ? 0 : v);
                m++;
            } else {
                float d = (float)row[c] - black_f;
                d = d < 0.0f ? 0.0f : d;
                if ((__float_as_uint(d) & 0x7f800000u) != 0x7f800000u) {
                    s += (SumT)d;
                    m++;
                }
            }
        }
        if (odd_row) {
            acc1 += s;
            cnt1 += m;
        } else {
            acc0 += s;
            cnt0 += m;
        }
    }
    if (cnt0) {
        const int k = sel4(a.pattern, cp);
        atomicAdd(&ssum[k], acc0);
        atomicAdd(&scnt[k], cnt0);
    }
    if (cnt1) {
        const int k = sel4(a.pattern, 2 + cp);
        atomicAdd(&ssum[k], acc1);
        atomicAdd(&scnt[k], cnt1);
    }
    __syncthreads();
    if (threadIdx.x < 4 && scnt[threadIdx.x]) {
        atomicAdd(&sums[threadIdx.x], ssum[threadIdx.x]);
        atomicAdd(&counts[threadIdx.x], scnt[threadIdx.x]);
    }
}

// pattern: a permutation of 0 .. 3 with red and blue on one diagonal.  black: integers 0 .. 65535 for uint16 input.
int bayer_args(const char *what, const int32_t *pattern_host, const float *black_host, const float *gain_host, int dtype, BayerArgs &a)
{
    unsigned seen = 0;
    a.rpos = 0;
    int bpos = 0, pos_of[4] = {0, 0, 0, 0};
    for (int p = 0; p < 4; p++) {
        const int k = pattern_host[p];
        if (k < 0 || k > 3) return fail(APGPU_EINVAL, "%s: pattern entries must be 0 .. 3", what);
        seen |= 1u << k;
        a.pattern[p] = k;
        pos_of[k] = p;
        if (k == 0) a.rpos = p;
        if (k == 2) bpos = p;
    }
    if (seen != 0xfu || (a.rpos ^ bpos) != 3)
        return fail(APGPU_EINVAL, "%s: pattern (%d, %d, %d, %d) is not a Bayer arrangement (a permutation of 0 .. 3, red and blue on one diagonal)",
                    what, pattern_host[0], pattern_host[1], pattern_host[2], pattern_host[3]);
    for (int k = 0; k < 4; k++) {
        const int p = pos_of[k];
        const float b = black_host ? black_host[k] : 0.0f;
        a.black_f[p] = b;
        a.black_i[p] = 0;
        if (dtype == APGPU_U16) {
            if (!(b >= 0.0f && b <= 65535.0f) || b != (float)(int)b)
                return fail(APGPU_EINVAL, "%s: a black level of uint16 data must be an integer 0 .. 65535, got %g", what, (double)b);
            a.black_i[p] = (int)b;
        }
        a.gain[p] = gain_host ? gain_host[k] : 1.0f;
    }
    return APGPU_OK;
}

template <typename InT, int METHOD, int OUTPUT, typename OutT>
void launch_stencil(bool g0, dim3 grid, hipStream_t s, const InT *in, long long H, long long W, const BayerArgs &a, OutT *out)
{
    if (g0) hipLaunchKernelGGL((demosaic_kernel<InT, METHOD, OUTPUT, true, OutT>), grid, dim3(kBlock), 0, s, in, H, W, a, out);
    else hipLaunchKernelGGL((demosaic_kernel<InT, METHOD, OUTPUT, false, OutT>), grid, dim3(kBlock), 0, s, in, H, W, a, out);
}

template <typename InT, int OUTPUT, typename OutT>
void launch_method(int method, bool g0, dim3 tiles, dim3 lanes, hipStream_t s, const InT *in, long long H, long long W, const BayerArgs &a,
                   OutT *out)
{
    if (method == APGPU_DEMOSAIC_RCD) {
        if (g0) hipLaunchKernelGGL((rcd_kernel<InT, OUTPUT, true, OutT>), tiles, dim3(kBlock), 0, s, in, H, W, a, out);
        else hipLaunchKernelGGL((rcd_kernel<InT, OUTPUT, false, OutT>), tiles, dim3(kBlock), 0, s, in, H, W, a, out);
    } else if (method == APGPU_DEMOSAIC_BILINEAR) launch_stencil<InT, APGPU_DEMOSAIC_BILINEAR, OUTPUT, OutT>(g0, tiles, s, in, H, W, a, out);
    else if (method == APGPU_DEMOSAIC_MHC) launch_stencil<InT, APGPU_DEMOSAIC_MHC, OUTPUT, OutT>(g0, tiles, s, in, H, W, a, out);
    else hipLaunchKernelGGL((superpixel_kernel<InT, OUTPUT, OutT>), lanes, dim3(kBlock), 0, s, in, H, W, a, out);
}

template <typename InT>
void launch_output(int method, int output, bool g0, dim3 tiles, dim3 lanes, hipStream_t s, const InT *in, long long H, long long W,
                   const BayerArgs &a, void *out)
{
    if (output == APGPU_DEMOSAIC_DIRECT_F32) hipLaunchKernelGGL((direct_kernel<InT>), lanes, dim3(kBlock), 0, s, in, H, W, a, (float *)out);
    else if (output == APGPU_DEMOSAIC_RGB_F32) launch_method<InT, APGPU_DEMOSAIC_RGB_F32, float>(method, g0, tiles, lanes, s, in, H, W, a, (float *)out);
    else if (output == APGPU_DEMOSAIC_RGB_U16) launch_method<InT, APGPU_DEMOSAIC_RGB_U16, uint16_t>(method, g0, tiles, lanes, s, in, H, W, a, (uint16_t *)out);
    else launch_method<InT, APGPU_DEMOSAIC_GREY_F32, float>(method, g0, tiles, lanes, s, in, H, W, a, (float *)out);
}

constexpr long long kMaxGridZ = 65535;

}  // namespace
}  // namespace apgpu

using namespace apgpu;

extern "C" int apgpu_bayer_demosaic(const void *mosaic, int32_t dtype, int64_t n_frames, int64_t height, int64_t width,
                                    const int32_t *pattern_host, const float *black_host, const float *gain_host, int32_t method,
                                    int32_t output, void *out, void *stream)
{
    if (!mosaic || !out || !pattern_host) return fail(APGPU_EINVAL, "bayer_demosaic: NULL pointer argument");
    if (dtype != APGPU_U16 && dtype != APGPU_F32) return fail(APGPU_EINVAL, "bayer_demosaic: dtype %d (uint16 or float32)", dtype);
    if (n_frames <= 0 || height < 2 || width < 2)
        return fail(APGPU_EINVAL, "bayer_demosaic: %lld frames of %lld x %lld (at least 1 of 2 x 2)", (long long)n_frames, (long long)height, (long long)width);
    if (output < APGPU_DEMOSAIC_RGB_F32 || output > APGPU_DEMOSAIC_DIRECT_F32) return fail(APGPU_EINVAL, "bayer_demosaic: output %d", output);
    const bool direct = output == APGPU_DEMOSAIC_DIRECT_F32;
    const bool known = (method >= APGPU_DEMOSAIC_BILINEAR && method <= APGPU_DEMOSAIC_SUPERPIXEL) || method == APGPU_DEMOSAIC_RCD;          // 3 is no method
    if (!direct && !known) return fail(APGPU_EINVAL, "bayer_demosaic: method %d", method);
    const bool super = !direct && method == APGPU_DEMOSAIC_SUPERPIXEL;
    if (super && ((height | width) & 1)) return fail(APGPU_EINVAL, "bayer_demosaic: SUPERPIXEL needs even height and width, got %lld x %lld", (long long)height, (long long)width);
    const size_t in_size = dtype == APGPU_U16 ? 2 : 4, out_size = output == APGPU_DEMOSAIC_RGB_U16 ? 2 : 4;
    if ((reinterpret_cast<uintptr_t>(mosaic) & (in_size - 1)) || (reinterpret_cast<uintptr_t>(out) & (out_size - 1)))
        return fail(APGPU_EINVAL, "bayer_demosaic: mosaic and out must be aligned to their element size");
    BayerArgs a;
    const int rc = bayer_args("bayer_demosaic", pattern_host, black_host, gain_host, dtype, a);
    if (rc != APGPU_OK) return rc;
    const bool g0 = (a.pattern[0] & 1) != 0;
    const long long oh = super ? height / 2 : height, ow = super ? width / 2 : width;
    const long long lane_blocks = ((ow + 3) / 4 * oh + kBlock - 1) / kBlock;
    const bool rcd = !direct && method == APGPU_DEMOSAIC_RCD;
    const long long tile_w = rcd ? kRcdTileW : kTileW, tile_h = rcd ? kRcdTileH : kTileH;
    const long long tiles_x = (width + tile_w - 1) / tile_w, tiles_y = (height + tile_h - 1) / tile_h;
    if (lane_blocks > 0x7fffffffLL || tiles_x > 0x7fffffffLL || tiles_y > kMaxGridZ)
        return fail(APGPU_EUNSUPPORTED, "bayer_demosaic: image of %lld x %lld is too large", (long long)height, (long long)width);
    const size_t in_frame = (size_t)height * (size_t)width * in_size;
    const size_t out_frame = (size_t)oh * (size_t)ow * out_size * (output == APGPU_DEMOSAIC_RGB_F32 || output == APGPU_DEMOSAIC_RGB_U16 ? 3 : 1);
    hipStream_t s = as_stream(stream);
    for (long long f0 = 0; f0 < n_frames; f0 += kMaxGridZ) {               // one launch up to 65535 frames
        const unsigned nf = (unsigned)(n_frames - f0 < kMaxGridZ ? n_frames - f0 : kMaxGridZ);
        const dim3 tiles((unsigned)tiles_x, (unsigned)tiles_y, nf), lanes((unsigned)lane_blocks, nf);
        const char *in = static_cast<const char *>(mosaic) + (size_t)f0 * in_frame;
        char *o = static_cast<char *>(out) + (size_t)f0 * out_frame;
        if (dtype == APGPU_U16) launch_output<uint16_t>(method, output, g0, tiles, lanes, s, (const uint16_t *)in, height, width, a, o);
        else launch_output<float>(method, output, g0, tiles, lanes, s, (const float *)in, height, width, a, o);
    }
    return check_launch("bayer_demosaic");
}

extern "C" int apgpu_bayer_channel_sums(const void *mosaic, int32_t dtype, int64_t height, int64_t width, const int32_t *pattern_host,
                                        const float *black_host, const int64_t *rect_host, void *sums, int64_t *counts, void *stream)
{
    if (!mosaic || !pattern_host || !rect_host || !sums || !counts) return fail(APGPU_EINVAL, "bayer_channel_sums: NULL pointer argument");
    if (dtype != APGPU_U16 && dtype != APGPU_F32) return fail(APGPU_EINVAL, "bayer_channel_sums: dtype %d (uint16 or float32)", dtype);
    if (height < 2 || width < 2) return fail(APGPU_EINVAL, "bayer_channel_sums: image of %lld x %lld (at least 2 x 2)", (long long)height, (long long)width);
    if ((reinterpret_cast<uintptr_t>(sums) & 7) || (reinterpret_cast<uintptr_t>(counts) & 7) ||
        (reinterpret_cast<uintptr_t>(mosaic) & (dtype == APGPU_U16 ? 1 : 3)))
        return fail(APGPU_EINVAL, "bayer_channel_sums: sums and counts must be 8-byte aligned, mosaic to its element size");
    BayerArgs a;
    const int rc = bayer_args("bayer_channel_sums", pattern_host, black_host, nullptr, dtype, a);
    if (rc != APGPU_OK) return rc;
    const long long r0 = rect_host[0] < 0 ? 0 : rect_host[0], r1 = rect_host[1] > height - 1 ? height - 1 : rect_host[1];
    const long long c0 = rect_host[2] < 0 ? 0 : rect_host[2], c1 = rect_host[3] > width - 1 ? width - 1 : rect_host[3];
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(sums, 0, 32, s) != hipSuccess || hipMemsetAsync(counts, 0, 32, s) != hipSuccess)
        return fail(APGPU_ELAUNCH, "bayer_channel_sums: hipMemsetAsync failed");
    if (r1 < r0 || c1 < c0) return APGPU_OK;                               // an empty region: zeros
    const long long bx = (c1 - c0 + kBlock) / kBlock, by = r1 - r0 + 1;
    const dim3 grid((unsigned)(bx < 8 ? bx : 8), (unsigned)(by < 1024 ? by : 1024));
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counts);
    if (dtype == APGPU_U16)
        hipLaunchKernelGGL((channel_sums_kernel<uint16_t, unsigned long long>), grid, dim3(kBlock), 0, s, (const uint16_t *)mosaic, (long long)width,
                           r0, r1, c0, c1, a, (unsigned long long *)sums, cnt);
    else
        hipLaunchKernelGGL((channel_sums_kernel<float, double>), grid, dim3(kBlock), 0, s, (const float *)mosaic, (long long)width, r0, r1, c0, c1,
                           a, (double *)sums, cnt);
    return check_launch("bayer_channel_sums");
}
