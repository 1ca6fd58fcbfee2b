// np_exact.h - the two pieces of arithmetic the bit-exact statistics rest on, stated once: the order in which numpy's
// np.add.reduce adds a contiguous 1-D array, and the order-preserving integer key of a float that every exact median is
// selected on.  Plus the finiteness test and the wavefront sum the same kernels share.
//
// Everything but wave_sum is __host__ __device__ and compiles as plain C++ (tools/np_exact_check.cpp runs it on the host
// against NumPy itself, tests/test_host_cpu.py).  No contraction anywhere: the units that include this are compiled with
// -ffp-contract=off, and every add below is a separately rounded one.
//
// np.add.reduce (numpy/_core/src/umath/loops_utils.h.src, pairwise_sum, PW_BLOCKSIZE 128, under the 8192-element buffer of
// the reduction): the array is cut into pieces of 8192; total = ((0 + piece0) + piece1) + ...; a piece of more than 128
// values is the sum of its two halves, the left one n / 2 rounded down to a multiple of 8; a piece or half of 8 .. 128
// values (a leaf) keeps 8 strided accumulators r[k] += a[8 j + k], folds them ((r0 + r1) + (r2 + r3)) + ((r4 + r5) +
// (r6 + r7)) and adds the n % 8 last values in order; fewer than 8 values are added in order from 0.
#pragma once

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define APGPU_HD __host__ __device__
#else
#define APGPU_HD
#endif

namespace apgpu {

// the bits of x as another type of the same size (what __float_as_uint and its kin do, on the host too)
template <typename To, typename From>
APGPU_HD inline To bits_as(const From &x)
{
    static_assert(sizeof(To) == sizeof(From), "");
    To t;
    __builtin_memcpy(&t, &x, sizeof t);
    return t;
}

// Order-preserving key: a < b (as floats, no NaN) <=> to(a) < to(b) (as unsigned); -0 sorts just below +0.
template <typename T> struct OrderKey;
template <> struct OrderKey<float> {
    using U = unsigned;
    static constexpr int bits = 32;
    APGPU_HD static U to(float x)
    {
        const U b = bits_as<U>(x);
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    APGPU_HD static float from(U k) { return bits_as<float>((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
};
template <> struct OrderKey<double> {
    using U = unsigned long long;
    static constexpr int bits = 64;
    APGPU_HD static U to(double x)
    {
        const U b = bits_as<U>(x);
        return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    }
    APGPU_HD static double from(U k) { return bits_as<double>((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k); }
};

// neither infinite nor NaN: the exponent bits are not all ones.  (By reference: by value, composite_kernel, which tests the
// elements of an array, came out 4 VGPRs and one wavefront per SIMD worse.)
APGPU_HD inline bool is_finite(const float &x) { return (bits_as<unsigned>(x) & 0x7f800000u) != 0x7f800000u; }
APGPU_HD inline bool is_finite(const double &x)
{
    return (bits_as<unsigned long long>(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
// the NaN that marks a pixel without data in every float32 output: quiet, positive, no payload
APGPU_HD inline float quiet_nan() { return bits_as<float>(0x7fc00000u); }

// numpy's sum of n <= 128 terms f(0) .. f(n - 1).  The index is 64-bit so that f(i + k) over an array is base + constant
// and the eight loads of a round stay one or two wide loads, as in a loop over a pointer.  The round loop is kept rolled:
// a leaf of known length (flat_piece_sums_kernel, 128 per lane) is otherwise unrolled whole, all 128 loads hoisted (276
// VGPRs and spills).
template <typename T, typename F>
APGPU_HD inline T np_leaf_sum(int n, F f)
{
    if (n < 8) {
        T res = (T)0;
        for (long long i = 0; i < n; i++) res = res + f(i);
        return res;
    }
    T r[8];
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = f(k);
    long long i = 8;
#pragma unroll 1
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; k++) r[k] = r[k] + f(i + k);
    }
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res = res + f(i);
    return res;
}

// the left half of a piece or half of n > 128 values: n / 2 rounded down to a multiple of 8 (the right half is the rest)
APGPU_HD inline int np_left_half(int n)
{
    const int n2 = n / 2;
    return n2 - n2 % 8;
}

// The explicit stack of np_pairwise_sum: the nodes on the path from the piece to the current leaf (8192 -> 128 halves
// 6 times, a ragged piece once more: at most 8 nodes).  The caller chooses where it lives (private or LDS).
template <typename T>
struct NpSumStack {
    static constexpr int depth = 8;
    int off[depth], n[depth];
    int state[depth];                      // 0: left half pending, 1: left half done (acc holds it)
    T acc[depth];
};

// numpy's pairwise sum of one piece, n <= 8192 terms, by one lane: an iterative post-order walk of the split tree
template <typename T, typename F>
APGPU_HD inline T np_pairwise_sum(int n, F f, NpSumStack<T> &st)
{
    int sp = 0;
    st.off[0] = 0; st.n[0] = n; st.state[0] = 0;
    T val = (T)0;
    bool have = false;
    while (true) {
        if (!have) {
            const int off = st.off[sp], cnt = st.n[sp];
            if (cnt <= 128) {
                val = np_leaf_sum<T>(cnt, [&](long long i) { return f(off + i); });
                have = true;
            } else {
                const int n2 = np_left_half(cnt);
                st.state[sp] = 0;
                st.off[sp + 1] = off; st.n[sp + 1] = n2; st.state[sp + 1] = 0;      // descend into the left half
                sp++;
                continue;
            }
        }
        // `val` is the sum of node sp: hand it to its parent
        if (sp == 0) break;
        const int par = sp - 1;
        if (st.state[par] == 0) {
            st.acc[par] = val;
            st.state[par] = 1;
            const int n2 = np_left_half(st.n[par]);
            st.off[sp] = st.off[par] + n2; st.n[sp] = st.n[par] - n2; st.state[sp] = 0;
            have = false;                  // now the right half
        } else {
            val = st.acc[par] + val;
            sp = par;                      // node par is complete
        }
    }
    return val;
}

// np.add.reduce of n terms: 8192-element pieces folded in order from 0 (so an empty sum, and a sum of -0s, is +0)
template <typename T, typename F>
APGPU_HD inline T np_add_reduce(long long n, F f, NpSumStack<T> &st)
{
    T total = (T)0;
    for (long long p0 = 0; p0 < n; p0 += 8192) {
        const int pn = (n - p0) < 8192 ? (int)(n - p0) : 8192;
        total = total + np_pairwise_sum<T>(pn, [&](long long i) { return f(p0 + i); }, st);
    }
    return total;
}

#if defined(__HIP__)
// the sum of x over the 64 lanes of a wavefront, the same value in every lane
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
#endif

}  // namespace apgpu
