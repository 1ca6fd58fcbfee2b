// Development aid / CPU test helper (tests/test_select_network_host.py): proves the 64-slot selection network of stack_sort.h
// (kSelect64: 8 rows, 8 columns, kSelect8x8Ops) and prints its instruction count.  The proof composes:
//   1. kSort8Ops sorts 8 values: all 2^8 0-1 inputs (0-1 principle);
//   2. stage 0 of the table is that sorter on the 8 rows of the 8 x 8 matrix (wire = 8 row + column), stage 1 on its 8 columns:
//      compared op for op; sorting the columns of a matrix with sorted rows leaves the rows sorted, so a 0-1 input is then a
//      staircase matrix - C(16, 8) = 12870 of them;
//   3. stage 2 (the searched post-phase) on every staircase: the needed wires 0..4, 29..34, 59..63 carry their ranks, wires 4..28
//      hold nothing above what wires 35..59 hold, nothing is lost; every sorter of every stage lists its wires ascending
//      (standard form: an ascending column passes through unchanged - also checked directly).
// Then 10^5 random float columns through the whole table against std::sort: needed wires bit-equal, the column a permutation of
// its input, the sides of the core apart - ties across the median window, +-0.0, all values equal, +-inf; and a NaN at each of
// the 64 positions must come out on wire 63 when the maxima propagate NaNs (sort_column's NANMAX).
// The float model of the instructions: minima / maxima / medians under the total order -0.0 < +0.0 (what v_min_f32 / v_max_f32
// do); with a NaN operand v_min_f32 and v_min3_f32 return the other operands' minimum, v_med3_f32 returns the minimum of the three,
// v_maximum3_f32 returns NaN.
//   hipcc -O2 -std=c++17 -I include -I astrophotography_amd/csrc tools/netsearch/verify_select64.cpp -o /tmp/verify_select64
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "stack_sort.h"

using namespace apgpu_stack;

// what clip_fast32 reads in rank order: the tails, the first value behind either tail (would a fifth one go?), the median window
static bool needed(int i) { return i <= 4 || i >= 59 || (i >= 29 && i <= 34); }

static uint64_t apply01(uint64_t v, const NetOp &o)
{
    int ones = 0;
    uint64_t mask = 0;
    for (int i = 0; i < o.k; i++) {
        ones += (int)((v >> o.w[i]) & 1);
        mask |= 1ull << o.w[i];
    }
    v &= ~mask;
    for (int i = o.k - ones; i < o.k; i++) v |= 1ull << o.w[i];
    return v;
}

static uint32_t bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

// total order on non-NaN floats: by value, -0.0 below +0.0
static bool below(float a, float b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); }

static void applyf(float *v, const NetOp &o)
{
    float x[4], nn[4];
    int n = 0;
    bool nan = false;
    for (int i = 0; i < o.k; i++) {
        x[i] = v[o.w[i]];
        if (std::isnan(x[i])) nan = true;
        else nn[n++] = x[i];
    }
    if (!nan) {
        std::sort(x, x + o.k, below);
        for (int i = 0; i < o.k; i++) v[o.w[i]] = x[i];
        return;
    }
    // a NaN among the operands: every minimum / median gives the minimum of the others, every maximum the NaN (sort4: the
    // instruction sequence of stack_sort.h, whose later steps read earlier results - all below the top wire, which is all that is
    // checked for these columns)
    const float lo = n ? *std::min_element(nn, nn + n, below) : std::nanf("");
    for (int i = 0; i + 1 < o.k; i++) v[o.w[i]] = lo;
    v[o.w[o.k - 1]] = std::nanf("");
}

int main()
{
    bool ok = true;
    const OpNet<64> &net = kSelect64;
    int instr[3] = {0, 0, 0}, cnt[5] = {0, 0, 0, 0, 0};
    for (int c = 0; c < net.n; c++) {
        const NetOp &o = net.op[c];
        instr[o.stage] += o.k == 4 ? 7 : o.k;
        cnt[o.k]++;
        for (int i = 0; i + 1 < o.k; i++)
            if (!(o.w[i] < o.w[i + 1]) || o.w[i + 1] >= 64) { printf("op %d: wires not ascending\n", c); ok = false; }
        if (c > 0 && o.stage < net.op[c - 1].stage) { printf("op %d: stages out of order\n", c); ok = false; }
    }
    // 1. the 8-sorter
    for (uint32_t xin = 0; xin < 256; xin++) {
        uint64_t v = xin;
        for (const NetOp &o : kSort8Ops) v = apply01(v, o);
        const int ones = __builtin_popcount(xin);
        if (v != ((0xffull >> (8 - ones)) << (8 - ones))) { printf("8-sorter fails on %02x\n", xin); ok = false; }
    }
    // 2. rows, then columns
    {
        int c = 0;
        for (int r = 0; r < 8; r++)
            for (const NetOp &o : kSort8Ops) {
                const NetOp &g = net.op[c++];
                for (int i = 0; i < 3; i++)
                    if (g.stage != 0 || g.k != 3 || g.w[i] != 8 * r + o.w[i]) ok = false;
            }
        for (int col = 0; col < 8; col++)
            for (const NetOp &o : kSort8Ops) {
                const NetOp &g = net.op[c++];
                for (int i = 0; i < 3; i++)
                    if (g.stage != 1 || g.k != 3 || g.w[i] != 8 * o.w[i] + col) ok = false;
            }
        for (; c < net.n; c++)
            if (net.op[c].stage != 2) ok = false;
        if (!ok) printf("pre-phase is not rows + columns of kSort8Ops\n");
    }
    // 3. the post-phase on every staircase (zeros per row non-increasing down the rows; zeros first in a row)
    long cases = 0;
    {
        int z[8] = {8, 8, 8, 8, 8, 8, 8, 8};
        for (;;) {
            bool stair = true;
            for (int r = 0; r + 1 < 8; r++) stair = stair && z[r] >= z[r + 1];
            if (stair) {
                uint64_t v = 0;
                int zeros = 0;
                for (int r = 0; r < 8; r++) {
                    zeros += z[r];
                    for (int col = z[r]; col < 8; col++) v |= 1ull << (8 * r + col);
                }
                for (int c = 0; c < net.n; c++)
                    if (net.op[c].stage == 2) v = apply01(v, net.op[c]);
                cases++;
                bool good = __builtin_popcountll(v) == 64 - zeros;
                int low_max = 0, high_min = 1;
                for (int i = 0; i < 64; i++) {
                    const int b = (int)((v >> i) & 1);
                    if (needed(i) && b != (i >= zeros)) good = false;
                    if (i >= 4 && i <= 28) low_max = std::max(low_max, b);
                    if (i >= 35 && i <= 59) high_min = std::min(high_min, b);
                }
                if (low_max > high_min) good = false;
                if (!good) {
                    if (ok) printf("post-phase fails on the staircase %d %d %d %d %d %d %d %d\n", z[0], z[1], z[2], z[3], z[4], z[5], z[6], z[7]);
                    ok = false;
                }
            }
            int k = 7;
            while (k >= 0 && z[k] == 0) z[k--] = 8;
            if (k < 0) break;
            z[k]--;
        }
        if (cases != 12870) { printf("%ld staircases?\n", cases); ok = false; }
    }
    // random float columns
    std::mt19937 rng(20240817);
    std::normal_distribution<float> normal(1000.f, 30.f);
    const float inf = std::numeric_limits<float>::infinity();
    long columns = 0, nan_columns = 0;
    for (int n = 0; n < 100000; n++) {
        float x[64], v[64], s[64];
        const int kind = n % 10;
        for (int i = 0; i < 64; i++) {
            switch (kind) {
            case 0: case 1: case 2: x[i] = normal(rng); break;
            case 3: x[i] = (float)(500 + (int)(rng() % 3)); break;                    // ties across the median window
            case 4: x[i] = (float)(int)(rng() % 40); break;
            case 5: x[i] = (rng() & 1) ? 0.f : -0.f; break;                          // +-0.0 only
            case 6: x[i] = (rng() % 3 == 0) ? ((rng() & 1) ? 0.f : -0.f) : (float)((int)(rng() % 5) - 2); break;
            case 7: x[i] = 777.25f; break;                                           // equal throughout
            case 8: x[i] = (rng() % 8 == 0) ? ((rng() & 1) ? inf : -inf) : normal(rng); break;
            default: x[i] = normal(rng); break;                                      // 9: a NaN below
            }
        }
        if (kind == 0) std::sort(x, x + 64);                                         // ascending columns pass through unchanged
        if (kind == 9) x[(n / 10) % 64] = std::nanf("");
        memcpy(v, x, sizeof v);
        for (int c = 0; c < net.n; c++) applyf(v, net.op[c]);
        if (kind == 9) {
            nan_columns++;
            if (!std::isnan(v[63])) { if (ok) printf("column %d: the NaN at %d did not reach wire 63\n", n, (n / 10) % 64); ok = false; }
            continue;
        }
        columns++;
        memcpy(s, x, sizeof s);
        std::sort(s, s + 64, below);
        bool good = true;
        for (int i = 0; i < 64; i++)
            if (needed(i) && bits(v[i]) != bits(s[i])) good = false;
        if (kind == 0 && memcmp(v, x, sizeof v) != 0) good = false;
        for (int i = 4; i <= 28; i++)
            for (int j = 35; j <= 59; j++)
                if (below(v[j], v[i])) good = false;
        float w[64];
        memcpy(w, v, sizeof w);
        std::sort(w, w + 64, below);
        if (memcmp(w, s, sizeof w) != 0) good = false;                               // a permutation of the input
        if (!good) { if (ok) printf("column %d (kind %d) fails\n", n, kind); ok = false; }
    }
    printf("select64: %d instructions (rows %d + columns %d + post-phase %d; %d 2-sorters, %d 3-sorters, %d 4-sorters), %ld staircases, "
           "%ld float columns, %ld NaN columns: %s\n", instr[0] + instr[1] + instr[2], instr[0], instr[1], instr[2], cnt[2], cnt[3], cnt[4], cases,
           columns, nan_columns, ok ? "ok" : "FAILED");
    printf(ok ? "ALL OK\n" : "FAILURES\n");
    return ok ? 0 : 1;
}
