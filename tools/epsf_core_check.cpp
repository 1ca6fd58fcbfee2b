// Host check of csrc/epsf_core.h (F22), to be run under the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iastrophotography_amd/csrc tools/epsf_core_check.cpp -o epsf_core_check && ./epsf_core_check
//
// The gather form of the sample -> node rule (epsf_pixel_of) against the forward expression (epsf_node_of) for o = 1 .. 4,
// R = 2, 8, 32 and 20000 centres each, every seventh on a node boundary; the interpolant at its own nodes, outside the stamp and
// for NaN.  Exit status 0 if nothing disagrees.
#include "epsf_core.h"
#include <climits>
#include <cstdio>
#include <random>
#include <vector>
using namespace apgpu;
int main() {
    std::mt19937_64 rng(1);
    std::uniform_real_distribution<double> ux(-50.0, 5000.0);
    long bad = 0, found = 0, total = 0;
    for (int o = 1; o <= 4; ++o)
        for (int R : {2, 8, 32})
            for (int t = 0; t < 20000; ++t) {
                double x = ux(rng);
                if (t % 7 == 0) x = std::floor(x) + (t % 5) * 0.25;      // phases on the node boundaries
                // forward: every pixel near the star -> node; each node must be found by the gather with the same pixel
                std::vector<long long> fw(2 * o * R + 1, LLONG_MIN);
                std::vector<int> cnt(2 * o * R + 1, 0);
                for (long long p = (long long)std::floor(x) - R - 3; p <= (long long)std::floor(x) + R + 3; ++p) {
                    double k = epsf_node_of(p, x, o);
                    if (k >= -o * R && k <= o * R) { fw[(int)k + o * R] = p; cnt[(int)k + o * R]++; }
                }
                for (int k = -o * R; k <= o * R; ++k) {
                    long long p; bool ok = epsf_pixel_of(k, x, o, &p);
                    ++total;
                    if (cnt[k + o * R] > 1) { ++bad; continue; }
                    if (ok != (cnt[k + o * R] == 1) || (ok && p != fw[k + o * R])) ++bad;
                    found += ok;
                }
            }
    // interpolant: nodes reproduced, clamp safe at the edges
    int o = 3, R = 5, G = 2 * o * R + 1;
    std::vector<float> E(G * G);
    for (auto &v : E) v = (float)ux(rng);
    EpsfGrid g{E.data(), G, o, R};
    long ebad = 0;
    for (int j = 0; j < G; ++j)
        for (int i = 0; i < G; ++i) {
            double gx, gy;
            double v = epsf_eval<true>(g, (double)(i - o * R) / o, (double)(j - o * R) / o, &gx, &gy);
            if (v != (double)E[j * G + i]) ++ebad;
        }
    double gx, gy;
    if (epsf_eval<true>(g, R + 1e-9, 0, &gx, &gy) != 0.0 || epsf_eval<false>(g, NAN, 0, nullptr, nullptr) != 0.0) ++ebad;
    printf("gather: %ld nodes, %ld found, %ld disagree; interpolant: %ld bad\n", total, found, bad, ebad);
    return bad || ebad;
}
