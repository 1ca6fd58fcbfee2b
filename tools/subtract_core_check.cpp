// Host check of csrc/subtract_core.h (F23), to be run under the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iastrophotography_amd/csrc tools/subtract_core_check.cpp -o subtract_core_check && ./subtract_core_check
//
// The basis for the default and the largest configuration (64 functions, radius 15) and the smallest (one function, radius 1), into
// arrays of exactly the documented sizes: the counts, every filter index in range, the first function summing to 1 and every other
// to 0 within rounding, the odd functions antisymmetric; the polynomial terms against pow() and their count; the normalised
// coordinate at the ends of an axis and for an axis of one pixel.  Exit status 0 if nothing disagrees.
#include "subtract_core.h"
#include <cstdio>
#include <vector>
using namespace apgpu;
static long check_basis(int ng, const double *sig, const int32_t *deg, int r, int want)
{
    long bad = 0;
    const int kw = 2 * r + 1;
    if (subtract_basis_count(ng, deg) != want) return 1;
    std::vector<double> filters((size_t)kSubMaxBasis * kw), scale(kSubMaxBasis);
    std::vector<int32_t> row(kSubMaxBasis), col(kSubMaxBasis), even(kSubMaxBasis);
    int nf = 0;
    const int nb = subtract_basis_build(ng, sig, deg, r, filters.data(), row.data(), col.data(), scale.data(), even.data(), &nf);
    if (nb != want || nf < 1 || nf > nb) ++bad;
    for (int n = 0; n < nb; ++n) {
        if (row[n] < 0 || row[n] >= nf || col[n] < 0 || col[n] >= nf) { ++bad; continue; }
        double sum = 0.0, asum = 0.0;
        for (int v = -r; v <= r; ++v)
            for (int u = -r; u <= r; ++u) {
                const double b = subtract_basis_value(filters.data(), row.data(), col.data(), scale.data(), even.data(), r, n, u, v);
                sum += b;
                asum += std::fabs(b);
                if (!even[n]) {                                  // odd in u or in v: b(-u, -v) = +-b(u, v), and the sum vanishes
                    const double m = subtract_basis_value(filters.data(), row.data(), col.data(), scale.data(), even.data(), r, n, -u, -v);
                    if (std::fabs(std::fabs(m) - std::fabs(b)) > 1e-12 * (std::fabs(b) + 1e-300)) ++bad;
                }
            }
        if (std::fabs(sum - (n == 0 ? 1.0 : 0.0)) > 1e-12 * (asum + 1.0)) ++bad;
    }
    return bad;
}
int main()
{
    long bad = 0;
    const double s3[3] = {0.7, 1.5, 3.0};
    const int32_t d_def[3] = {6, 4, 2}, d_max[3] = {6, 5, 4}, d_over[3] = {6, 5, 5}, d_neg[1] = {-1}, d0[1] = {0};
    const double s1[1] = {1.0};
    bad += check_basis(3, s3, d_def, 10, 49);
    bad += check_basis(3, s3, d_max, 15, 64);
    bad += check_basis(1, s1, d0, 1, 1);
    if (subtract_basis_count(3, d_over) != -1 || subtract_basis_count(1, d_neg) != -1) ++bad;
    long pbad = 0;
    for (int d = 0; d <= kSubMaxDegree; ++d) {
        double out[kSubMaxTerms];
        const double X = -0.37, Y = 0.81;
        const int n = subtract_poly_terms(d, X, Y, out);
        if (n != subtract_poly_count(d) || n > kSubMaxTerms) ++pbad;
        int t = 0;
        for (int i = 0; i <= d; ++i)
            for (int j = 0; i + j <= d; ++j, ++t)
                if (std::fabs(out[t] - std::pow(X, i) * std::pow(Y, j)) > 1e-15) ++pbad;
    }
    if (subtract_norm_coord(0, 101) != -1.0 || subtract_norm_coord(100, 101) != 1.0 || subtract_norm_coord(50, 101) != 0.0 ||
        subtract_norm_coord(0, 1) != 0.0 || subtract_norm_coord((1LL << 40), (1LL << 41) + 1) != 0.0)
        ++pbad;
    printf("basis: %ld bad; polynomials: %ld bad\n", bad, pbad);
    return bad || pbad;
}
