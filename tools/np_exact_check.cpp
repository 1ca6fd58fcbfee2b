// Runs csrc/np_exact.h on the host for tests/test_host_cpu.py::test_np_exact_header_equals_numpy, which compares what this
// prints with NumPy itself.  Plain C++, no GPU:  np_exact_check <file>
//
// The file is a sequence of records: int32 kind ('S' sums, 'K' keys), int32 item size (4 float32, 8 float64), int64 n,
// float64 m, then n values.  Per record one line, every number the hex of its bits:
//   S <np_add_reduce(a)> <np_add_reduce((a - m)(a - m))> <np_add_reduce(a, NaN as 0)> <NaN count>
//   K <to(a[0])> <bits of from(to(a[0]))> <to(a[1])> ...
#include <cstdint>
#include <cstdio>
#include <vector>

#include "np_exact.h"

using namespace apgpu;

template <typename T>
static void record(int kind, const std::vector<T> &a, T m)
{
    using K = OrderKey<T>;
    const long long n = (long long)a.size();
    auto hex = [](T v) { return (unsigned long long)__builtin_bit_cast(typename K::U, v); };
    if (kind == 'K') {
        printf("K");
        for (long long i = 0; i < n; i++) printf(" %llx %llx", (unsigned long long)K::to(a[i]), hex(K::from(K::to(a[i]))));
        printf("\n");
        return;
    }
    NpSumStack<T> st;
    long long nans = 0;
    const T sum = np_add_reduce<T>(n, [&](long long i) { return a[i]; }, st);
    const T sq = np_add_reduce<T>(n, [&](long long i) { const T d = a[i] - m; return d * d; }, st);
    const T nansum = np_add_reduce<T>(n, [&](long long i) {
        if (a[i] != a[i]) { nans++; return (T)0; }
        return a[i];
    }, st);
    printf("S %llx %llx %llx %lld\n", hex(sum), hex(sq), hex(nansum), nans);
}

int main(int argc, char **argv)
{
    FILE *fh = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!fh) { fprintf(stderr, "usage: np_exact_check <file>\n"); return 2; }
    int32_t head[2];
    int64_t n;
    double m;
    while (fread(head, sizeof head, 1, fh) == 1) {
        if (fread(&n, sizeof n, 1, fh) != 1 || fread(&m, sizeof m, 1, fh) != 1 || n < 0) return 3;
        if (head[1] == 4) {
            std::vector<float> a((size_t)n);
            if (n && fread(a.data(), 4, (size_t)n, fh) != (size_t)n) return 3;
            record<float>(head[0], a, (float)m);
        } else if (head[1] == 8) {
            std::vector<double> a((size_t)n);
            if (n && fread(a.data(), 8, (size_t)n, fh) != (size_t)n) return 3;
            record<double>(head[0], a, m);
        } else {
            return 3;
        }
    }
    fclose(fh);
    return 0;
}
