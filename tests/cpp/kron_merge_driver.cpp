// kron_merge_driver.cpp -- stand-alone driver of the host side of fdapde_kron_compute (fdapde-core_amd/csrc/host_kron.cpp: terms that share a spatial
// factor are merged, their time factors summed, the band of every T-row found).  Plain C++ with its own main: meant to be built with
//     g++ -std=c++17 -g -fsanitize=address,undefined -I fdapde-core_amd/csrc tests/cpp/kron_merge_driver.cpp fdapde-core_amd/csrc/host_kron.cpp
// and run on the host; it touches no device.  Exit code 0 = every check held.
#include <cstdio>
#include <vector>

#include "host_kron.h"

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { ++failures; std::printf("FAILED %d: %s\n", __LINE__, #cond); } \
    } while (0)

int main() {
    using fdapde_hip::kron_merge_terms;
    for (int q : {1, 2, 3, 33, 64}) {
        const int K = 8;
        std::vector<std::vector<double>> T(K, std::vector<double>((size_t)q * q, 0.0));
        std::vector<double> sa(5, 1.0), sb(5, 2.0), sc(5, 3.0);
        // factors: a b a c b a c a -> three distinct ones in the order a, b, c
        const double* S[K] = {sa.data(), sb.data(), sa.data(), sc.data(), sb.data(), sa.data(), sc.data(), sa.data()};
        const double* Tp[K];
        for (int k = 0; k < K; ++k) {
            for (int r = 0; r < q; ++r)
                for (int s = 0; s < q; ++s)
                    if (s >= r - 1 && s <= r + 1 && r != q / 2) T[(size_t)k][(size_t)s * q + r] = (double)(k + 1) + 0.01 * (r * q + s);   // tridiagonal, row q / 2 all zero
            Tp[k] = T[(size_t)k].data();
        }
        std::vector<const double*> s_out(K);
        std::vector<double> tm((size_t)K * q * q, -7.0);
        std::vector<int32_t> band(2 * (size_t)q, -9);
        const int ns = kron_merge_terms(q, K, Tp, S, s_out.data(), tm.data(), band.data());
        CHECK(ns == 3 && s_out[0] == sa.data() && s_out[1] == sb.data() && s_out[2] == sc.data());
        const int members[3][4] = {{0, 2, 5, 7}, {1, 4, -1, -1}, {3, 6, -1, -1}};
        for (int sg = 0; sg < 3; ++sg)
            for (int e = 0; e < q * q; ++e) {
                double want = 0.0;
                bool first = true;
                for (int m = 0; m < 4; ++m)
                    if (members[sg][m] >= 0) want = first ? T[(size_t)members[sg][m]][(size_t)e] : want + T[(size_t)members[sg][m]][(size_t)e], first = false;
                CHECK(tm[(size_t)sg * q * q + e] == want);
            }
        for (int r = 0; r < q; ++r) {
            if (r == q / 2) CHECK(band[2 * r] == 0 && band[2 * r + 1] == -1);
            else CHECK(band[2 * r] == (r > 0 ? r - 1 : 0) && band[2 * r + 1] == (r + 1 < q ? r + 1 : q - 1));
        }
        // one term alone: copied, full band
        std::vector<double> full((size_t)q * q, 1.5);
        const double* one_t[1] = {full.data()};
        const double* one_s[1] = {sc.data()};
        CHECK(kron_merge_terms(q, 1, one_t, one_s, s_out.data(), tm.data(), band.data()) == 1 && s_out[0] == sc.data());
        for (int e = 0; e < q * q; ++e) CHECK(tm[(size_t)e] == 1.5);
        for (int r = 0; r < q; ++r) CHECK(band[2 * r] == 0 && band[2 * r + 1] == q - 1);
    }
    std::printf("%d failures\n", failures);
    return failures == 0 ? 0 : 1;
}
