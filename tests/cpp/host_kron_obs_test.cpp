// host_kron_obs_test.cpp -- the host set-up of the Kronecker-sum handle's factored data term (fdapde-core_amd/csrc/host_kron_obs.cpp, with host_obs.cpp) on
// its own, no device:
//   * kron_obs_validate refuses each malformed input fdapde_kron_set_obs names (p out of range, Phi == NULL with p > q, a non-finite entry of Phi, weight or
//     scale, and what obs_validate refuses of Psi), names itself in the message, and takes the well-formed input;
//   * kron_obs_weights: the (instant, location) weights into the per-observation interleaved order; kron_obs_phi: NULL -> [I_p 0]; the team width and the form rule;
//   * kron_obs_merge_dense: the merged q n-row CSR against a dense A + scale B^T W B, B = Phi (x) Psi, on a 5 x 5 grid (5-point pattern, q = 3, p = 2, random
//     expanded values in the stacked order), for a Psi with an empty row, a one-entry row and a row over every DOF, for one where a DOF is in no row, and with
//     Phi = NULL; a pair (r, s) whose Phi columns never meet gets no entry off the pattern.
// Every value is a small multiple of 1/8, every weight a power of two or zero: all sums are exact in any order, the comparisons are ==.
// Compiled and run by tests/test_host_kron_obs.py (g++ -std=c++20), a second time with -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../fdapde-core_amd/csrc/host_kron_obs.h"

using namespace fdapde_hip;

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                     \
    do {                                                                                                      \
        ++checks;                                                                                             \
        if (!(cond)) { ++failures; std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); }          \
    } while (0)

static uint32_t lcg_state = 2468u;
static int lcg(int lo, int hi) {   // integers in [lo, hi]
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lo + (int)((lcg_state >> 8) % (uint32_t)(hi - lo + 1));
}
static double eighths() { return lcg(1, 24) / 8.0 * (lcg(0, 1) ? 1 : -1); }

struct Csr {
    std::vector<int64_t> rp {0};
    std::vector<int32_t> ci;
    std::vector<double> v;
    void row(const std::vector<int32_t>& cols) {
        for (int32_t c : cols) ci.push_back(c), v.push_back(eighths());
        rp.push_back((int64_t)ci.size());
    }
    int64_t rows() const { return (int64_t)rp.size() - 1; }
};

static bool valid(int64_t n, int q, int p, const double* Phi, const Csr& P, const double* w, double scale, std::string* why = nullptr) {
    return kron_obs_validate(n, q, p, Phi, P.rows(), P.rp.data(), P.ci.data(), P.v.data(), w, scale, why);
}

// the expanded matrix of a Kronecker sum on the 5-point pattern of an nx x nx grid: q n rows in the stacked order r n + i, columns s n + j ascending
struct Expanded {
    int64_t n = 0;
    int q = 0;
    std::vector<int32_t> rp, ci;
    std::vector<double> v;
};
static Expanded grid_system(int nx, int q) {
    Expanded E;
    E.n = (int64_t)nx * nx, E.q = q;
    E.rp.push_back(0);
    for (int r = 0; r < q; ++r)
        for (int64_t i = 0; i < E.n; ++i) {
            const int ix = (int)(i % nx), iy = (int)(i / nx);
            for (int s = 0; s < q; ++s) {
                std::vector<int32_t> cols;
                if (iy > 0) cols.push_back((int32_t)(i - nx));
                if (ix > 0) cols.push_back((int32_t)(i - 1));
                cols.push_back((int32_t)i);
                if (ix < nx - 1) cols.push_back((int32_t)(i + 1));
                if (iy < nx - 1) cols.push_back((int32_t)(i + nx));
                for (int32_t j : cols) E.ci.push_back((int32_t)(s * E.n + j)), E.v.push_back(eighths());
            }
            E.rp.push_back((int32_t)E.ci.size());
        }
    return E;
}

static void check_merge(const char* what, const Expanded& E, const std::vector<int32_t>& e2i, const Csr& P, int p, const double* Phi, const std::vector<double>& weights,
                        double scale, bool expect_dead_pair) {
    const int64_t n = E.n, m = P.rows(), nq = E.q * n;
    const int q = E.q;
    ObsHost H;
    obs_build(n, m, P.rp.data(), P.ci.data(), P.v.data(), nullptr, e2i.data(), &H);
    std::vector<double> phi, w;
    kron_obs_phi(q, p, Phi, &phi);
    kron_obs_weights(p, m, weights.empty() ? nullptr : weights.data(), &w);
    std::vector<double> psi((size_t)(m * n), 0.0);   // Psi in the internal order, dense
    for (int64_t k = 0; k < m; ++k)
        for (int64_t e = P.rp[k]; e < P.rp[k + 1]; ++e) psi[(size_t)(k * n + e2i[P.ci[e]])] = P.v[e];
    std::vector<double> ref((size_t)(nq * nq), 0.0);
    std::vector<uint8_t> on_pattern((size_t)(nq * nq), 0);
    for (int64_t row = 0; row < nq; ++row)
        for (int32_t e = E.rp[row]; e < E.rp[row + 1]; ++e) ref[(size_t)(row * nq + E.ci[e])] += E.v[e], on_pattern[(size_t)(row * nq + E.ci[e])] = 1;
    for (int r = 0; r < q; ++r)
        for (int s = 0; s < q; ++s)
            for (int tau = 0; tau < p; ++tau) {
                const double f = phi[tau + (size_t)r * p] * phi[tau + (size_t)s * p];
                if (f == 0.0) continue;
                for (int64_t k = 0; k < m; ++k) {
                    const double wk = weights.empty() ? 1.0 : weights[(size_t)tau * m + k];
                    for (int64_t i = 0; i < n; ++i)
                        for (int64_t j = 0; j < n; ++j) ref[(size_t)((r * n + i) * nq + s * n + j)] += scale * f * wk * psi[(size_t)(k * n + i)] * psi[(size_t)(k * n + j)];
                }
            }
    std::vector<int32_t> rp2, ci2;
    std::vector<double> v2;
    kron_obs_merge_dense(q, E.rp.data(), E.ci.data(), E.v.data(), H, p, phi.data(), w.data(), scale, &rp2, &ci2, &v2);
    EXPECT_TRUE((int64_t)rp2.size() == nq + 1 && rp2[0] == 0 && rp2[(size_t)nq] == (int32_t)ci2.size() && ci2.size() == v2.size());
    bool sorted = true, equal = true, pattern_kept = true;
    int64_t off_pattern = 0, dead_inserted = 0;
    std::vector<double> got((size_t)(nq * nq), 0.0);
    std::vector<uint8_t> stored((size_t)(nq * nq), 0);
    for (int64_t row = 0; row < nq; ++row)
        for (int32_t e = rp2[(size_t)row]; e < rp2[(size_t)row + 1]; ++e) {
            if (e > rp2[(size_t)row] && ci2[(size_t)e] <= ci2[(size_t)e - 1]) sorted = false;
            if (ci2[(size_t)e] < 0 || ci2[(size_t)e] >= nq) {
                sorted = false;
                continue;
            }
            got[(size_t)(row * nq + ci2[(size_t)e])] = v2[(size_t)e], stored[(size_t)(row * nq + ci2[(size_t)e])] = 1;
            if (!on_pattern[(size_t)(row * nq + ci2[(size_t)e])]) {
                ++off_pattern;
                const int r = (int)(row / n), s = (int)(ci2[(size_t)e] / n);
                bool live = false;
                for (int tau = 0; tau < p; ++tau) live = live || phi[tau + (size_t)r * p] * phi[tau + (size_t)s * p] != 0.0;
                if (!live) ++dead_inserted;
            }
        }
    for (size_t t = 0; t < ref.size(); ++t) {
        if (got[t] != ref[t]) equal = false;
        if (on_pattern[t] && !stored[t]) pattern_kept = false;
    }
    EXPECT_TRUE(sorted);
    EXPECT_TRUE(equal);
    EXPECT_TRUE(pattern_kept);
    EXPECT_TRUE(dead_inserted == 0);
    if (expect_dead_pair) EXPECT_TRUE(off_pattern > 0);
    std::printf("%s: %lld x %lld, %zu entries (%lld off the pattern)\n", what, (long long)nq, (long long)nq, ci2.size(), (long long)off_pattern);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int nx = 5, q = 3, p = 2;
    const int64_t n = nx * nx;
    {   // validation
        Csr P;
        P.row({0, 3, 7}), P.row({}), P.row({24});
        std::vector<double> Phi((size_t)p * q, 0.5), w((size_t)p * 3, 1.0);
        std::string why;
        EXPECT_TRUE(valid(n, q, p, Phi.data(), P, w.data(), -1.0));
        EXPECT_TRUE(valid(n, q, p, nullptr, P, nullptr, 2.0));                 // Phi = NULL with p <= q, no weights
        EXPECT_TRUE(valid(n, q, q, nullptr, P, nullptr, 2.0));
        EXPECT_TRUE(!valid(n, q, 0, Phi.data(), P, nullptr, -1.0, &why) && why.find("fdapde_kron_set_obs") == 0);
        EXPECT_TRUE(!valid(n, q, 65, nullptr, P, nullptr, -1.0));
        EXPECT_TRUE(!valid(n, q, q + 1, nullptr, P, nullptr, -1.0, &why) && why.find("p <= q") != std::string::npos);
        std::vector<double> Phi4((size_t)(q + 1) * q, 0.25);
        EXPECT_TRUE(valid(n, q, q + 1, Phi4.data(), P, nullptr, -1.0));        // p > q with an explicit Phi is fine
        std::vector<double> bad = Phi;
        bad[4] = nan;
        EXPECT_TRUE(!valid(n, q, p, bad.data(), P, nullptr, -1.0, &why) && why.find("Phi") != std::string::npos);
        bad = Phi, bad[0] = inf;
        EXPECT_TRUE(!valid(n, q, p, bad.data(), P, nullptr, -1.0));
        std::vector<double> wb = w;
        wb[5] = inf;                                                           // (the last of the p n_obs weights: beyond the first n_obs)
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), P, wb.data(), -1.0, &why) && why.find("weight 5") != std::string::npos);
        wb = w, wb[0] = nan;
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), P, wb.data(), -1.0));
        wb = w, wb[2] = 0.0;                                                   // an exact zero is a missing observation, not an error
        EXPECT_TRUE(valid(n, q, p, Phi.data(), P, wb.data(), -1.0));
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), P, nullptr, nan));
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), P, nullptr, inf));
        Csr B = P;
        B.ci[1] = (int32_t)n;
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), B, nullptr, -1.0, &why) && why.find("fdapde_kron_set_obs") == 0 && why.find("fdapde_block") == std::string::npos);
        B = P, B.ci[1] = -1;
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), B, nullptr, -1.0));
        B = P, std::swap(B.ci[0], B.ci[1]);
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), B, nullptr, -1.0));
        B = P, B.ci[1] = B.ci[0];
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), B, nullptr, -1.0));
        B = P, B.rp[2] = B.rp[1] - 1;
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), B, nullptr, -1.0));
        B = P, B.rp[0] = 1;
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), B, nullptr, -1.0));
        B = P, B.v[2] = nan;
        EXPECT_TRUE(!valid(n, q, p, Phi.data(), B, nullptr, -1.0));
    }
    {   // the weights' transposition, Phi = NULL, widths and forms
        std::vector<double> w {1, 2, 3, 4, 5, 6}, out;   // p = 2 instants x 3 locations, instant-major
        kron_obs_weights(2, 3, w.data(), &out);
        EXPECT_TRUE((out == std::vector<double> {1, 4, 2, 5, 3, 6}));
        kron_obs_weights(2, 3, nullptr, &out);
        EXPECT_TRUE((out == std::vector<double>(6, 1.0)));
        std::vector<double> phi;
        kron_obs_phi(3, 2, nullptr, &phi);
        EXPECT_TRUE((phi == std::vector<double> {1, 0, 0, 1, 0, 0}));   // column-major 2 x 3
        const double given[6] = {1, 2, 3, 4, 5, 6};
        kron_obs_phi(3, 2, given, &phi);
        EXPECT_TRUE((phi == std::vector<double>(given, given + 6)));
        EXPECT_TRUE(kron_obs_team_width(1, 1) == 2 && kron_obs_team_width(2, 1) == 2 && kron_obs_team_width(3, 5) == 8 && kron_obs_team_width(6, 4) == 8);
        EXPECT_TRUE(kron_obs_team_width(10, 7) == 16 && kron_obs_team_width(16, 16) == 16 && kron_obs_team_width(33, 40) == 64 && kron_obs_team_width(4, 64) == 64);
        EXPECT_TRUE(kron_obs_form(10, 160, 0) == 1 && kron_obs_form(10, 161, 0) == 2 && kron_obs_form(10, 1000, 1) == 1 && kron_obs_form(10, 1, 2) == 2);
    }
    // the merged matrix
    const Expanded E = grid_system(nx, q);
    std::vector<int32_t> e2i((size_t)n), all((size_t)n);
    for (int64_t i = 0; i < n; ++i) e2i[(size_t)i] = (int32_t)((i * 7 + 3) % n), all[(size_t)i] = (int32_t)i;   // a non-trivial numbering
    {
        Csr P;   // an empty row, a one-entry row, a row over every DOF, a short row
        P.row({}), P.row({12}), P.row(all), P.row({1, 2, 20});
        std::vector<double> Phi {0.5, -1.0, 0.25, 2.0, 0.0, 0.0};   // 2 x 3 column-major: the third column is zero -- no entry in block row or column 2
        std::vector<double> w {1.0, 0.5, 2.0, 0.0, 4.0, 1.0, 0.0, 0.25};
        check_merge("empty, single, full and short rows", E, e2i, P, p, Phi.data(), w, -1.0, true);
        check_merge("... without weights, scale 0.5", E, e2i, P, p, Phi.data(), {}, 0.5, true);
    }
    {
        Csr P;   // DOF 24 (reference numbering) in no row
        P.row({0, 1, 5, 6}), P.row({6, 7, 11, 12, 13}), P.row({3}), P.row({18, 19, 23});
        std::vector<double> Phi {1.0, 0.5, -0.5, 1.5, 0.125, -2.0};
        std::vector<double> w {1, 1, 0, 2, 0.5, 0, 1, 1};
        check_merge("a DOF in no row, dense Phi", E, e2i, P, p, Phi.data(), w, -1.0, true);
        check_merge("... with Phi = NULL", E, e2i, P, p, nullptr, w, -1.0, true);
    }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
