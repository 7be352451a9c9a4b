// host_obs_test.cpp -- the host set-up of the 2 x 2 block handle's factored data term (fdapde-core_amd/csrc/host_obs.cpp) on its own, no device:
//   * obs_validate refuses each malformed input fdapde_block_set_obs names, and takes the well-formed one;
//   * obs_build: Psi in the internal order (columns through a non-trivial dof_e2i, rows sorted again) and Psi^T (observations ascending) against dense;
//   * obs_merge_dense: the 2 n-row CSR against a dense A + scale Psi^T W Psi on a 5 x 5 grid (5-point pattern, four random blocks), for a Psi with an empty
//     row, a one-entry row and a row covering every DOF, and for one where a DOF is in no row.
// Every value is a small multiple of 1/8, every weight a power of two: all sums are exact in any order, the comparisons are ==.
// Compiled and run by tests/test_host_obs.py (g++ -std=c++20; add -fsanitize=address,undefined for a sanitizer run of this program).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../fdapde-core_amd/csrc/host_obs.h"

using namespace fdapde_hip;

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                     \
    do {                                                                                                      \
        ++checks;                                                                                             \
        if (!(cond)) { ++failures; std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); }          \
    } while (0)

static uint32_t lcg_state = 12345u;
static int lcg(int lo, int hi) {   // integers in [lo, hi]
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lo + (int)((lcg_state >> 8) % (uint32_t)(hi - lo + 1));
}

struct Csr {
    std::vector<int64_t> rp {0};
    std::vector<int32_t> ci;
    std::vector<double> v;
    void row(const std::vector<int32_t>& cols) {
        for (int32_t c : cols) ci.push_back(c), v.push_back(lcg(1, 24) / 8.0 * (lcg(0, 1) ? 1 : -1));
        rp.push_back((int64_t)ci.size());
    }
    int64_t rows() const { return (int64_t)rp.size() - 1; }
};

static bool valid(int64_t n, const Csr& P, const double* w, double scale, std::string* why = nullptr) {
    return obs_validate(n, P.rows(), P.rp.data(), P.ci.data(), P.v.data(), w, scale, why);
}

static void check_case(const char* what, int64_t n, const std::vector<int32_t>& rowptr, const std::vector<int32_t>& colidx, const std::vector<double>& raw,
                       const std::vector<int32_t>& e2i, const Csr& P, const std::vector<double>& w, double scale) {
    const int64_t m = P.rows();
    ObsHost H;
    obs_build(n, m, P.rp.data(), P.ci.data(), P.v.data(), w.empty() ? nullptr : w.data(), e2i.data(), &H);
    std::vector<double> dense((size_t)(m * n), 0.0);   // Psi in the internal order
    for (int64_t k = 0; k < m; ++k)
        for (int64_t e = P.rp[k]; e < P.rp[k + 1]; ++e) dense[(size_t)(k * n + e2i[P.ci[e]])] = P.v[e];
    EXPECT_TRUE(H.n_obs == m && H.n == n && H.nnz == P.rp[m] && (int64_t)H.w.size() == m);
    bool psi_ok = true, t_ok = true;
    int32_t longest_row = 0, longest_col = 0;
    std::vector<double> back((size_t)(m * n), 0.0), tback((size_t)(m * n), 0.0);
    for (int64_t k = 0; k < m; ++k) {
        longest_row = std::max(longest_row, H.rp[k + 1] - H.rp[k]);
        for (int32_t e = H.rp[k]; e < H.rp[k + 1]; ++e) {
            if (e > H.rp[k] && H.ci[e] <= H.ci[e - 1]) psi_ok = false;
            back[(size_t)(k * n + H.ci[e])] = H.v[e];
        }
    }
    for (int64_t i = 0; i < n; ++i) {
        longest_col = std::max(longest_col, H.trp[i + 1] - H.trp[i]);
        for (int32_t s = H.trp[i]; s < H.trp[i + 1]; ++s) {
            if (s > H.trp[i] && H.tci[s] <= H.tci[s - 1]) t_ok = false;
            tback[(size_t)(H.tci[s] * n + i)] = H.tv[s];
        }
    }
    EXPECT_TRUE(psi_ok && back == dense);
    EXPECT_TRUE(t_ok && tback == dense && H.trp[n] == H.nnz);
    EXPECT_TRUE(H.longest_row == longest_row && H.longest_col == longest_col);
    for (int64_t k = 0; k < m; ++k) EXPECT_TRUE(H.w[k] == (w.empty() ? 1.0 : w[k]));

    // A + scale Psi^T W Psi, dense, interleaved order
    const int64_t n2 = 2 * n;
    std::vector<double> full((size_t)(n2 * n2), 0.0);
    for (int64_t i = 0; i < n; ++i)
        for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
            for (int p = 0; p < 2; ++p)
                for (int q = 0; q < 2; ++q) full[(size_t)((2 * i + p) * n2 + 2 * colidx[k] + q)] = raw[(size_t)(4 * k + 2 * p + q)];
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j) {
            double g = 0;
            for (int64_t k = 0; k < m; ++k) g += (H.w[k] * dense[(size_t)(k * n + i)]) * dense[(size_t)(k * n + j)];
            full[(size_t)(2 * i * n2 + 2 * j)] += scale * g;
        }
    std::vector<int32_t> rp2, ci2;
    std::vector<double> v2;
    obs_merge_dense(rowptr.data(), colidx.data(), raw.data(), H, scale, &rp2, &ci2, &v2);
    EXPECT_TRUE((int64_t)rp2.size() == n2 + 1 && rp2[0] == 0 && rp2[n2] == (int32_t)ci2.size() && ci2.size() == v2.size());
    bool sorted = true, in_range = true;
    std::vector<double> merged((size_t)(n2 * n2), 0.0);
    for (int64_t r = 0; r < n2; ++r)
        for (int32_t e = rp2[r]; e < rp2[r + 1]; ++e) {
            if (e > rp2[r] && ci2[e] <= ci2[e - 1]) sorted = false;
            if (ci2[e] < 0 || ci2[e] >= n2) { in_range = false; continue; }
            merged[(size_t)(r * n2 + ci2[e])] = v2[e];
        }
    EXPECT_TRUE(sorted && in_range);
    EXPECT_TRUE(merged == full);
    int64_t off = 0;   // entries the term put off the pattern
    for (int64_t r = 0; r < n2; r += 2) off += (rp2[r + 1] - rp2[r]) - 2 * (rowptr[r / 2 + 1] - rowptr[r / 2]);
    std::printf("  %s: n_obs %lld, nnz(Psi) %lld, longest row %d / column %d, merged entries %zu (%lld off the pattern)\n", what, (long long)m, (long long)H.nnz,
                H.longest_row, H.longest_col, ci2.size(), (long long)off);
}

int main() {
    // the 5-point pattern of a 5 x 5 grid, four random blocks per entry
    const int g = 5;
    const int64_t n = g * g;
    std::vector<int32_t> rowptr {0}, colidx;
    for (int i = 0; i < g; ++i)
        for (int j = 0; j < g; ++j) {
            if (i > 0) colidx.push_back((i - 1) * g + j);
            if (j > 0) colidx.push_back(i * g + j - 1);
            colidx.push_back(i * g + j);
            if (j + 1 < g) colidx.push_back(i * g + j + 1);
            if (i + 1 < g) colidx.push_back((i + 1) * g + j);
            rowptr.push_back((int32_t)colidx.size());
        }
    std::vector<double> raw(4 * colidx.size());
    for (double& v : raw) v = lcg(-16, 16) / 8.0;
    std::vector<int32_t> e2i((size_t)n);   // reference id -> internal id: 7 is a unit mod 25, a permutation that reverses the order of some neighbours
    for (int64_t i = 0; i < n; ++i) e2i[(size_t)i] = (int32_t)((7 * i + 3) % n);

    std::vector<int32_t> all, all_but_7;
    for (int32_t i = 0; i < n; ++i) {
        all.push_back(i);
        if (i != 7) all_but_7.push_back(i);
    }
    Csr A;   // an empty row, a one-entry row, a row covering every DOF, short rows
    A.row({}), A.row({11}), A.row(all), A.row({0, 1, 5}), A.row({3, 12, 24}), A.row({});
    Csr B;   // reference DOF 7 is in no row
    B.row({2, 8, 9}), B.row(all_but_7), B.row({}), B.row({6});
    const std::vector<double> wA {0.5, 2.0, 1.0, 4.0, 0.25, 2.0}, none;

    // ---- validation
    std::string why;
    EXPECT_TRUE(valid(n, A, nullptr, -1.0, &why) && valid(n, A, wA.data(), 0.375) && valid(n, B, nullptr, -1.0));
    {
        Csr P = A;
        P.ci[1] = (int32_t)n;   // a column outside [0, n_dofs)
        EXPECT_TRUE(!valid(n, P, nullptr, -1.0, &why) && why.find("outside") != std::string::npos);
        P.ci[1] = -1;
        EXPECT_TRUE(!valid(n, P, nullptr, -1.0));
    }
    {
        Csr P = A;   // rows not strictly ascending: a swap, a duplicate
        std::swap(P.ci[(size_t)P.rp[3]], P.ci[(size_t)P.rp[3] + 1]);
        EXPECT_TRUE(!valid(n, P, nullptr, -1.0, &why) && why.find("ascending") != std::string::npos);
        P = A, P.ci[(size_t)P.rp[3] + 1] = P.ci[(size_t)P.rp[3]];
        EXPECT_TRUE(!valid(n, P, nullptr, -1.0));
    }
    {
        Csr P = A;   // rowptr: decreasing, not starting at 0
        P.rp[2] = P.rp[1] - 1;
        EXPECT_TRUE(!valid(n, P, nullptr, -1.0, &why) && why.find("rowptr") != std::string::npos);
        P = A, P.rp[0] = 1;
        EXPECT_TRUE(!valid(n, P, nullptr, -1.0));
    }
    {
        Csr P = A;   // values, weights, scale that are not finite
        P.v[4] = std::numeric_limits<double>::quiet_NaN();
        EXPECT_TRUE(!valid(n, P, nullptr, -1.0));
        P.v[4] = std::numeric_limits<double>::infinity();
        EXPECT_TRUE(!valid(n, P, nullptr, -1.0));
        std::vector<double> w = wA;
        w[5] = std::numeric_limits<double>::quiet_NaN();
        EXPECT_TRUE(!valid(n, A, w.data(), -1.0, &why) && why.find("weight") != std::string::npos);
        EXPECT_TRUE(!valid(n, A, nullptr, std::numeric_limits<double>::infinity(), &why) && why.find("scale") != std::string::npos);
        EXPECT_TRUE(!valid(n, A, nullptr, std::numeric_limits<double>::quiet_NaN()));
    }

    // ---- the rule of the team width
    EXPECT_TRUE(obs_team_width(10, 160, 0) == 8 && obs_team_width(10, 161, 0) == 64 && obs_team_width(10, 1000, 8) == 8 && obs_team_width(10, 10, 64) == 64);

    // ---- Psi, Psi^T, the merged matrix
    check_case("Psi with a full row, W = I, scale -1", n, rowptr, colidx, raw, e2i, A, none, -1.0);
    check_case("Psi with a full row, weights, scale 0.375", n, rowptr, colidx, raw, e2i, A, wA, 0.375);
    check_case("a DOF in no row, W = I, scale -1", n, rowptr, colidx, raw, e2i, B, none, -1.0);
    {
        ObsHost H;
        obs_build(n, B.rows(), B.rp.data(), B.ci.data(), B.v.data(), nullptr, e2i.data(), &H);
        EXPECT_TRUE(H.trp[e2i[7] + 1] == H.trp[e2i[7]]);   // its row of Psi^T is empty
    }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
