// host_obs_coarsen_test.cpp -- obs_coarsen (fdapde-core_amd/csrc/host_obs.cpp) on its own, no device: the observation matrix of the next level of an
// aggregation hierarchy, Psi_c = Psi P with P piecewise constant, which FDAPDE_SOLVER_BLOCK_AMG carries beside its pattern levels (knob block_amg_obs).
//   * Psi_c and Psi_c^T against the dense Psi P: the same rows and weights, columns ascending, duplicates within a row summed, longest_row / longest_col;
//   * (Psi P)^T W (Psi P) == P^T (Psi^T W Psi) P: the Galerkin product of the term is the term of the coarsened Psi;
//   * the merged coarsest matrix: obs_merge_dense on the coarse pattern (the Galerkin product of the 5-point pattern) with Psi_c against the dense
//     P^T (A + scale [Psi^T W Psi, 0; 0, 0]) P, P = P_s (x) I_2;
//   * a second coarsening (Psi P_0 P_1) row for row.
// 5 x 5 grid; Psi has an empty row, a one-entry row, a row covering every DOF, a row whose entries all fall into one aggregate, and a DOF in no row; the
// aggregates have 1 - 4 members.  Every value is a small multiple of 1/8, every weight a power of two: all sums are exact in any order, the comparisons are ==.
// Compiled and run by tests/test_host_obs_coarsen.py (g++ -std=c++20; add -fsanitize=address,undefined for a sanitizer run of this program).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "../../fdapde-core_amd/csrc/host_obs.h"

using namespace fdapde_hip;

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                     \
    do {                                                                                                      \
        ++checks;                                                                                             \
        if (!(cond)) { ++failures; std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); }          \
    } while (0)

static uint32_t lcg_state = 2024u;
static int lcg(int lo, int hi) {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lo + (int)((lcg_state >> 8) % (uint32_t)(hi - lo + 1));
}

typedef std::vector<double> Dense;   // row-major

static Dense dense_of(const ObsHost& H) {
    Dense d((size_t)(H.n_obs * H.n), 0.0);
    for (int64_t k = 0; k < H.n_obs; ++k)
        for (int32_t e = H.rp[k]; e < H.rp[k + 1]; ++e) d[(size_t)(k * H.n + H.ci[e])] += H.v[e];
    return d;
}

// Psi_c against the dense Psi P, and its structure
static void check_coarse(const char* what, const ObsHost& F, const std::vector<int32_t>& agg, int64_t nc, const ObsHost& Cs) {
    const int64_t m = F.n_obs;
    const Dense fine = dense_of(F);
    Dense want((size_t)(m * nc), 0.0);
    for (int64_t k = 0; k < m; ++k)
        for (int64_t i = 0; i < F.n; ++i) want[(size_t)(k * nc + agg[(size_t)i])] += fine[(size_t)(k * F.n + i)];
    EXPECT_TRUE(Cs.n_obs == m && Cs.n == nc && Cs.w == F.w && (int64_t)Cs.rp.size() == m + 1 && (int64_t)Cs.trp.size() == nc + 1);
    EXPECT_TRUE(Cs.nnz == (int64_t)Cs.ci.size() && Cs.rp[m] == Cs.nnz && Cs.trp[nc] == Cs.nnz && Cs.v.size() == Cs.ci.size() && Cs.tv.size() == Cs.ci.size());
    bool asc = true, tasc = true;
    int32_t longest_row = 0, longest_col = 0;
    Dense back((size_t)(m * nc), 0.0), tback((size_t)(m * nc), 0.0);
    int64_t structural = 0;   // the coarse columns a row touches: an entry each, whatever the sum
    for (int64_t k = 0; k < m; ++k) {
        longest_row = std::max(longest_row, Cs.rp[k + 1] - Cs.rp[k]);
        for (int32_t e = Cs.rp[k]; e < Cs.rp[k + 1]; ++e) {
            if (e > Cs.rp[k] && Cs.ci[e] <= Cs.ci[e - 1]) asc = false;
            back[(size_t)(k * nc + Cs.ci[e])] = Cs.v[e];
        }
        std::vector<uint8_t> hit((size_t)nc, 0);
        for (int32_t e = F.rp[k]; e < F.rp[k + 1]; ++e) hit[(size_t)agg[(size_t)F.ci[e]]] = 1;
        structural += std::count(hit.begin(), hit.end(), 1);
        EXPECT_TRUE((F.rp[k + 1] == F.rp[k]) == (Cs.rp[k + 1] == Cs.rp[k]));   // an empty row stays empty, no other row becomes empty
    }
    for (int64_t i = 0; i < nc; ++i) {
        longest_col = std::max(longest_col, Cs.trp[i + 1] - Cs.trp[i]);
        for (int32_t s = Cs.trp[i]; s < Cs.trp[i + 1]; ++s) {
            if (s > Cs.trp[i] && Cs.tci[s] <= Cs.tci[s - 1]) tasc = false;
            tback[(size_t)(Cs.tci[s] * nc + i)] = Cs.tv[s];
        }
    }
    EXPECT_TRUE(asc && back == want);
    EXPECT_TRUE(tasc && tback == want);
    EXPECT_TRUE(Cs.nnz == structural);
    EXPECT_TRUE(Cs.longest_row == longest_row && Cs.longest_col == longest_col);
    std::printf("  %s: %lld rows, columns %lld -> %lld, entries %lld -> %lld, longest row %d -> %d, longest column %d -> %d\n", what, (long long)m, (long long)F.n,
                (long long)nc, (long long)F.nnz, (long long)Cs.nnz, F.longest_row, Cs.longest_row, F.longest_col, Cs.longest_col);
}

static Dense gram(const ObsHost& H) {   // Psi^T W Psi, dense n x n
    const Dense d = dense_of(H);
    Dense g((size_t)(H.n * H.n), 0.0);
    for (int64_t i = 0; i < H.n; ++i)
        for (int64_t j = 0; j < H.n; ++j)
            for (int64_t k = 0; k < H.n_obs; ++k) g[(size_t)(i * H.n + j)] += (H.w[(size_t)k] * d[(size_t)(k * H.n + i)]) * d[(size_t)(k * H.n + j)];
    return g;
}

int main() {
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

    // aggregates of 1 - 4 members over the grid: 2 x 2 boxes (4), the pairs of the last column (2) and of the last row (2), the corner alone (1), and
    // DOF 12 taken out of its box to stand alone (its box keeps 3)
    std::vector<int32_t> agg((size_t)n);
    for (int i = 0; i < g; ++i)
        for (int j = 0; j < g; ++j) agg[(size_t)(i * g + j)] = (i / 2) * 3 + (j / 2);   // 3 x 3 boxes: ids 0 .. 8
    agg[12] = 9;
    const int64_t nc = 10;
    std::vector<int> size((size_t)nc, 0);
    for (int32_t a : agg) ++size[(size_t)a];
    EXPECT_TRUE(*std::min_element(size.begin(), size.end()) == 1 && *std::max_element(size.begin(), size.end()) == 4 && std::count(size.begin(), size.end(), 2) >= 1 &&
                std::count(size.begin(), size.end(), 3) == 1);

    // Psi: an empty row, a one-entry row, a row over every DOF but 7, a row within one aggregate (box 0 = DOFs 0 1 5 6), short rows; DOF 7 is in no row
    std::vector<int64_t> prp {0};
    std::vector<int32_t> pci;
    std::vector<double> pv;
    auto row = [&](const std::vector<int32_t>& cols) {
        for (int32_t c : cols) pci.push_back(c), pv.push_back(lcg(1, 24) / 8.0 * (lcg(0, 1) ? 1 : -1));
        prp.push_back((int64_t)pci.size());
    };
    std::vector<int32_t> all_but_7;
    for (int32_t i = 0; i < n; ++i)
        if (i != 7) all_but_7.push_back(i);
    row({}), row({11}), row(all_but_7), row({0, 1, 5, 6}), row({3, 12, 24}), row({2, 8, 13, 18}), row({});
    const int64_t m = (int64_t)prp.size() - 1;
    const std::vector<double> w {0.5, 2.0, 1.0, 4.0, 0.25, 2.0, 8.0};
    std::vector<int32_t> ident((size_t)n);
    for (int64_t i = 0; i < n; ++i) ident[(size_t)i] = (int32_t)i;

    for (int pass = 0; pass < 2; ++pass) {
        const double scale = pass ? 0.375 : -1.0;
        ObsHost F, Cs;
        obs_build(n, m, prp.data(), pci.data(), pv.data(), pass ? w.data() : nullptr, ident.data(), &F);
        obs_coarsen(F, agg.data(), nc, &Cs);
        check_coarse(pass ? "weights, scale 0.375" : "W = I, scale -1", F, agg, nc, Cs);
        EXPECT_TRUE(Cs.rp[4] - Cs.rp[3] == 1);   // the row within one aggregate collapsed to one entry ...
        EXPECT_TRUE(Cs.v[(size_t)Cs.rp[3]] == F.v[(size_t)F.rp[3]] + F.v[(size_t)F.rp[3] + 1] + F.v[(size_t)F.rp[3] + 2] + F.v[(size_t)F.rp[3] + 3]);   // ... the sum of its four

        // (Psi P)^T W (Psi P) == P^T (Psi^T W Psi) P
        const Dense Gf = gram(F), Gc = gram(Cs);
        Dense want((size_t)(nc * nc), 0.0);
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = 0; j < n; ++j) want[(size_t)(agg[(size_t)i] * nc + agg[(size_t)j])] += Gf[(size_t)(i * n + j)];
        EXPECT_TRUE(Gc == want);

        // the merged coarsest matrix: the Galerkin product of the pattern part (keys ascending) + the coarse term, against dense P^T (A + term) P
        std::map<std::pair<int32_t, int32_t>, std::vector<double>> ce;
        for (int64_t i = 0; i < n; ++i)
            for (int32_t k = rowptr[(size_t)i]; k < rowptr[(size_t)i + 1]; ++k) {
                std::vector<double>& b = ce[{agg[(size_t)i], agg[(size_t)colidx[(size_t)k]]}];
                b.resize(4, 0.0);
                for (int q = 0; q < 4; ++q) b[(size_t)q] += raw[(size_t)(4 * k + q)];
            }
        std::vector<int32_t> crp((size_t)nc + 1, 0), cci;
        std::vector<double> craw;
        for (const auto& [key, b] : ce) {
            ++crp[(size_t)key.first + 1], cci.push_back(key.second);
            craw.insert(craw.end(), b.begin(), b.end());
        }
        for (int64_t i = 0; i < nc; ++i) crp[(size_t)i + 1] += crp[(size_t)i];
        const int64_t c2 = 2 * nc;
        Dense full((size_t)(c2 * c2), 0.0);
        for (int64_t i = 0; i < n; ++i)
            for (int32_t k = rowptr[(size_t)i]; k < rowptr[(size_t)i + 1]; ++k)
                for (int p = 0; p < 2; ++p)
                    for (int q = 0; q < 2; ++q)
                        full[(size_t)((2 * agg[(size_t)i] + p) * c2 + 2 * agg[(size_t)colidx[(size_t)k]] + q)] += raw[(size_t)(4 * k + 2 * p + q)];
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = 0; j < n; ++j) full[(size_t)(2 * agg[(size_t)i] * c2 + 2 * agg[(size_t)j])] += scale * Gf[(size_t)(i * n + j)];
        std::vector<int32_t> rp2, ci2;
        std::vector<double> v2;
        obs_merge_dense(crp.data(), cci.data(), craw.data(), Cs, scale, &rp2, &ci2, &v2);
        Dense merged((size_t)(c2 * c2), 0.0);
        bool sorted = true;
        for (int64_t r = 0; r < c2; ++r)
            for (int32_t e = rp2[(size_t)r]; e < rp2[(size_t)r + 1]; ++e) {
                if (e > rp2[(size_t)r] && ci2[(size_t)e] <= ci2[(size_t)e - 1]) sorted = false;
                merged[(size_t)(r * c2 + ci2[(size_t)e])] = v2[(size_t)e];
            }
        EXPECT_TRUE(sorted && (int64_t)rp2.size() == c2 + 1);
        EXPECT_TRUE(merged == full);
        std::printf("  merged coarsest matrix: %lld rows, %zu entries\n", (long long)c2, ci2.size());

        // a second level: Psi P_0 P_1, the coarse aggregates of sizes 1 - 4 again
        const std::vector<int32_t> agg1 {0, 0, 1, 0, 0, 1, 2, 2, 3, 1};
        ObsHost C2;
        obs_coarsen(Cs, agg1.data(), 4, &C2);
        check_coarse("the second level", Cs, agg1, 4, C2);
        std::vector<int32_t> both((size_t)n);
        for (int64_t i = 0; i < n; ++i) both[(size_t)i] = agg1[(size_t)agg[(size_t)i]];
        ObsHost direct;
        obs_coarsen(F, both.data(), 4, &direct);
        EXPECT_TRUE(dense_of(direct) == dense_of(C2) && direct.rp == C2.rp && direct.ci == C2.ci);
    }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
