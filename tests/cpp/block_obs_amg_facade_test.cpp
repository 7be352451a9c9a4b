// block_obs_amg_facade_test.cpp -- PDE::BlockSolver::carry_observations (include/fdapde_amd/pde.h): FDAPDE_SOLVER_BLOCK_AMG with the data term kept factored,
// the hierarchy carrying the term level by level (the knob "block_amg_obs").  On the reference's quasi_circle fixture with its golden incidence matrix, the
// AREAL smoothing system of tests/cpp/block_obs_facade_test.cpp, amg_coarse_rows = 256 (two levels):
//   * compute(A, Psi) -> solve with method FDAPDE_SOLVER_BLOCK_AMG throws, and the message contains "term";
//   * after carry_observations() the same solve agrees with PartialPivLU on the densified system to 1e-8, and fdapde_block_obs_amg_levels reports the levels;
//   * SMW<PDE::BlockSolver> with a rank-3 update on top agrees with the densified system's LU to 1e-8;
//   * carry_observations(false) restores the refusal.
// Runs on a real MI355X (pytest -m gpu: tests/test_cpp_block_obs_amg.py, which also compiles it); without a device it refuses to run.
//
// usage: block_obs_amg_facade_test <path to tests/golden/mesh>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "fdapde_amd/io.h"
#include "fdapde_amd/linear_algebra.h"
#include "fdapde_amd/pde.h"

using namespace fdapde::amd;

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                     \
    do {                                                                                                      \
        ++checks;                                                                                             \
        if (!(cond)) { ++failures; std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); }          \
    } while (0)

using Mesh = Triangulation<2, 2>;
using Pde = PDE<Mesh, DifferentialExpr, DMatrix<double>, FEM_HIP, fem_order<1>>;
// what a model writes against the reference keeps compiling on a solver that can hold a factored term
template struct fdapde::amd::SMW<Pde::BlockSolver>;

static const double kLambda = 1e-2;

static SpMatrix<double> scaled(const SpMatrix<double>& a, double s) {
    SpMatrix<double> b = a;
    for (double& v : b.values) v *= s;
    return b;
}
static SpMatrix<double> transposed(const SpMatrix<double>& a) {   // on the (structurally symmetric) pattern of a
    SpMatrix<double> t = a;
    for (int64_t i = 0; i < a.rows(); ++i)
        for (int32_t k = a.rowptr[(size_t)i]; k < a.rowptr[(size_t)i + 1]; ++k) t.values[(size_t)k] = a.coeff(a.colidx[(size_t)k], i);
    return t;
}
static double rel_diff(const DMatrix<double>& a, const DMatrix<double>& b) {
    double d = 0, s = 0;
    for (int64_t i = 0; i < a.size(); ++i) d += (a.data()[i] - b.data()[i]) * (a.data()[i] - b.data()[i]), s += b.data()[i] * b.data()[i];
    return std::sqrt(d / s);
}
// the four blocks densified (stacked order) + scale Psi^T W Psi in the (1,1) block
static DMatrix<double> densified(const SparseBlockMatrix<double, 2, 2>& A, int64_t n, const SpMatrix<double>& Psi, const std::vector<double>& w, double scale) {
    DMatrix<double> dense(2 * n, 2 * n, 0.0);
    for (int bi = 0; bi < 2; ++bi)
        for (int bj = 0; bj < 2; ++bj) {
            const SpMatrix<double>& blk = A.block(bi, bj);
            if (blk.values.empty()) continue;
            for (int64_t i = 0; i < n; ++i)
                for (int32_t k = blk.rowptr[(size_t)i]; k < blk.rowptr[(size_t)i + 1]; ++k) dense(bi * n + i, bj * n + blk.colidx[(size_t)k]) = blk.values[(size_t)k];
        }
    for (int64_t r = 0; r < Psi.rows(); ++r)
        for (int32_t a = Psi.rowptr[(size_t)r]; a < Psi.rowptr[(size_t)r + 1]; ++a)
            for (int32_t b = Psi.rowptr[(size_t)r]; b < Psi.rowptr[(size_t)r + 1]; ++b)
                dense(Psi.colidx[(size_t)a], Psi.colidx[(size_t)b]) += scale * w[(size_t)r] * Psi.values[(size_t)a] * Psi.values[(size_t)b];
    return dense;
}
static DMatrix<double> right_hand_side(int64_t n, const SpMatrix<double>& Psi, const std::vector<double>& w) {
    DMatrix<double> b(2 * n, 1, 0.0);
    for (int64_t r = 0; r < Psi.rows(); ++r)   // -Psi^T W z, z_r = sin(r + 1)
        for (int32_t k = Psi.rowptr[(size_t)r]; k < Psi.rowptr[(size_t)r + 1]; ++k)
            b(Psi.colidx[(size_t)k]) -= Psi.values[(size_t)k] * w[(size_t)r] * std::sin((double)(r + 1));
    for (int64_t i = 0; i < n; ++i) b(n + i) = kLambda * 0.1 * std::cos(0.37 * (double)i);
    return b;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <tests/golden/mesh>\n", argv[0]); return 2; }
    const std::string meshes = argv[1];
    MeshLoader<2, 2> circle(meshes, "quasi_circle");
    const DMatrix<int> inc_i = CSVReader<int>().parse_file(meshes + "/quasi_circle/incidence_matrix.csv");
    EXPECT_TRUE(inc_i.cols() == circle.mesh.n_cells() && inc_i.rows() == 7);
    if (fdapde_device_count() < 1) { std::printf("no HIP device: these tests have no CPU fallback\n"); return 3; }
    const Mesh& mesh = circle.mesh;
    auto L = -laplacian<FEM_HIP>();
    Pde pde(mesh, L);
    pde.set_forcing(DMatrix<double>::Zero(pde.quadrature_nodes().rows(), 1));
    pde.init();
    const int64_t n = pde.n_dofs();
    DMatrix<double> inc(inc_i.rows(), inc_i.cols());
    for (int64_t i = 0; i < inc.rows(); ++i)
        for (int64_t j = 0; j < inc.cols(); ++j) inc(i, j) = (double)inc_i(i, j);
    const auto e = pde.eval_basis(1, inc);
    EXPECT_TRUE(e.has_value() && e->Psi.rows() == 7 && e->Psi.cols() == n);
    const SpMatrix<double>& Psi = e->Psi;

    const SparseBlockMatrix<double, 2, 2> A(zero_block<double>(n, n), scaled(transposed(pde.stiff()), kLambda), scaled(pde.stiff(), kLambda), scaled(pde.mass(), kLambda));
    const std::vector<double> ones((size_t)Psi.rows(), 1.0);
    EXPECT_TRUE(fdapde_tune(pde.context(), "amg_coarse_rows", 256) == FDAPDE_OK);   // (2 n = 682: two levels)
    auto invA = pde.make_block_solver();
    invA.solver_options().method = FDAPDE_SOLVER_BLOCK_AMG;
    invA.solver_options().rtol = 1e-12;
    invA.compute(A, Psi, {}, -1.0, true);
    EXPECT_TRUE(bool(invA));
    const DMatrix<double> b = right_hand_side(n, Psi, ones);
    DMatrix<double> dense = densified(A, n, Psi, ones, -1.0);
    auto refused_with_term = [&]() {
        try { invA.solve(b); } catch (const std::runtime_error& err) { return std::string(err.what()).find("term") != std::string::npos; }
        return false;
    };
    EXPECT_TRUE(refused_with_term());   // without carry_observations() the multilevel stage refuses a live term
    {
        int32_t nl = 0;
        EXPECT_TRUE(fdapde_block_obs_amg_levels(pde.context(), 0, &nl, nullptr, nullptr, nullptr, nullptr) == FDAPDE_ENOTINIT);
    }
    invA.carry_observations();
    {
        const DMatrix<double> x = invA.solve(b);
        PartialPivLU lu;
        lu.compute(dense);
        const double d = rel_diff(x, lu.solve(b));
        std::printf("  BlockSolver with an areal term (BLOCK_AMG, the term carried): against the densified system's LU %.3e, |A x - b| / |b| = %.3e\n", d,
                    rel_diff(dense * x, b));
        EXPECT_TRUE(d <= 1e-8);
        int32_t nl = 0, longest[8] = {0}, tr[8] = {0}, tc[8] = {0};
        int64_t nnz[8] = {0};
        EXPECT_TRUE(fdapde_block_obs_amg_levels(pde.context(), 8, &nl, nnz, longest, tr, tc) == FDAPDE_OK);
        EXPECT_TRUE(nl == 2 && nnz[0] == Psi.nonZeros() && nnz[1] > 0 && nnz[1] <= nnz[0] && longest[1] <= longest[0] && tr[0] == 8 && tc[1] == 8);
        std::printf("  levels %d, nnz(Psi_l) %lld / %lld\n", nl, (long long)nnz[0], (long long)nnz[1]);
    }
    {   // Sherman-Morrison-Woodbury on top: (A + term + U V) x = b with a rank-3 update
        const int64_t q = 3;
        DMatrix<double> U(2 * n, q), V(q, 2 * n), invC(q, q, 0.0);
        for (int64_t k = 0; k < q; ++k) {
            invC(k, k) = 1.0;
            for (int64_t i = 0; i < 2 * n; ++i) U(i, k) = 1e-2 * std::sin(0.1 * (double)(i + 1) * (double)(k + 1)), V(k, i) = U(i, k);
        }
        SMW<Pde::BlockSolver> smw;
        const DMatrix<double> xs = smw.solve(invA, U, invC, V, b);
        const DMatrix<double> UV = U * V;
        for (int64_t i = 0; i < dense.size(); ++i) dense.data()[i] += UV.data()[i];
        PartialPivLU lu;
        lu.compute(dense);
        const double d = rel_diff(xs, lu.solve(b));
        std::printf("  SMW<BlockSolver> on the multilevel stage with the term carried, rank 3: against the densified system's LU %.3e\n", d);
        EXPECT_TRUE(d <= 1e-8);
    }
    invA.carry_observations(false);
    EXPECT_TRUE(refused_with_term());
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
