// block_amg_cols_facade_test.cpp -- the columns of a multilevel handle solve side by side, through the header-only facade: SMW<PDE::BlockSolver> with a
// four-column U under FDAPDE_SOLVER_BLOCK_AMG hands the handle five columns in ONE solve (b and U), which go as a batch of four and a single column (knob
// `amg_cols`, default 8; fdapde_amg_cols_trace says so).  The answer is that of the column-by-column path (`amg_cols` = 1) bit for bit, and agrees with
// PartialPivLU on the densified system to 1e-8.  The system is block_amg_facade_test.cpp's: unit_square_16, observations at every second node,
// `amg_coarse_rows` = 256 (two levels), `amg_setup_check` = 1.  The facade needs no new names: the handle passes n_rhs through.
// Runs on a real MI355X (pytest -m gpu: tests/test_cpp_block_amg_cols.py, which also compiles it); without a device it refuses to run.
//
// usage: block_amg_cols_facade_test <path to tests/golden/mesh>
#include <cmath>
#include <cstdio>
#include <cstring>
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

static const double kLambda = 1e-4;

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

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <tests/golden/mesh>\n", argv[0]); return 2; }
    MeshLoader<2, 2> square(argv[1], "unit_square_16");
    EXPECT_TRUE(square.mesh.n_nodes() == 289);
    if (fdapde_device_count() < 1) { std::printf("no HIP device: these tests have no CPU fallback\n"); return 3; }
    const Mesh& mesh = square.mesh;
    auto L = -laplacian<FEM_HIP>();
    Pde pde(mesh, L);
    pde.set_forcing(DMatrix<double>::Zero(pde.quadrature_nodes().rows(), 1));
    pde.init();
    const int64_t n = pde.n_dofs();

    const int64_t nl = (mesh.n_nodes() + 1) / 2;
    DMatrix<double> locs(nl, 2);
    for (int64_t i = 0; i < nl; ++i)
        for (int d = 0; d < 2; ++d) locs(i, d) = mesh.nodes()(2 * i, d);
    const auto e = pde.eval_basis(0, locs);
    EXPECT_TRUE(e.has_value());
    const SpMatrix<double> G = pde.gram(*e);
    const SparseBlockMatrix<double, 2, 2> A(scaled(G, -1.0), scaled(transposed(pde.stiff()), kLambda), scaled(pde.stiff(), kLambda), scaled(pde.mass(), kLambda));
    DMatrix<double> b(2 * n, 1, 0.0);
    for (int64_t i = 0; i < nl; ++i) b(2 * i) = -std::sin((double)i);   // -Psi^T z: location i sits on node 2 i
    for (int64_t i = 0; i < n; ++i) b(n + i) = kLambda * 0.1 * std::cos(0.37 * (double)i);

    auto invA = pde.make_block_solver();
    EXPECT_TRUE(fdapde_tune(pde.context(), "amg_coarse_rows", 256) == FDAPDE_OK && fdapde_tune(pde.context(), "amg_setup_check", 1) == FDAPDE_OK);
    invA.solver_options().method = FDAPDE_SOLVER_BLOCK_AMG;   // the method is taken by name
    invA.compute(A, true);
    EXPECT_TRUE(bool(invA));

    // Sherman-Morrison-Woodbury: (A + U V) x = b with a rank-4 update: one handle solve of five columns
    const int64_t q = 4;
    DMatrix<double> U(2 * n, q), V(q, 2 * n), invC(q, q, 0.0);
    for (int64_t k = 0; k < q; ++k) {
        invC(k, k) = 1.0;
        for (int64_t i = 0; i < 2 * n; ++i) U(i, k) = 1e-2 * std::sin(0.1 * (double)(i + 1) * (double)(k + 1)), V(k, i) = U(i, k);
    }
    SMW<Pde::BlockSolver> smw;
    const DMatrix<double> xs = smw.solve(invA, U, invC, V, b);   // (the default amg_cols = 8)
    fdapde_info info;
    EXPECT_TRUE(fdapde_info_get(pde.context(), &info) == FDAPDE_OK && info.method_used == FDAPDE_SOLVER_BLOCK_AMG && info.converged == 1);
    int32_t batches = -1, batched = -1, single = -1;
    EXPECT_TRUE(fdapde_amg_cols_trace(pde.context(), 2, &batches, &batched, &single) == FDAPDE_OK);
    std::printf("  five columns in one solve: %d batch(es) of %d columns in all, %d single column(s); %d outer iterations summed\n", batches, batched, single, info.iters);
    EXPECT_TRUE(batches == 1 && batched == 4 && single == 1);
    const int iters_batched = info.iters;

    // ... and column by column: the same bits
    EXPECT_TRUE(fdapde_tune(pde.context(), "amg_cols", 1) == FDAPDE_OK);
    const DMatrix<double> x1 = smw.solve(invA, U, invC, V, b);
    EXPECT_TRUE(fdapde_info_get(pde.context(), &info) == FDAPDE_OK && info.converged == 1 && info.iters == iters_batched);
    EXPECT_TRUE(fdapde_amg_cols_trace(pde.context(), 2, &batches, &batched, &single) == FDAPDE_OK && batches == 1 && batched == 4 && single == 6);
    EXPECT_TRUE(xs.size() == x1.size() && std::memcmp(xs.data(), x1.data(), sizeof(double) * (size_t)xs.size()) == 0);

    DMatrix<double> dense(2 * n, 2 * n, 0.0);
    for (int bi = 0; bi < 2; ++bi)
        for (int bj = 0; bj < 2; ++bj) {
            const SpMatrix<double>& blk = A.block(bi, bj);
            for (int64_t i = 0; i < n; ++i)
                for (int32_t k = blk.rowptr[(size_t)i]; k < blk.rowptr[(size_t)i + 1]; ++k) dense(bi * n + i, bj * n + blk.colidx[(size_t)k]) = blk.values[(size_t)k];
        }
    const DMatrix<double> UV = U * V;
    for (int64_t i = 0; i < dense.size(); ++i) dense.data()[i] += UV.data()[i];
    PartialPivLU lu;
    lu.compute(dense);
    const double d = rel_diff(xs, lu.solve(b));
    std::printf("  SMW<BlockSolver> with FDAPDE_SOLVER_BLOCK_AMG, rank 4, batched: against the densified system's LU %.3e\n", d);
    EXPECT_TRUE(d <= 1e-8);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
