// block_obs_facade_test.cpp -- PDE::BlockSolver with the data term kept factored (include/fdapde_amd/pde.h: compute(A, Psi, weights, scale),
// set_observations) on the reference's quasi_circle fixture with its golden incidence matrix: the AREAL smoothing system
//     [ -Psi^T W Psi   lambda R1^T ] [f]   [ -Psi^T W z ]
//     [ lambda R1      lambda R0   ] [g] = [ lambda u    ]
// whose Psi^T Psi does not lie on the FEM pattern (PDE::gram refuses an areal evaluation, a SparseBlockMatrix block with such entries is refused).
// eval_basis(1, incidence) -> compute(A, Psi) -> solve agrees with PartialPivLU on the densified system to 1e-8; set_observations with new weights changes the
// system accordingly; SMW<PDE::BlockSolver> with a rank-3 update on top agrees with the densified system's LU to 1e-8.
// Runs on a real MI355X (pytest -m gpu: tests/test_cpp_block_obs.py, which also compiles it); without a device it refuses to run.
//
// usage: block_obs_facade_test <path to tests/golden/mesh>
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
    {   // Psi^T Psi is off the pattern: two DOFs of a region that share no cell
        int64_t off = 0;
        for (int64_t r = 0; r < Psi.rows(); ++r)
            for (int32_t a = Psi.rowptr[(size_t)r]; a < Psi.rowptr[(size_t)r + 1]; ++a)
                for (int32_t b = Psi.rowptr[(size_t)r]; b < Psi.rowptr[(size_t)r + 1]; ++b) {
                    const int32_t i = Psi.colidx[(size_t)a], j = Psi.colidx[(size_t)b];
                    bool on = false;
                    for (int32_t k = pde.stiff().rowptr[(size_t)i]; k < pde.stiff().rowptr[(size_t)i + 1]; ++k) on = on || pde.stiff().colidx[(size_t)k] == j;
                    off += on ? 0 : 1;
                }
        EXPECT_TRUE(off > 0);
        bool refused = false;
        try { pde.gram(*e); } catch (const std::runtime_error&) { refused = true; }
        EXPECT_TRUE(refused);
    }

    const SparseBlockMatrix<double, 2, 2> A(zero_block<double>(n, n), scaled(transposed(pde.stiff()), kLambda), scaled(pde.stiff(), kLambda), scaled(pde.mass(), kLambda));
    const std::vector<double> ones((size_t)Psi.rows(), 1.0);
    auto invA = pde.make_block_solver();
    EXPECT_TRUE(!invA && pde.owns_context_of(invA));
    invA.solver_options().method = FDAPDE_SOLVER_GMRES;
    invA.solver_options().rtol = 1e-12;
    bool early = false;
    try { invA.set_observations(Psi); } catch (const std::runtime_error&) { early = true; }
    EXPECT_TRUE(early);   // compute() first
    invA.compute(A, Psi, {}, -1.0, true);
    EXPECT_TRUE(bool(invA));
    {
        int64_t n_obs = 0, nnz = 0;
        int32_t tr = 0, tc = 0;
        EXPECT_TRUE(fdapde_block_obs_info(pde.context(), &n_obs, &nnz, &tr, &tc) == FDAPDE_OK && n_obs == 7 && nnz == Psi.nonZeros() && tr == 8 && tc == 8);
    }
    const DMatrix<double> b = right_hand_side(n, Psi, ones);
    DMatrix<double> dense = densified(A, n, Psi, ones, -1.0);
    {
        const DMatrix<double> x = invA.solve(b);
        PartialPivLU lu;
        lu.compute(dense);
        const double d = rel_diff(x, lu.solve(b));
        std::printf("  BlockSolver with an areal term (GMRES): against the densified system's LU %.3e, |A x - b| / |b| = %.3e\n", d, rel_diff(dense * x, b));
        EXPECT_TRUE(d <= 1e-8);
        invA.solver_options().method = FDAPDE_SOLVER_DENSE;   // the dense stage sees the merged matrix
        const double dd = rel_diff(invA.solve(b), lu.solve(b));
        std::printf("  ... (dense inverse of the merged matrix): %.3e\n", dd);
        EXPECT_TRUE(dd <= 1e-8);
        invA.solver_options().method = FDAPDE_SOLVER_GMRES;
    }

    // the reweighting loop: new weights replace the term, the four blocks stay
    {
        std::vector<double> w((size_t)Psi.rows());
        DVector<double> wv(Psi.rows(), 1);
        for (int64_t r = 0; r < Psi.rows(); ++r) w[(size_t)r] = 0.5 + 0.2 * (double)r, wv(r) = w[(size_t)r];
        invA.set_observations(Psi, wv);
        const DMatrix<double> bw = right_hand_side(n, Psi, w);
        const DMatrix<double> dw = densified(A, n, Psi, w, -1.0);
        PartialPivLU lu;
        lu.compute(dw);
        const double d = rel_diff(invA.solve(bw), lu.solve(bw));
        std::printf("  set_observations with new weights: against the densified system's LU %.3e\n", d);
        EXPECT_TRUE(d <= 1e-8);
        bool refused = false;   // one weight per row of Psi
        try { invA.set_observations(Psi, DVector<double>(3, 1, 1.0)); } catch (const std::runtime_error&) { refused = true; }
        EXPECT_TRUE(refused);
        invA.set_observations(Psi);   // W = I again
    }

    // Sherman-Morrison-Woodbury on top: (A + term + U V) x = b with a rank-3 update
    {
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
        std::printf("  SMW<BlockSolver> with an areal term, rank 3: against the densified system's LU %.3e\n", d);
        EXPECT_TRUE(d <= 1e-8);
    }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
