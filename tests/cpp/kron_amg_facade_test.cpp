// kron_amg_facade_test.cpp -- FDAPDE_SOLVER_KRON_AMG through the header-only facade (include/fdapde_amd/pde.h, linear_algebra.h) on the reference's
// unit_square_16 fixture: PDE::KroneckerSolver::solver_options() names the method, and SMW<PDE::KroneckerSolver> solves the space-time separable smoothing
// system
//     [ -(I_m (x) G) - lambda (P_t (x) R0)    lambda (M_t (x) R1^T) ]
//     [  lambda (M_t (x) R1)                  lambda (M_t (x) R0)   ]
// (m = 3 time nodes, q = 6, G the indicator of every second node) plus a rank-3 update through it; the result agrees with PartialPivLU on the densified
// system to 1e-8.  The context's `amg_coarse_rows` is set to 256, so that the 1 734-row system has several levels and the cycle kernels run, and
// `amg_setup_check` to 1.
// Runs on a real MI355X (pytest -m gpu: tests/test_cpp_kron_amg.py, which also compiles it); without a device it refuses to run.
//
// usage: kron_amg_facade_test <path to tests/golden/mesh>
#include <cmath>
#include <cstdio>
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
static const int kM = 3;

static SpMatrix<double> transposed(const SpMatrix<double>& a) {   // on the (structurally symmetric) pattern of a
    SpMatrix<double> t = a;
    for (int64_t i = 0; i < a.rows(); ++i)
        for (int32_t k = a.rowptr[(size_t)i]; k < a.rowptr[(size_t)i + 1]; ++k) t.values[(size_t)k] = a.coeff(a.colidx[(size_t)k], i);
    return t;
}
static SpMatrix<double> indicator(const SpMatrix<double>& a) {   // of every second DOF on the diagonal, on the pattern of a
    SpMatrix<double> g = a;
    for (int64_t i = 0; i < a.rows(); ++i)
        for (int32_t k = a.rowptr[(size_t)i]; k < a.rowptr[(size_t)i + 1]; ++k) g.values[(size_t)k] = (a.colidx[(size_t)k] == i && i % 2 == 0) ? 1.0 : 0.0;
    return g;
}
// P1 mass (stiff = false) / stiffness matrix of kM nodes on [0, 1], times s, as block (r, c) of a 2 kM x 2 kM matrix
static DMatrix<double> time_block(bool stiff, double s, int r, int c) {
    const double h = 1.0 / (kM - 1);
    DMatrix<double> t(2 * kM, 2 * kM, 0.0);
    for (int e = 0; e + 1 < kM; ++e)
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) t(r * kM + e + a, c * kM + e + b) += s * (stiff ? (a == b ? 1.0 : -1.0) / h : (a == b ? 2.0 : 1.0) * h / 6.0);
    return t;
}
static DMatrix<double> identity_block(double s, int r, int c) {
    DMatrix<double> t(2 * kM, 2 * kM, 0.0);
    for (int i = 0; i < kM; ++i) t(r * kM + i, c * kM + i) = s;
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
    const int64_t n = pde.n_dofs(), q = 2 * kM, N = q * n;

    const SpMatrix<double> G = indicator(pde.stiff()), R1t = transposed(pde.stiff());
    const KroneckerSum A = Kronecker(identity_block(-1.0, 0, 0), G) + Kronecker(time_block(true, -kLambda, 0, 0), pde.mass()) +
                           Kronecker(time_block(false, kLambda, 0, 1), R1t) + Kronecker(time_block(false, kLambda, 1, 0), pde.stiff()) +
                           Kronecker(time_block(false, kLambda, 1, 1), pde.mass());
    EXPECT_TRUE(A.rows() == N && A.time_size() == q);
    DMatrix<double> b(N, 1, 0.0);
    for (int r = 0; r < kM; ++r)
        for (int64_t i = 0; i < n; ++i) {
            if (i % 2 == 0) b(r * n + i) = -std::sin((double)(i + 7 * r));
            b((kM + r) * n + i) = kLambda * 0.1 * std::cos(0.37 * (double)(i + r));
        }

    auto invA = pde.make_kronecker_solver();
    EXPECT_TRUE(fdapde_tune(pde.context(), "amg_coarse_rows", 256) == FDAPDE_OK && fdapde_tune(pde.context(), "amg_setup_check", 1) == FDAPDE_OK);
    invA.solver_options().method = FDAPDE_SOLVER_KRON_AMG;   // the method is taken by name
    invA.solver_options().rtol = 1e-12;
    invA.compute(A, true);
    EXPECT_TRUE(bool(invA));

    const SpMatrix<double> E = A.eval();
    DMatrix<double> dense(N, N, 0.0);
    for (int64_t i = 0; i < N; ++i)
        for (int32_t k = E.rowptr[(size_t)i]; k < E.rowptr[(size_t)i + 1]; ++k) dense(i, E.colidx[(size_t)k]) = E.values[(size_t)k];
    // Sherman-Morrison-Woodbury: (A + U V) x = b with a rank-3 update, every inner solve through the multilevel stage
    const int64_t rk = 3;
    DMatrix<double> U(N, rk), V(rk, N), invC(rk, rk, 0.0);
    for (int64_t k = 0; k < rk; ++k) {
        invC(k, k) = 1.0;
        for (int64_t i = 0; i < N; ++i) U(i, k) = 1e-3 * std::sin(0.1 * (double)(i + 1) * (double)(k + 1)), V(k, i) = U(i, k);
    }
    SMW<Pde::KroneckerSolver> smw;
    const DMatrix<double> xs = smw.solve(invA, U, invC, V, b);
    fdapde_info info;
    EXPECT_TRUE(fdapde_info_get(pde.context(), &info) == FDAPDE_OK && info.method_used == FDAPDE_SOLVER_KRON_AMG && info.converged == 1);
    int32_t levels = 0;
    EXPECT_TRUE(fdapde_kron_amg_hierarchy(pde.context(), 0, &levels, nullptr, nullptr, nullptr, nullptr) == FDAPDE_OK && levels >= 3);
    const DMatrix<double> UV = U * V;
    for (int64_t i = 0; i < dense.size(); ++i) dense.data()[i] += UV.data()[i];
    PartialPivLU lu;
    lu.compute(dense);
    const double d = rel_diff(xs, lu.solve(b));
    std::printf("  SMW<KroneckerSolver> with FDAPDE_SOLVER_KRON_AMG, rank 3, %d levels: against the densified system's LU %.3e (%d outer iterations in the last solve)\n",
                levels, d, info.iters);
    EXPECT_TRUE(d <= 1e-8);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
