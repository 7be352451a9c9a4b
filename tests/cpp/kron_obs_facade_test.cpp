// kron_obs_facade_test.cpp -- PDE::KroneckerSolver with the data term kept factored (include/fdapde_amd/pde.h: compute(A, Phi, Psi, weights, scale),
// set_observations) on the reference's quasi_circle fixture with its golden incidence matrix: the space-time AREAL smoothing system
//     [ -(Phi_t (x) Psi)^T W (Phi_t (x) Psi) - lambda (P_t (x) R0)    lambda (M_t (x) R1^T) ]
//     [  lambda (M_t (x) R1)                                          lambda (M_t (x) R0)   ]
// with kM = 2 time nodes, p = 3 observation instants off the nodes (Phi = [Phi_t, 0]: P1 hat functions) and missing observations (exact zeros in W).
// eval_basis(1, incidence) -> compute(A, Phi, Psi, weights) -> solve equals the same system driven through the C ABI on a context of its own bit for bit and
// agrees with PartialPivLU on the densified system to 1e-8; set_observations replaces the term; SMW<PDE::KroneckerSolver> with a rank-2 update on top agrees
// with the densified system's LU to 1e-8.
// Runs on a real MI355X (pytest -m gpu: tests/test_cpp_kron_obs.py, which also compiles it); without a device it refuses to run.
//
// usage: kron_obs_facade_test <path to tests/golden/mesh>
#include <algorithm>
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
template struct fdapde::amd::SMW<Pde::KroneckerSolver>;

static const double kLambda = 1e-2;
static const int kM = 2, kP = 3;
static const double kTimes[kP] = {0.125, 0.5, 0.8125};

static SpMatrix<double> transposed(const SpMatrix<double>& a) {   // on the (structurally symmetric) pattern of a
    SpMatrix<double> t = a;
    for (int64_t i = 0; i < a.rows(); ++i)
        for (int32_t k = a.rowptr[(size_t)i]; k < a.rowptr[(size_t)i + 1]; ++k) t.values[(size_t)k] = a.coeff(a.colidx[(size_t)k], i);
    return t;
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
// [Phi_t, 0]: the hat functions of the kM time nodes at the kP instants
static DMatrix<double> time_basis() {
    const double h = 1.0 / (kM - 1);
    DMatrix<double> phi(kP, 2 * kM, 0.0);
    for (int t = 0; t < kP; ++t)
        for (int r = 0; r < kM; ++r) phi(t, r) = std::max(0.0, 1.0 - std::fabs(kTimes[t] - r * h) / h);
    return phi;
}
// weights in the Kronecker order (instant tau, location k at tau n_obs + k); every fourth observation is missing
static DVector<double> weights_of(int64_t n_obs, double base) {
    DVector<double> w(kP * n_obs, 1);
    for (int64_t e = 0; e < kP * n_obs; ++e) w(e) = e % 4 == 1 ? 0.0 : base + 0.125 * (double)(e % 3);
    return w;
}
static double rel_diff(const DMatrix<double>& a, const DMatrix<double>& b) {
    double d = 0, s = 0;
    for (int64_t i = 0; i < a.size(); ++i) d += (a.data()[i] - b.data()[i]) * (a.data()[i] - b.data()[i]), s += b.data()[i] * b.data()[i];
    return std::sqrt(d / s);
}
// the Kronecker sum densified + scale B^T W B, B = Phi (x) Psi
static DMatrix<double> densified(const KroneckerSum& A, int64_t n, const DMatrix<double>& Phi, const SpMatrix<double>& Psi, const DVector<double>& w, double scale) {
    const int64_t q = 2 * kM, m = Psi.rows();
    const SpMatrix<double> E = A.eval();
    DMatrix<double> dense(q * n, q * n, 0.0);
    for (int64_t i = 0; i < q * n; ++i)
        for (int32_t k = E.rowptr[(size_t)i]; k < E.rowptr[(size_t)i + 1]; ++k) dense(i, E.colidx[(size_t)k]) = E.values[(size_t)k];
    for (int64_t r = 0; r < q; ++r)
        for (int64_t s = 0; s < q; ++s)
            for (int t = 0; t < kP; ++t) {
                const double f = Phi(t, r) * Phi(t, s);
                if (f == 0.0) continue;
                for (int64_t o = 0; o < m; ++o)
                    for (int32_t a = Psi.rowptr[(size_t)o]; a < Psi.rowptr[(size_t)o + 1]; ++a)
                        for (int32_t b = Psi.rowptr[(size_t)o]; b < Psi.rowptr[(size_t)o + 1]; ++b)
                            dense(r * n + Psi.colidx[(size_t)a], s * n + Psi.colidx[(size_t)b]) += scale * f * w(t * m + o) * Psi.values[(size_t)a] * Psi.values[(size_t)b];
            }
    return dense;
}
static DMatrix<double> right_hand_side(int64_t n, const DMatrix<double>& Phi, const SpMatrix<double>& Psi, const DVector<double>& w) {
    const int64_t m = Psi.rows();
    DMatrix<double> b(2 * kM * n, 1, 0.0);
    for (int t = 0; t < kP; ++t)   // -B^T W z, z[tau m + o] = sin(tau m + o + 1)
        for (int64_t o = 0; o < m; ++o)
            for (int r = 0; r < kM; ++r)
                for (int32_t k = Psi.rowptr[(size_t)o]; k < Psi.rowptr[(size_t)o + 1]; ++k)
                    b(r * n + Psi.colidx[(size_t)k]) -= Phi(t, r) * Psi.values[(size_t)k] * w(t * m + o) * std::sin((double)(t * m + o + 1));
    for (int r = 0; r < kM; ++r)
        for (int64_t i = 0; i < n; ++i) b((kM + r) * n + i) = kLambda * 0.1 * std::cos(0.37 * (double)(i + r));
    return b;
}

// the same system through the C ABI alone, on a context of its own: four terms, the two on R0 handing over one pointer, then fdapde_kron_set_obs
static bool abi_route(const Mesh& mesh, const DMatrix<double>& Phi, const SpMatrix<double>& Psi, const DVector<double>& w, const DMatrix<double>& b,
                      const fdapde_options& opt, DMatrix<double>& x) {
    fdapde_ctx* ctx = nullptr;
    if (fdapde_ctx_create(0, &ctx) != FDAPDE_OK) return false;
    const int64_t nn = mesh.n_nodes(), nc = mesh.n_cells();
    std::vector<int32_t> cells((size_t)(nc * 3));
    std::vector<uint8_t> bnd((size_t)nn);
    for (int64_t c = 0; c < nc; ++c)
        for (int v = 0; v < 3; ++v) cells[(size_t)(c * 3 + v)] = mesh.cells()(c, v);
    for (int64_t i = 0; i < nn; ++i) bnd[(size_t)i] = mesh.boundary_nodes()(i, 0) ? 1 : 0;
    int64_t nd = 0, nnz = 0, ne = 0;
    int32_t nb = 0, nq = 0;
    bool ok = fdapde_mesh_upload(ctx, 2, 2, nn, mesh.nodes().data(), nc, cells.data(), bnd.data()) == FDAPDE_OK && fdapde_dofs_build(ctx, 1, &nd) == FDAPDE_OK &&
              fdapde_sizes(ctx, &nd, &nnz, &nb, &nq, &ne) == FDAPDE_OK;
    if (ok) {
        fdapde_term lap {};
        lap.kind = FDAPDE_LAPLACIAN, lap.coef = -1.0;
        const std::vector<double> f((size_t)(nq * nc), 0.0);
        SpMatrix<double> R1, R0;
        R1.n_rows = R1.n_cols = nd, R1.rowptr.resize((size_t)nd + 1), R1.colidx.resize((size_t)nnz), R1.values.resize((size_t)nnz);
        ok = fdapde_set_operator(ctx, 1, &lap) == FDAPDE_OK && fdapde_set_forcing(ctx, f.data(), 1) == FDAPDE_OK && fdapde_init(ctx, nullptr) == FDAPDE_OK &&
             fdapde_pattern_get(ctx, R1.rowptr.data(), R1.colidx.data()) == FDAPDE_OK && fdapde_matrix_values(ctx, FDAPDE_MAT_STIFF, R1.values.data()) == FDAPDE_OK;
        R0 = R1;
        ok = ok && fdapde_matrix_values(ctx, FDAPDE_MAT_MASS, R0.values.data()) == FDAPDE_OK;
        if (ok) {
            const SpMatrix<double> R1t = transposed(R1);
            const DMatrix<double> T[4] = {time_block(true, -kLambda, 0, 0), time_block(false, kLambda, 0, 1), time_block(false, kLambda, 1, 0),
                                          time_block(false, kLambda, 1, 1)};
            const double* tp[4] = {T[0].data(), T[1].data(), T[2].data(), T[3].data()};
            const double* sp[4] = {R0.values.data(), R1t.values.data(), R1.values.data(), R0.values.data()};
            const std::vector<int64_t> rowptr(Psi.rowptr.begin(), Psi.rowptr.end());
            x.resize(2 * kM * nd, b.cols());
            fdapde_info info;
            int32_t p = 0, fr = 0, fc = 0;
            int64_t n_obs = 0, nz = 0;
            ok = fdapde_kron_compute(ctx, 2 * kM, 4, tp, sp, 1) == FDAPDE_OK &&
                 fdapde_kron_set_obs(ctx, kP, Phi.data(), Psi.rows(), rowptr.data(), Psi.colidx.data(), Psi.values.data(), w.data(), -1.0) == FDAPDE_OK &&
                 fdapde_kron_obs_info(ctx, &p, &n_obs, &nz, &fr, &fc) == FDAPDE_OK && p == kP && n_obs == Psi.rows() && nz == Psi.nonZeros() && fr >= 1 && fc >= 1 &&
                 fdapde_kron_solve(ctx, &opt, b.data(), (int32_t)b.cols(), x.data(), &info) == FDAPDE_OK;
        }
    }
    if (!ok) std::printf("  C ABI route: %s\n", fdapde_last_error(ctx));
    fdapde_ctx_destroy(ctx);
    return ok;
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
    const int64_t n = pde.n_dofs(), q = 2 * kM;

    DMatrix<double> inc(inc_i.rows(), inc_i.cols());
    for (int64_t i = 0; i < inc.rows(); ++i)
        for (int64_t j = 0; j < inc.cols(); ++j) inc(i, j) = (double)inc_i(i, j);
    const auto e = pde.eval_basis(1, inc);
    EXPECT_TRUE(e.has_value() && e->Psi.rows() == 7 && e->Psi.cols() == n);
    const SpMatrix<double>& Psi = e->Psi;

    const SpMatrix<double> R1t = transposed(pde.stiff());
    const KroneckerSum A = Kronecker(time_block(true, -kLambda, 0, 0), pde.mass()) + Kronecker(time_block(false, kLambda, 0, 1), R1t) +
                           Kronecker(time_block(false, kLambda, 1, 0), pde.stiff()) + Kronecker(time_block(false, kLambda, 1, 1), pde.mass());
    const DMatrix<double> Phi = time_basis();
    const DVector<double> w = weights_of(Psi.rows(), 1.0);
    auto invA = pde.make_kronecker_solver();
    EXPECT_TRUE(!invA && pde.owns_context_of(invA));
    invA.solver_options().method = FDAPDE_SOLVER_GMRES;
    invA.solver_options().rtol = 1e-12;
    bool early = false;
    try { invA.set_observations(Phi, Psi); } catch (const std::runtime_error&) { early = true; }
    EXPECT_TRUE(early);   // compute() first
    invA.compute(A, Phi, Psi, w, -1.0, true);
    EXPECT_TRUE(bool(invA));
    {
        int32_t p = 0, fr = 0, fc = 0;
        int64_t n_obs = 0, nnz = 0;
        EXPECT_TRUE(fdapde_kron_obs_info(pde.context(), &p, &n_obs, &nnz, &fr, &fc) == FDAPDE_OK && p == kP && n_obs == 7 && nnz == Psi.nonZeros());
    }
    const DMatrix<double> b = right_hand_side(n, Phi, Psi, w);
    DMatrix<double> dense = densified(A, n, Phi, Psi, w, -1.0);
    const DMatrix<double> x = invA.solve(b);
    EXPECT_TRUE(invA.info().converged == 1 && invA.info().method_used == FDAPDE_SOLVER_GMRES && invA.info().iters > 0);
    {
        PartialPivLU lu;
        lu.compute(dense);
        const double d = rel_diff(x, lu.solve(b));
        std::printf("  KroneckerSolver with an areal term (GMRES, %d iterations): against the densified system's LU %.3e, |A x - b| / |b| = %.3e\n", invA.info().iters, d,
                    rel_diff(dense * x, b));
        EXPECT_TRUE(d <= 1e-8);
    }
    DMatrix<double> x_abi;
    const bool abi_ok = abi_route(mesh, Phi, Psi, w, b, invA.solver_options(), x_abi);
    EXPECT_TRUE(abi_ok);
    if (abi_ok) EXPECT_TRUE(x_abi.rows() == x.rows() && x_abi.cols() == x.cols() && std::equal(x.data(), x.data() + x.size(), x_abi.data()));

    // set_observations replaces the term (other weights, the pattern terms stay); the dense stage sees the merged matrix
    {
        const DVector<double> w2 = weights_of(Psi.rows(), 0.5);
        invA.set_observations(Phi, Psi, w2);
        invA.solver_options().method = FDAPDE_SOLVER_DENSE;
        const DMatrix<double> b2 = right_hand_side(n, Phi, Psi, w2);
        PartialPivLU lu;
        lu.compute(densified(A, n, Phi, Psi, w2, -1.0));
        const DMatrix<double> x2 = invA.solve(b2);
        const double d = rel_diff(x2, lu.solve(b2));
        std::printf("  set_observations with new weights (dense inverse of the merged matrix): against the densified system's LU %.3e\n", d);
        EXPECT_TRUE(invA.info().method_used == FDAPDE_SOLVER_DENSE && d <= 1e-8);
        bool refused = false;   // p weights per row of Psi
        try { invA.set_observations(Phi, Psi, DVector<double>(5, 1, 1.0)); } catch (const std::runtime_error&) { refused = true; }
        EXPECT_TRUE(refused);
        refused = false;        // Phi needs q columns
        try { invA.set_observations(DMatrix<double>(kP, q + 1, 1.0), Psi); } catch (const std::runtime_error&) { refused = true; }
        EXPECT_TRUE(refused);
        invA.set_observations(Phi, Psi, w);   // the first term again
    }

    // Sherman-Morrison-Woodbury on top: (A + term + U V) x = b with a rank-2 update
    {
        const int64_t rk = 2, N = q * n;
        DMatrix<double> U(N, rk), V(rk, N), invC(rk, rk, 0.0);
        for (int64_t k = 0; k < rk; ++k) {
            invC(k, k) = 1.0;
            for (int64_t i = 0; i < N; ++i) U(i, k) = 1e-2 * std::sin(0.1 * (double)(i + 1) * (double)(k + 1)), V(k, i) = U(i, k);
        }
        SMW<Pde::KroneckerSolver> smw;
        const DMatrix<double> xs = smw.solve(invA, U, invC, V, b);
        const DMatrix<double> UV = U * V;
        for (int64_t i = 0; i < dense.size(); ++i) dense.data()[i] += UV.data()[i];
        PartialPivLU lu;
        lu.compute(dense);
        const double d = rel_diff(xs, lu.solve(b));
        std::printf("  SMW<KroneckerSolver> with an areal term, rank 2: against the densified system's LU %.3e\n", d);
        EXPECT_TRUE(d <= 1e-8);
    }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
