// network_facade_test.cpp -- the header-only facade (include/fdapde_amd/pde.h, io.h) on 1-D meshes: the reference's linear network
// (test/data/mesh/network) loaded through MeshLoader<1,2>, and the interval Triangulation<1,1>(0, 1, 64).  -u'' + u = f (network) and
// -u'' = f (interval) with zero Dirichlet data solved through PDE<Triangulation<1,N>, ..., FEM_HIP, fem_order<R>> at R = 1, 2 and compared with
// the same problem driven through the C ABI directly; SMatrix<2> diffusion + SVector<2> advection through stiff(); Integrator<FEM_HIP, 1, R>
// over the network against the sum of the segment lengths.  Runs on a real MI355X (pytest -m gpu: tests/test_cpp_network.py, which also
// compiles it).
//
// usage: network_facade_test <path to tests/golden/mesh>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "fdapde_amd/io.h"
#include "fdapde_amd/pde.h"

using namespace fdapde::amd;

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                     \
    do {                                                                                                      \
        ++checks;                                                                                             \
        if (!(cond)) { ++failures; std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); }          \
    } while (0)

template <int N> static double f_rhs(const std::array<double, N>& x) {
    if constexpr (N == 1) return std::sin(3.0 * x[0]) + 1.0;
    else return std::sin(x[0]) + x[1] + 1.0;
}

// the same problem through the C ABI: mesh, space, operator, forcing at the device's quadrature nodes, zero Dirichlet data, init, solve
template <int N, int R>
static std::vector<double> capi_solution(const Triangulation<1, N>& mesh, const std::vector<fdapde_term>& terms, std::vector<double>* stiff) {
    fdapde_ctx* ctx = nullptr;
    std::vector<double> u;
    if (fdapde_ctx_create(0, &ctx) != FDAPDE_OK) return u;
    const int64_t nn = mesh.n_nodes(), nc = mesh.n_cells();
    std::vector<int32_t> cells((size_t)(nc * 2));
    std::vector<uint8_t> bnd((size_t)nn);
    for (int64_t c = 0; c < nc; ++c)
        for (int v = 0; v < 2; ++v) cells[(size_t)(c * 2 + v)] = mesh.cells()(c, v);
    for (int64_t i = 0; i < nn; ++i) bnd[(size_t)i] = mesh.boundary_nodes()(i, 0) ? 1 : 0;
    int64_t nd = 0, nnz = 0, ne = 0;
    int32_t nb = 0, nq = 0;
    bool ok = fdapde_mesh_upload(ctx, 1, N, nn, mesh.nodes().data(), nc, cells.data(), bnd.data()) == FDAPDE_OK &&
              fdapde_dofs_build(ctx, R, &nd) == FDAPDE_OK && fdapde_sizes(ctx, &nd, &nnz, &nb, &nq, &ne) == FDAPDE_OK;
    if (ok) {
        const int64_t rows = (int64_t)nq * nc;
        std::vector<double> q((size_t)(rows * N)), f((size_t)rows), g((size_t)nd, 0.0);
        ok = fdapde_quadrature_nodes(ctx, q.data()) == FDAPDE_OK;
        for (int64_t i = 0; ok && i < rows; ++i) {
            std::array<double, N> x;
            for (int d = 0; d < N; ++d) x[(size_t)d] = q[(size_t)(d * rows + i)];
            f[(size_t)i] = f_rhs<N>(x);
        }
        fdapde_options opt {FDAPDE_SOLVER_AUTO, 0, 1e-12, FDAPDE_ASSEMBLY_ROWS, 0, 0};
        fdapde_info info {};
        ok = ok && fdapde_set_operator(ctx, (int32_t)terms.size(), terms.data()) == FDAPDE_OK && fdapde_set_forcing(ctx, f.data(), 1) == FDAPDE_OK &&
             fdapde_init(ctx, &opt) == FDAPDE_OK;
        if (ok && stiff) {
            stiff->resize((size_t)nnz);
            ok = fdapde_matrix_values(ctx, FDAPDE_MAT_STIFF, stiff->data()) == FDAPDE_OK;
        }
        ok = ok && fdapde_set_dirichlet(ctx, g.data()) == FDAPDE_OK && fdapde_solve(ctx, &opt, &info) == FDAPDE_OK;
        if (ok) {
            u.resize((size_t)nd);
            if (fdapde_solution(ctx, u.data()) != FDAPDE_OK) u.clear();
        }
    }
    if (!ok) std::printf("  C ABI path: %s\n", fdapde_last_error(ctx));
    fdapde_ctx_destroy(ctx);
    return u;
}

static double rel_diff(const DMatrix<double>& a, const std::vector<double>& b) {
    double d = 0, n = 0;
    for (int64_t i = 0; i < a.rows(); ++i) d += (a(i) - b[(size_t)i]) * (a(i) - b[(size_t)i]), n += b[(size_t)i] * b[(size_t)i];
    return std::sqrt(d / n);
}

template <int N, int R, typename Op> static void solve_against_capi(const Triangulation<1, N>& mesh, const Op& L, const char* what) {
    PDE<Triangulation<1, N>, Op, ScalarField<N>, FEM_HIP, fem_order<R>> pde(mesh, L, ScalarField<N>(f_rhs<N>));
    EXPECT_TRUE(pde.n_dofs() == mesh.n_nodes() + (R == 2 ? mesh.n_cells() : 0));
    EXPECT_TRUE(pde.dof_coords().cols() == N && pde.quadrature_nodes().cols() == N);
    pde.set_dirichlet_bc(DMatrix<double>::Zero(pde.n_dofs(), 1));
    pde.init();
    std::vector<double> stiff;
    const std::vector<double> ref = capi_solution<N, R>(mesh, L.c_terms(), &stiff);
    EXPECT_TRUE(stiff.size() == pde.stiff().values.size());
    if (stiff.size() == pde.stiff().values.size()) {
        double d = 0;
        for (size_t k = 0; k < stiff.size(); ++k) d = std::fmax(d, std::fabs(stiff[k] - pde.stiff().values[k]));
        EXPECT_TRUE(d == 0.0);   // the same sweep on the same data
    }
    pde.solve();
    EXPECT_TRUE(pde.success());
    EXPECT_TRUE((int64_t)ref.size() == pde.n_dofs());
    if ((int64_t)ref.size() == pde.n_dofs()) {
        const double e = rel_diff(pde.solution(), ref);
        std::printf("  %s P%d: facade against the C ABI: relative difference %.3e\n", what, R, e);
        EXPECT_TRUE(e <= 1e-12);
    }
    for (int64_t i = 0; i < pde.n_dofs(); ++i)
        if (pde.boundary_dofs()(i)) EXPECT_TRUE(pde.solution()(i) == 0.0);
}

template <int N, int R> static void total_length(const Triangulation<1, N>& mesh, const char* what) {
    double len = 0, lin = 0;   // sum of |x1 - x0|, and the exact integral of x_1 (linear on every segment: |e| (x0 + x1) / 2)
    for (int64_t c = 0; c < mesh.n_cells(); ++c) {
        double l2 = 0;
        for (int d = 0; d < N; ++d) {
            const double a = mesh.nodes()(mesh.cells()(c, 1), d) - mesh.nodes()(mesh.cells()(c, 0), d);
            l2 += a * a;
        }
        len += std::sqrt(l2);
        lin += std::sqrt(l2) * 0.5 * (mesh.nodes()(mesh.cells()(c, 0), 0) + mesh.nodes()(mesh.cells()(c, 1), 0));
    }
    Integrator<FEM_HIP, 1, R> integrator;
    const double one = integrator.integrate(mesh, [](const std::array<double, N>&) { return 1.0; });
    std::printf("  %s P%d: integral of 1 %.15f, sum of the segment lengths %.15f\n", what, R, one, len);
    EXPECT_TRUE(std::fabs(one - len) <= 1e-12 * len);
    const double got = integrator.integrate(mesh, [](const std::array<double, N>& x) { return x[0]; });
    EXPECT_TRUE(std::fabs(got - lin) <= 1e-12 * std::fmax(1.0, std::fabs(lin)));
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <tests/golden/mesh>\n", argv[0]); return 2; }
    MeshLoader<1, 2> network(argv[1], "network");   // (host side: CSV reading and the shape checks of Triangulation<1,2>)
    EXPECT_TRUE(network.mesh.n_nodes() == 201 && network.mesh.n_cells() == 200 && network.points_.cols() == 2);
    const Triangulation<1, 1> interval(0.0, 1.0, 64);
    EXPECT_TRUE(interval.n_nodes() == 65 && interval.n_cells() == 64 && interval.nodes()(64) == 1.0);
    EXPECT_TRUE(interval.boundary_nodes()(0) == 1 && interval.boundary_nodes()(64) == 1 && interval.boundary_nodes()(32) == 0);
    EXPECT_TRUE(interval.cells()(10, 0) == 10 && interval.cells()(10, 1) == 11);
    const Triangulation<1, 1> from_nodes(interval.nodes());
    EXPECT_TRUE(from_nodes.n_cells() == 64);
    if (fdapde_device_count() < 1) { std::printf("no HIP device: these tests have no CPU fallback\n"); return 3; }
    const SMatrix<2> K {2.0, 0.3, 0.3, 1.0};
    const SVector<2> b {0.7, -0.2};
    auto L2 = -laplacian<FEM_HIP>() + reaction<FEM_HIP>(1.0);
    auto D2 = -diffusion<FEM_HIP>(K) + advection<FEM_HIP>(b) + reaction<FEM_HIP>(1.0);
    auto L1 = -laplacian<FEM_HIP>();
    solve_against_capi<2, 1>(network.mesh, L2, "network -u'' + u");
    solve_against_capi<2, 2>(network.mesh, L2, "network -u'' + u");
    solve_against_capi<2, 1>(network.mesh, D2, "network -div(K grad u) + b.grad u + u");
    solve_against_capi<2, 2>(network.mesh, D2, "network -div(K grad u) + b.grad u + u");
    solve_against_capi<1, 1>(interval, L1, "interval -u''");
    solve_against_capi<1, 2>(interval, L1, "interval -u''");
    total_length<2, 1>(network.mesh, "network");
    total_length<2, 2>(network.mesh, "network");
    total_length<1, 1>(interval, "interval");
    total_length<1, 2>(interval, "interval");
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
