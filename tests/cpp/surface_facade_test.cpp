// surface_facade_test.cpp -- the header-only facade (include/fdapde_amd/pde.h, io.h) on a surface mesh, Triangulation<2,3>:
// the reference's 2.5-D fixture (test/data/mesh/surface) loaded through MeshLoader<2,3>, -Lap_S u = f with zero Dirichlet data solved through
// PDE<Triangulation<2,3>, ..., FEM_HIP, fem_order<R>> at R = 1, 2 and compared with the same problem driven through the C ABI directly;
// SMatrix<3> diffusion + SVector<3> advection through stiff(); Integrator<FEM_HIP, 2, R>::integrate over the surface against the sum of the
// cells' areas computed here.  Runs on a real MI355X (pytest -m gpu: tests/test_cpp_surface.py, which also compiles it).
//
// usage: surface_facade_test <path to tests/golden/mesh>
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

static std::string MESH_PATH;
static double f_rhs(const std::array<double, 3>& x) { return std::sin(x[0]) + x[1] * x[2] + 1.0; }

// the same problem through the C ABI: mesh, space, operator, forcing at the device's quadrature nodes, zero Dirichlet data, init, solve
template <int R>
static std::vector<double> capi_solution(const Triangulation<2, 3>& mesh, const std::vector<fdapde_term>& terms, std::vector<double>* stiff) {
    fdapde_ctx* ctx = nullptr;
    std::vector<double> u;
    if (fdapde_ctx_create(0, &ctx) != FDAPDE_OK) return u;
    const int64_t nn = mesh.n_nodes(), nc = mesh.n_cells();
    std::vector<int32_t> cells((size_t)(nc * 3));
    std::vector<uint8_t> bnd((size_t)nn);
    for (int64_t c = 0; c < nc; ++c)
        for (int v = 0; v < 3; ++v) cells[(size_t)(c * 3 + v)] = mesh.cells()(c, v);
    for (int64_t i = 0; i < nn; ++i) bnd[(size_t)i] = mesh.boundary_nodes()(i, 0) ? 1 : 0;
    int64_t nd = 0, nnz = 0, ne = 0;
    int32_t nb = 0, nq = 0;
    bool ok = fdapde_mesh_upload(ctx, 2, 3, nn, mesh.nodes().data(), nc, cells.data(), bnd.data()) == FDAPDE_OK &&
              fdapde_dofs_build(ctx, R, &nd) == FDAPDE_OK && fdapde_sizes(ctx, &nd, &nnz, &nb, &nq, &ne) == FDAPDE_OK;
    if (ok) {
        const int64_t rows = (int64_t)nq * nc;
        std::vector<double> q((size_t)(rows * 3)), f((size_t)rows), g((size_t)nd, 0.0);
        ok = fdapde_quadrature_nodes(ctx, q.data()) == FDAPDE_OK;
        for (int64_t i = 0; ok && i < rows; ++i) f[(size_t)i] = f_rhs({q[(size_t)i], q[(size_t)(rows + i)], q[(size_t)(2 * rows + i)]});
        fdapde_options opt {FDAPDE_SOLVER_AUTO, 0, 1e-10, FDAPDE_ASSEMBLY_ROWS, 0, 0};
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

template <int R> static void surface_laplace_beltrami(const Triangulation<2, 3>& mesh) {
    auto L = -laplacian<FEM_HIP>();
    PDE<Triangulation<2, 3>, decltype(L), ScalarField<3>, FEM_HIP, fem_order<R>> pde(mesh, L, ScalarField<3>(f_rhs));
    EXPECT_TRUE(pde.n_dofs() == (R == 1 ? 340 : 1296));
    EXPECT_TRUE(pde.dof_coords().cols() == 3 && pde.quadrature_nodes().cols() == 3);
    pde.set_dirichlet_bc(DMatrix<double>::Zero(pde.n_dofs(), 1));
    pde.init();
    pde.solve();
    EXPECT_TRUE(pde.success());
    const std::vector<double> ref = capi_solution<R>(mesh, L.c_terms(), nullptr);
    EXPECT_TRUE((int64_t)ref.size() == pde.n_dofs());
    if ((int64_t)ref.size() == pde.n_dofs()) {
        const double e = rel_diff(pde.solution(), ref);
        std::printf("  P%d: facade against the C ABI: relative difference %.3e\n", R, e);
        EXPECT_TRUE(e <= 1e-12);
    }
    for (int64_t i = 0; i < pde.n_dofs(); ++i)   // zero Dirichlet data on the open surface's boundary
        if (pde.boundary_dofs()(i)) EXPECT_TRUE(pde.solution()(i) == 0.0);
}

template <int R> static void surface_diffusion_advection(const Triangulation<2, 3>& mesh) {
    const SMatrix<3> K {2.0, 0.3, 0.1, 0.3, 1.0, 0.2, 0.1, 0.2, 1.5};
    const SVector<3> b {0.7, -0.2, 0.4};
    auto L = -diffusion<FEM_HIP>(K) + advection<FEM_HIP>(b) + reaction<FEM_HIP>(1.0);
    PDE<Triangulation<2, 3>, decltype(L), ScalarField<3>, FEM_HIP, fem_order<R>> pde(mesh, L, ScalarField<3>(f_rhs));
    pde.set_dirichlet_bc(DMatrix<double>::Zero(pde.n_dofs(), 1));
    pde.init();
    std::vector<double> stiff;
    const std::vector<double> ref = capi_solution<R>(mesh, L.c_terms(), &stiff);
    EXPECT_TRUE(stiff.size() == pde.stiff().values.size());
    if (stiff.size() == pde.stiff().values.size()) {
        double d = 0;
        for (size_t k = 0; k < stiff.size(); ++k) d = std::fmax(d, std::fabs(stiff[k] - pde.stiff().values[k]));
        EXPECT_TRUE(d == 0.0);   // the same sweep on the same data
    }
    pde.solve();
    EXPECT_TRUE(pde.success());
    EXPECT_TRUE((int64_t)ref.size() == pde.n_dofs());
    if ((int64_t)ref.size() == pde.n_dofs()) EXPECT_TRUE(rel_diff(pde.solution(), ref) <= 1e-12);
}

template <int R> static void surface_integral(const Triangulation<2, 3>& mesh) {
    double area = 0;   // sum of |(x1 - x0) x (x2 - x0)| / 2
    for (int64_t c = 0; c < mesh.n_cells(); ++c) {
        double a[3], bb[3];
        for (int d = 0; d < 3; ++d) {
            const double x0 = mesh.nodes()(mesh.cells()(c, 0), d);
            a[d] = mesh.nodes()(mesh.cells()(c, 1), d) - x0, bb[d] = mesh.nodes()(mesh.cells()(c, 2), d) - x0;
        }
        const double c0 = a[1] * bb[2] - a[2] * bb[1], c1 = a[2] * bb[0] - a[0] * bb[2], c2 = a[0] * bb[1] - a[1] * bb[0];
        area += 0.5 * std::sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    }
    Integrator<FEM_HIP, 2, R> integrator;
    const double one = integrator.integrate(mesh, [](const std::array<double, 3>&) { return 1.0; });
    std::printf("  P%d: integral of 1 over the surface %.15f, sum of the cell areas %.15f\n", R, one, area);
    EXPECT_TRUE(std::fabs(one - area) <= 1e-12 * area);
    // the quadrature of a linear function is exact on every flat cell: integral of x_3 = sum |e| (z0 + z1 + z2) / 3
    double lin = 0;
    for (int64_t c = 0; c < mesh.n_cells(); ++c) {
        double a[3], bb[3], zs = 0;
        for (int d = 0; d < 3; ++d) {
            const double x0 = mesh.nodes()(mesh.cells()(c, 0), d);
            a[d] = mesh.nodes()(mesh.cells()(c, 1), d) - x0, bb[d] = mesh.nodes()(mesh.cells()(c, 2), d) - x0;
        }
        for (int v = 0; v < 3; ++v) zs += mesh.nodes()(mesh.cells()(c, v), 2);
        const double c0 = a[1] * bb[2] - a[2] * bb[1], c1 = a[2] * bb[0] - a[0] * bb[2], c2 = a[0] * bb[1] - a[1] * bb[0];
        lin += 0.5 * std::sqrt(c0 * c0 + c1 * c1 + c2 * c2) * zs / 3.0;
    }
    const double got = integrator.integrate(mesh, [](const std::array<double, 3>& x) { return x[2]; });
    EXPECT_TRUE(std::fabs(got - lin) <= 1e-12 * std::fabs(lin));
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <tests/golden/mesh>\n", argv[0]); return 2; }
    MESH_PATH = argv[1];
    MeshLoader<2, 3> surface(MESH_PATH, "surface");   // (host side: CSV reading and the shape checks of Triangulation<2,3>)
    EXPECT_TRUE(surface.mesh.n_nodes() == 340 && surface.mesh.n_cells() == 616 && surface.points_.cols() == 3);
    if (fdapde_device_count() < 1) { std::printf("no HIP device: these tests have no CPU fallback\n"); return 3; }
    // the topology built on the device against the fixture's neigh.csv (MeshLoader realigns it to 0-based, -1 = none)
    const DMatrix<int>& nb = surface.mesh.neighbors();
    bool same = nb.rows() == surface.neighbors_.rows() && nb.cols() == surface.neighbors_.cols();
    for (int64_t i = 0; same && i < nb.size(); ++i) same = nb.data()[i] == surface.neighbors_.data()[i];
    EXPECT_TRUE(same);
    EXPECT_TRUE(surface.mesh.n_edges() == surface.edges_.rows());
    surface_laplace_beltrami<1>(surface.mesh);
    surface_laplace_beltrami<2>(surface.mesh);
    surface_diffusion_advection<1>(surface.mesh);
    surface_diffusion_advection<2>(surface.mesh);
    surface_integral<1>(surface.mesh);
    surface_integral<2>(surface.mesh);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
