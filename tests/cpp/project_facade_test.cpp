// project_facade_test.cpp -- Projection<Triangulation<2,3>> (include/fdapde_amd/project.h) and PDE::eval_basis_nearest on the reference's surface
// fixture against fdapde_project driven through the C ABI directly: projected points and distances <= 1e-12, the same cells, Psi with the
// identical pattern and values <= 1e-12, D = ones, no empty row.  The three call forms (points), (points, Exact), (points, NotExact) agree bit
// for bit.  Runs on a real MI355X (pytest -m gpu: tests/test_cpp_project.py, which also compiles it); without a device it refuses to run.
//
// usage: project_facade_test <path to tests/golden/mesh>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "fdapde_amd/io.h"
#include "fdapde_amd/pde.h"
#include "fdapde_amd/project.h"

using namespace fdapde::amd;

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                     \
    do {                                                                                                      \
        ++checks;                                                                                             \
        if (!(cond)) { ++failures; std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); }          \
    } while (0)

// measured locations near the surface: every cell's barycentre moved by +-0.02 along the cell's normal, and a lattice over the widened bounding box
static DMatrix<double> locations(const Triangulation<2, 3>& mesh) {
    const int64_t nc = mesh.n_cells();
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int64_t i = 0; i < mesh.n_nodes(); ++i)
        for (int d = 0; d < 3; ++d) lo[d] = std::fmin(lo[d], mesh.nodes()(i, d)), hi[d] = std::fmax(hi[d], mesh.nodes()(i, d));
    const int g = 5;
    DMatrix<double> p(nc + g * g * g, 3);
    for (int64_t c = 0; c < nc; ++c) {
        double a[3], b[3], bc[3];
        for (int d = 0; d < 3; ++d) {
            const double x0 = mesh.nodes()(mesh.cells()(c, 0), d), x1 = mesh.nodes()(mesh.cells()(c, 1), d), x2 = mesh.nodes()(mesh.cells()(c, 2), d);
            a[d] = x1 - x0, b[d] = x2 - x0, bc[d] = (x0 + x1 + x2) / 3.0;
        }
        const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), s = (c % 2 ? -0.02 : 0.02) / len;
        for (int d = 0; d < 3; ++d) p(c, d) = bc[d] + s * n[d];
    }
    int64_t r = nc;
    for (int i = 0; i < g; ++i)
        for (int j = 0; j < g; ++j)
            for (int k = 0; k < g; ++k, ++r) {
                const int idx[3] = {i, j, k};
                for (int d = 0; d < 3; ++d) p(r, d) = lo[d] - 0.25 * (hi[d] - lo[d]) + 1.5 * (hi[d] - lo[d]) * (idx[d] + 0.37) / g;
            }
    return p;
}

struct AbiResult {
    std::vector<int32_t> cell, dofs;
    std::vector<double> q, dist, val;
    int32_t nb = 0;
    int64_t nd = 0;
    bool ok = false;
};

template <int R> static AbiResult abi_project(const Triangulation<2, 3>& mesh, const DMatrix<double>& pts) {
    AbiResult out;
    fdapde_ctx* ctx = nullptr;
    if (fdapde_ctx_create(0, &ctx) != FDAPDE_OK) return out;
    const int64_t nn = mesh.n_nodes(), nc = mesh.n_cells(), n = pts.rows();
    std::vector<int32_t> cells((size_t)(nc * 3));
    std::vector<uint8_t> bnd((size_t)nn);
    for (int64_t c = 0; c < nc; ++c)
        for (int v = 0; v < 3; ++v) cells[(size_t)(c * 3 + v)] = mesh.cells()(c, v);
    for (int64_t i = 0; i < nn; ++i) bnd[(size_t)i] = mesh.boundary_nodes()(i, 0) ? 1 : 0;
    int64_t nnz = 0, ne = 0;
    int32_t nq = 0;
    bool ok = fdapde_mesh_upload(ctx, 2, 3, nn, mesh.nodes().data(), nc, cells.data(), bnd.data()) == FDAPDE_OK &&
              fdapde_dofs_build(ctx, R, &out.nd) == FDAPDE_OK && fdapde_sizes(ctx, &out.nd, &nnz, &out.nb, &nq, &ne) == FDAPDE_OK;
    if (ok) {
        out.cell.resize((size_t)n), out.q.resize((size_t)(3 * n)), out.dist.resize((size_t)n), out.val.resize((size_t)(n * out.nb));
        out.dofs.resize((size_t)(nc * out.nb));
        ok = fdapde_project(ctx, n, pts.data(), out.cell.data(), out.q.data(), out.dist.data(), out.val.data()) == FDAPDE_OK &&
             fdapde_dofs_get(ctx, out.dofs.data(), nullptr, nullptr) == FDAPDE_OK;
    }
    if (!ok) std::printf("  C ABI path: %s\n", fdapde_last_error(ctx));
    fdapde_ctx_destroy(ctx);
    out.ok = ok;
    return out;
}

static bool same_bits(const DMatrix<double>& a, const DMatrix<double>& b) {
    return a.rows() == b.rows() && a.cols() == b.cols() && std::equal(a.data(), a.data() + a.size(), b.data());
}

static void projection(const Triangulation<2, 3>& mesh, const DMatrix<double>& pts, const AbiResult& ref) {
    Projection<Triangulation<2, 3>> project(mesh);
    const DMatrix<double> q0 = project(pts), q1 = project(pts, Exact), q2 = project(pts, NotExact);
    EXPECT_TRUE(same_bits(q0, q1) && same_bits(q0, q2));
    const auto all = project.nearest(pts);
    EXPECT_TRUE(same_bits(q0, all.points));
    EXPECT_TRUE(q0.rows() == pts.rows() && q0.cols() == 3);
    double dq = 0, dd = 0;
    bool cells = true;
    for (int64_t i = 0; i < pts.rows(); ++i) {
        for (int d = 0; d < 3; ++d) dq = std::fmax(dq, std::fabs(q0(i, d) - ref.q[(size_t)(d * pts.rows() + i)]));
        dd = std::fmax(dd, std::fabs(all.distances(i) - ref.dist[(size_t)i]));
        cells = cells && all.cells(i) == ref.cell[(size_t)i];
    }
    std::printf("  Projection against the C ABI: points %.3e, distances %.3e\n", dq, dd);
    EXPECT_TRUE(dq <= 1e-12 && dd <= 1e-12 && cells);
    Projection<Triangulation<2, 3>> copy = project;   // (a copy shares the context built by the first call)
    EXPECT_TRUE(same_bits(copy(pts), q0));
}

template <int R> static void basis_at_nearest(const Triangulation<2, 3>& mesh, const DMatrix<double>& pts) {
    const AbiResult ref = abi_project<R>(mesh, pts);
    EXPECT_TRUE(ref.ok);
    if (!ref.ok) return;
    if (R == 1) projection(mesh, pts, ref);
    auto L = -laplacian<FEM_HIP>();
    PDE<Triangulation<2, 3>, decltype(L), DMatrix<double>, FEM_HIP, fem_order<R>> pde(mesh, L, DMatrix<double> {});
    DMatrix<double> projected;
    const EvalReturnType e = pde.eval_basis_nearest(pts, &projected);
    const int64_t n = pts.rows();
    EXPECT_TRUE(e.Psi.rows() == n && e.Psi.cols() == pde.n_dofs() && e.D.rows() == n && projected.rows() == n && projected.cols() == 3);
    bool pattern = true, ones = true, none_empty = true;
    double dv = 0, dq = 0, rowsum = 0;
    for (int64_t i = 0; i < n; ++i) {
        std::vector<std::pair<int32_t, double>> row;
        for (int32_t h = 0; h < ref.nb; ++h) row.push_back({ref.dofs[(size_t)(ref.cell[(size_t)i] * ref.nb + h)], ref.val[(size_t)(i * ref.nb + h)]});
        std::sort(row.begin(), row.end());
        const int32_t k0 = e.Psi.rowptr[(size_t)i], k1 = e.Psi.rowptr[(size_t)i + 1];
        none_empty = none_empty && k1 > k0;
        pattern = pattern && k1 - k0 == (int32_t)row.size();
        double s = 0;
        for (int32_t k = k0; pattern && k < k1; ++k) {
            pattern = e.Psi.colidx[(size_t)k] == row[(size_t)(k - k0)].first;
            dv = std::fmax(dv, std::fabs(e.Psi.values[(size_t)k] - row[(size_t)(k - k0)].second));
            s += e.Psi.values[(size_t)k];
        }
        rowsum = std::fmax(rowsum, std::fabs(s - 1.0));
        ones = ones && e.D(i) == 1.0;
        for (int d = 0; d < 3; ++d) dq = std::fmax(dq, std::fabs(projected(i, d) - ref.q[(size_t)(d * n + i)]));
    }
    std::printf("  P%d: eval_basis_nearest against the C ABI: values %.3e, projected %.3e, row sums - 1 %.3e\n", R, dv, dq, rowsum);
    EXPECT_TRUE(pattern && ones && none_empty);
    EXPECT_TRUE(dv <= 1e-12 && dq <= 1e-12 && rowsum <= 1e-13);
    // eval_basis (point location) still refuses a surface
    bool refused = false;
    try {
        (void)pde.eval_basis(0, pts);
    } catch (const std::runtime_error& err) { refused = std::string(err.what()).find("surface") != std::string::npos; }
    EXPECT_TRUE(refused);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <tests/golden/mesh>\n", argv[0]); return 2; }
    MeshLoader<2, 3> surface(argv[1], "surface");
    EXPECT_TRUE(surface.mesh.n_nodes() == 340 && surface.mesh.n_cells() == 616);
    if (fdapde_device_count() < 1) { std::printf("no HIP device: these tests have no CPU fallback\n"); return 3; }
    const DMatrix<double> pts = locations(surface.mesh);
    basis_at_nearest<1>(surface.mesh, pts);
    basis_at_nearest<2>(surface.mesh, pts);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
