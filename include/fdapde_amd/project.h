// project.h -- Projection<Triangulation<M,N>> (fdaPDE/geometry/project.h): points onto the mesh, through fdapde_project on MI355X.
//
//   Projection<Triangulation<2, 3>> project(mesh);
//   DMatrix<double> q = project(points);            // n_points x N: the closest point of the mesh to every row of `points`
//   q = project(points, Exact);  q = project(points, NotExact);
//
// The reference has two algorithms: Exact scans every cell, NotExact (its default) looks only at the cells around the nearest NODE, which
// can miss the nearest cell.  Here all three call forms give the exact answer of the device search (a global nearest-cell search over a bin
// grid: include/fdapde_hip.h fdapde_project), and the closest point of a cell is the true one, not Simplex::nearest's (simplex.h:156-181:
// drop the farthest vertex and recurse), which is off on obtuse cells.  nearest() also returns the cells and the distances.
// The device context (mesh upload + order-1 space) is created by the first call, as the reference builds its KD-tree lazily, and is shared by
// copies of the object.  Header-only; C++20.
#ifndef FDAPDE_AMD_PROJECT_H
#define FDAPDE_AMD_PROJECT_H

#include "pde.h"

namespace fdapde {
namespace amd {

struct tag_exact { };
struct tag_not_exact { };
inline constexpr tag_exact Exact {};
inline constexpr tag_not_exact NotExact {};

template <typename TriangulationType> class Projection {
   public:
    static constexpr int M = TriangulationType::local_dim, N = TriangulationType::embed_dim;
    struct Nearest {
        DMatrix<double> points;       // n_points x N: the projections
        DMatrix<int> cells;           // n_points x 1: the nearest cell of every point
        DVector<double> distances;    // n_points x 1
    };
    Projection() = default;
    explicit Projection(const TriangulationType& mesh, int device = 0) : mesh_(&mesh), device_(device) { }

    DMatrix<double> operator()(const DMatrix<double>& points, tag_exact) const { return nearest(points).points; }
    DMatrix<double> operator()(const DMatrix<double>& points, tag_not_exact) const { return nearest(points).points; }
    DMatrix<double> operator()(const DMatrix<double>& points) const { return nearest(points).points; }

    Nearest nearest(const DMatrix<double>& points) const {
        if (!mesh_) throw std::runtime_error("Projection: no mesh");
        if (points.cols() != N) throw std::runtime_error("Projection: points must have one column per coordinate of the mesh");
        fdapde_ctx* const ctx = context();
        const int64_t n = points.rows();
        Nearest out {DMatrix<double>(n, N), DMatrix<int>(n, 1), DVector<double>(n, 1)};
        std::vector<int32_t> cell((size_t)n);
        const int rc = fdapde_project(ctx, n, points.data(), cell.data(), out.points.data(), out.distances.data(), nullptr);
        if (rc != FDAPDE_OK) {
            const std::string msg = fdapde_last_error(ctx);
            throw std::runtime_error(msg.empty() ? fdapde_status_string(rc) : msg);
        }
        for (int64_t i = 0; i < n; ++i) out.cells(i) = cell[(size_t)i];
        return out;
    }

   private:
    struct Owner {
        fdapde_ctx* ctx = nullptr;
        ~Owner() {
            if (ctx) fdapde_ctx_destroy(ctx);
        }
    };
    fdapde_ctx* context() const {
        if (owner_ && owner_->ctx) return owner_->ctx;
        auto o = std::make_shared<Owner>();
        if (fdapde_ctx_create(device_, &o->ctx) != FDAPDE_OK) throw std::runtime_error("Projection: no HIP device (there is no CPU fallback)");
        const int64_t nn = mesh_->n_nodes(), nc = mesh_->n_cells();
        std::vector<int32_t> cells((size_t)(nc * (M + 1)));
        std::vector<uint8_t> bnd((size_t)nn);
        for (int64_t c = 0; c < nc; ++c)
            for (int v = 0; v <= M; ++v) cells[(size_t)(c * (M + 1) + v)] = mesh_->cells()(c, v);
        for (int64_t i = 0; i < nn; ++i) bnd[(size_t)i] = mesh_->boundary_nodes()(i, 0) ? 1 : 0;
        int64_t nd = 0;
        if (fdapde_mesh_upload(o->ctx, M, N, nn, mesh_->nodes().data(), nc, cells.data(), bnd.data()) != FDAPDE_OK ||
            fdapde_dofs_build(o->ctx, 1, &nd) != FDAPDE_OK)
            throw std::runtime_error(std::string("Projection: ") + fdapde_last_error(o->ctx));
        owner_ = o;
        return owner_->ctx;
    }
    const TriangulationType* mesh_ = nullptr;   // must outlive the object (project.h:28)
    int device_ = 0;
    mutable std::shared_ptr<Owner> owner_;      // built by the first call (project.h:29: the KD-tree)
};

}   // namespace amd
}   // namespace fdapde
#endif
