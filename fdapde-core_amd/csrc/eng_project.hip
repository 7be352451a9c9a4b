// eng_project.hip -- fdapde_project: every point onto its nearest cell (Projection<Triangulation>, geometry/project.h), the projection, the
// distance and the basis values there (kernels_project.h).  Shares the bin grid and the staging buffers of fdapde_eval_pointwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "context.h"
#include "dev_setup.h"
#include "engine.h"
#include "kernels_project.h"

namespace fdapde_engine {

int e_project(fdapde_ctx* c, int64_t n_pts, const double* pts_colmajor, int32_t* cell_ids, double* proj_colmajor, double* dist, double* values) {
    if (!c || n_pts < 1 || !pts_colmajor || !cell_ids || !proj_colmajor || !dist) return FDAPDE_EINVAL;   // (values may be NULL)
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready) return fail(c, FDAPDE_ENOTINIT, "call fdapde_dofs_build first");
    const HostSpace& hs = c->hs;
    const int M = hs.M, N = hs.N;
    for (int64_t k = 0; k < n_pts * N; ++k)
        if (!std::isfinite(pts_colmajor[k])) {
            c->err = "fdapde_project: point " + std::to_string(k % n_pts) + " has a non-finite coordinate (axis " + std::to_string(k / n_pts) + ")";
            return FDAPDE_EINVAL;
        }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (int rc = ensure_eval_grid(c)) return rc;
    fdapde_ctx::EvalGrid& eg = c->eval_grid;
    HIPCHK(c, c->eval_locs.upload(pts_colmajor, (size_t)n_pts * N, st));
    HIPCHK(c, c->eval_out.alloc((size_t)n_pts));
    HIPCHK(c, c->proj_q.alloc((size_t)n_pts * N));
    HIPCHK(c, c->proj_d.alloc((size_t)n_pts));
    if (values) HIPCHK(c, c->eval_vals.alloc((size_t)n_pts * hs.nb));
    AsmArgs a{};   // (the kernel reads the cells' vertices and their coordinates only)
    a.n_dofs = hs.n_dofs, a.n_cells = hs.n_cells, a.cverts = c->cverts.p, a.vcoords = c->vcoords.p;
    const dim3 grid(g1(n_pts)), block(256);
    double* d_vals = values ? c->eval_vals.p : nullptr;
    static const bool timed = std::getenv("FDAPDE_DEBUG_TIMING") != nullptr;   // (the kernel alone, on stderr: tools/project_time.py reads it)
    if (timed) HIPCHK(c, hipEventRecord(c->ev0, st));
#define PROJECT_GO(MM, RR, NN)                                                                                                                     \
    hipLaunchKernelGGL((k_project<MM, RR, NN>), grid, block, 0, st, a, n_pts, c->eval_locs.p, eg.lo.p, eg.invh.p, eg.dims.p, eg.ptr.p, eg.cells.p, \
                       c->cell_i2e.p, c->eval_out.p, c->proj_q.p, c->proj_d.p, d_vals)
#define PROJECT_ORDER(MM, NN)                    \
    do {                                         \
        if (hs.order == 1) PROJECT_GO(MM, 1, NN); \
        else PROJECT_GO(MM, 2, NN);              \
    } while (0)
    if (M == 1 && N == 1) PROJECT_ORDER(1, 1);
    else if (M == 1 && N == 2) PROJECT_ORDER(1, 2);
    else if (M == 2 && N == 2) PROJECT_ORDER(2, 2);
    else if (M == 2 && N == 3) PROJECT_ORDER(2, 3);
    else if (M == 3 && N == 3) PROJECT_ORDER(3, 3);
    else return fail(c, FDAPDE_EUNSUPPORTED, "fdapde_project: this (M, N) has no projection kernel");
#undef PROJECT_ORDER
#undef PROJECT_GO
    HIPCHK(c, hipGetLastError());
    if (timed) {
        float ms = 0;
        HIPCHK(c, hipEventRecord(c->ev1, st));
        HIPCHK(c, hipEventSynchronize(c->ev1));
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        std::fprintf(stderr, "[timing] %-34s %8.3f ms\n", "k_project", (double)ms);
    }
    HIPCHK(c, hipMemcpyAsync(cell_ids, c->eval_out.p, sizeof(int32_t) * (size_t)n_pts, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(proj_colmajor, c->proj_q.p, sizeof(double) * (size_t)n_pts * N, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(dist, c->proj_d.p, sizeof(double) * (size_t)n_pts, hipMemcpyDeviceToHost, st));
    if (values) HIPCHK(c, hipMemcpyAsync(values, c->eval_vals.p, sizeof(double) * (size_t)n_pts * hs.nb, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDAPDE_OK;
}

}   // namespace fdapde_engine
