// eng_handle.h -- what the operator handles that bring their own matrix share (the 2 x 2 block handle, eng_block.hip, and the Kronecker-sum handle,
// eng_kron.hip): the buffers and the per-matrix state of a handle (HandleCore), the guards, and ONE solve driver (handle_solve) that owns the defaults of
// rtol / maxit, the dense stage with its rent-or-buy rule, the Krylov column loop, the multilevel stage's column loop and the ending of every path.  A
// handle brings its refusals, its words and a HandleOps of lambdas: staging, the Krylov operator, the dense build, the multilevel build and run.
#ifndef FDAPDE_ENG_HANDLE_H
#define FDAPDE_ENG_HANDLE_H

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <string>
#include <type_traits>
#include <vector>

#include "context.h"
#include "engine.h"
#include "eng_gmres.h"
#include "kernels_dense.h"

namespace fdapde_engine {

struct HandleCore {
    bool ready = false, symmetric = false;
    bool jacobi_ok = false;            // every diagonal block was invertible (and D^-1 is there): the Krylov stage is available
    int64_t n = 0, nnz = 0;            // the space the handle was computed on
    DBuf<double> ext;                  // staging: the caller's blocks / factors / columns in the reference numbering
    DBuf<double> bt, x, r, w, t, sc, gm_V, gm_s, gm_part;
    DBuf<int32_t> ctl, flag;
    DBuf<int32_t> rowptr2, colidx2;    // the expanded CSR form (dense stage), built on first use
    DBuf<double> val2, dn_b, dn_x;
    bool expanded = false;
    fdapde_ctx::Dense dense;
    int64_t cols = 0;                  // columns solved against the current matrix
    double krylov_ms = 0;              // ... and the host time the Krylov columns among them took
    HandleGmresWork gmres_work() { return {bt, x, r, w, t, sc, gm_V, gm_s, gm_part, ctl}; }
};

// the texts of the answers both handles give, each handle's in its own words (whole literals: a message is found by searching for it)
struct HandleWords {
    const char *one_gpu, *compute_first, *methods, *dense_rows, *dense_singular;   // the guards, the method, DENSE by name above the limit / on a singular matrix
    const char *amg_broke, *amg_maxit;                                            // the multilevel stage's two endings without convergence
};

inline int handle_guard(fdapde_ctx* c, const HandleWords& w) {
    if (int rc = need_device(c)) return rc;
    if (c->comm != nullptr || c->ar_fn != nullptr || c->halo_ready || c->rd.ready)
        return fail(c, FDAPDE_EUNSUPPORTED, w.one_gpu);
    if (!c->dev_ready) return fail(c, FDAPDE_ENOTINIT, "call fdapde_dofs_build first");
    return FDAPDE_OK;
}
// the handle (NULL: never computed) belongs to the context's current space
inline int handle_live(fdapde_ctx* c, const HandleCore* h, const HandleWords& w) {
    if (!h || !h->ready || h->n != c->hs.n_dofs || h->nnz != c->hs.nnz) return fail(c, FDAPDE_ENOTINIT, w.compute_first);
    return FDAPDE_OK;
}
// what a change of the matrix invalidates here: the dense inverse, the expanded matrix, the rent-or-buy count (the multilevel hierarchy is the handle's to drop)
inline void handle_matrix_changed(HandleCore& h) { h.dense.ready = h.dense.failed = false, h.expanded = false, h.cols = 0, h.krylov_ms = 0; }

// how a column lies in the handle's vectors: D^-1 b in the internal order (the Krylov stage), b in the internal order (products, the multilevel stage), the
// order of the expanded matrix (the dense stage)
enum HandleLayout { kLayoutKrylov, kLayoutPlain, kLayoutDense };

// one call as its handle's refusals and the driver see it
struct HandleCall {
    int method;
    bool open, dense_named, amg, eligible;   // eligible: the dense inverse takes a system of this many rows
};
// the method of the call and the refusals every handle words alike (amg_method: the handle's multilevel stage, which has refusals of its own only)
inline int handle_call(fdapde_ctx* c, const HandleWords& w, int amg_method, int64_t rows, const fdapde_options* opt, HandleCall* k) {
    k->method = opt ? opt->method : FDAPDE_SOLVER_AUTO;
    k->open = k->method == FDAPDE_SOLVER_AUTO, k->dense_named = k->method == FDAPDE_SOLVER_DENSE, k->amg = k->method == amg_method;
    k->eligible = c->dense_rows > 0 && rows <= c->dense_rows && rows <= kDenseMaxRows;
    if (k->amg) return FDAPDE_OK;
    if (!k->open && !k->dense_named && k->method != FDAPDE_SOLVER_GMRES) return fail(c, FDAPDE_EUNSUPPORTED, w.methods);
    if (k->dense_named && !k->eligible) return fail(c, FDAPDE_EUNSUPPORTED, w.dense_rows);
    return FDAPDE_OK;
}

// the columns of one stage: iterations of all, FDAPDE_ENOCONV if one did not converge, the worst relres, a breakdown among those
struct HandleTally {
    int total = 0, rc_all = FDAPDE_OK;
    double worst = 0;
    bool broke = false;
};

// What a handle brings.  All launches go to the context's stream; ext is the handle's staging buffer.
//   stage(layout, ext, dst, ncols)    ncols stacked columns of the caller's, in ext, into dst under `layout`;  unstage(layout, src, ext, ncols) back
//   op(x, y, stop)                    the Krylov stage's operator (handle_gmres, eng_gmres.h)
//   dense_build()                     the inverse of the expanded matrix into the handle's `dense`
//   amg_build()                       the hierarchy of the current matrix, if it is not there yet
//   amg_run(b, x, rtol, maxit, &it, &rel, &conv, &broke)   one column against it (plain layout, on the device)
//   amg_batch(b, x, left, rtol, maxit, tally, &took)       nullptr, or: the next `took` of the `left` columns at the HOST addresses b, x side by side
//                                     (took = 0: none, the next column goes alone)
template <class Stage, class Unstage, class Op, class DenseBuild, class AmgBuild, class AmgRun, class AmgBatch> struct HandleOps {
    HandleWords words;
    int amg_method;
    int64_t rows, ext_words;   // words of a column; the staging buffer's size for this call
    Stage stage;
    Unstage unstage;
    Op op;
    DenseBuild dense_build;
    AmgBuild amg_build;
    AmgRun amg_run;
    AmgBatch amg_batch;
};
template <class... F> HandleOps(HandleWords, int, int64_t, int64_t, F...) -> HandleOps<F...>;

// One fdapde_*_solve behind its handle's guards and refusals (k: handle_call's reading of the call): n_rhs columns of ops.rows words, b and x on the host.
template <class Ops> int handle_solve(fdapde_ctx* c, HandleCore& H, const Ops& ops, const HandleCall& k, const fdapde_options* opt, const double* b, int32_t n_rhs,
                                      double* x, fdapde_info* info) {
    const int64_t rows = ops.rows;
    {   // an in-place solve: finished columns are written to x while later ones still read b
        const double *b0 = b, *b1 = b + (size_t)rows * n_rhs, *x0 = x, *x1 = x + (size_t)rows * n_rhs;
        if (b0 < x1 && x0 < b1) {
            std::vector<double> b_copy(b0, b1);
            return handle_solve(c, H, ops, k, opt, b_copy.data(), n_rhs, x, info);
        }
    }
    hipStream_t st = c->stream;
    const double rtol = (opt && opt->rtol > 0) ? opt->rtol : 1e-10;
    const int maxit = (opt && opt->maxit > 0) ? opt->maxit : (k.amg ? 200 : 2000);
    const auto t_call = std::chrono::steady_clock::now();
    auto ms_since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    if (k.amg)   // (a failed build still leaves the record of a call of this method)
        if (int rc = ops.amg_build()) return bare_answer(c, ops.amg_method, 0.0, info, rc);
    HIPCHK(c, H.ext.alloc((size_t)ops.ext_words));
    fdapde_info out{};
    if ((k.open || k.dense_named) && k.eligible) {   // the rent-or-buy rule of fdapde_lin_solve, with the handle's row count
        fdapde_ctx::Dense& D = H.dense;
        if (!D.ready && (!D.failed || k.dense_named) &&
            (k.dense_named || !H.jacobi_ok || c->dense_after == 0 || (H.cols + n_rhs > c->dense_after && H.krylov_ms >= 0.5 * dense_build_estimate_ms(rows))))
            if (int rc = ops.dense_build()) return rc;
        if ((k.dense_named || !H.jacobi_ok) && !D.ready)
            return c->err = dense_singular(ops.words.dense_singular), bare_answer(c, FDAPDE_SOLVER_DENSE, D.check, info, FDAPDE_ENOCONV);
        if (D.ready) {
            const size_t cnt = (size_t)rows * (size_t)n_rhs;
            HIPCHK(c, H.dn_b.alloc(cnt));
            HIPCHK(c, H.dn_x.alloc(cnt));
            // the columns cross in slices of the staging buffer's size, every slice one product
            const int per = (int)std::max<int64_t>(1, (int64_t)(H.ext.n / (size_t)rows));
            for (int j0 = 0; j0 < n_rhs; j0 += per) {
                const int nc = std::min(per, n_rhs - j0);
                HIPCHK(c, hipMemcpyAsync(H.ext.p, b + (size_t)j0 * rows, sizeof(double) * (size_t)rows * nc, hipMemcpyHostToDevice, st));
                ops.stage(kLayoutDense, H.ext.p, H.dn_b.p + (size_t)j0 * rows, nc);
            }
            if (int rc = dense_apply(c, D, n_rhs, H.dn_b.p, H.dn_x.p)) return rc;
            for (int j0 = 0; j0 < n_rhs; j0 += per) {
                const int nc = std::min(per, n_rhs - j0);
                ops.unstage(kLayoutDense, H.dn_x.p + (size_t)j0 * rows, H.ext.p, nc);
                HIPCHK(c, hipGetLastError());
                HIPCHK(c, hipMemcpyAsync(x + (size_t)j0 * rows, H.ext.p, sizeof(double) * (size_t)rows * nc, hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
            }
            H.cols += n_rhs;
            out.iters = D.refine ? 1 : 0, out.converged = 1, out.relres = D.check, out.method_used = FDAPDE_SOLVER_DENSE, out.t_solve_ms = ms_since();
            c->info = out;
            if (info) *info = out;
            return FDAPDE_OK;
        }
    }
    // the columns one after another: the Krylov stage on D^-1 A (its columns count towards the rent-or-buy rule), or the multilevel stage on the unscaled
    // system (they do not; a NaN residual is the worst there is)
    if (!k.amg) H.cols += n_rhs;
    const double tol2 = rtol * rtol;
    HandleTally t;
    for (int32_t j = 0; j < n_rhs; ++j) {
        const double* bj = b + (size_t)j * rows;
        double* xj = x + (size_t)j * rows;
        if constexpr (!std::is_null_pointer_v<decltype(ops.amg_batch)>) {
            int took = 0;
            if (k.amg)
                if (int rc = ops.amg_batch(bj, xj, n_rhs - j, rtol, maxit, t, &took)) return rc;
            if (took > 0) {
                j += took - 1;
                continue;
            }
        }
        HIPCHK(c, hipMemcpyAsync(H.ext.p, bj, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice, st));
        ops.stage(k.amg ? kLayoutPlain : kLayoutKrylov, H.ext.p, H.bt.p, 1);
        if (k.amg) {
            int it = 0;
            double rel = 0;
            bool conv = false, broke = false;
            if (int rc = ops.amg_run(H.bt.p, H.x.p, rtol, maxit, &it, &rel, &conv, &broke)) return rc;
            if (!conv) t.rc_all = FDAPDE_ENOCONV, t.broke = t.broke || broke;
            t.total += it, t.worst = rel > t.worst || std::isnan(rel) ? rel : t.worst;
        } else {
            int32_t h_ctl[4] = {0, 0, 0, 0};
            double h_sc[4] = {0, 0, 0, 0};
            if (int rc = handle_gmres(c, H.gmres_work(), rows, ops.op, tol2, maxit, h_ctl, h_sc)) return rc;
            const Outcome o = outcome_from(h_sc, h_ctl, tol2);
            if (!o.converged) t.rc_all = FDAPDE_ENOCONV, t.broke = t.broke || h_ctl[2] != 0;
            t.total += h_ctl[1], t.worst = o.relres > t.worst ? o.relres : t.worst;
        }
        ops.unstage(k.amg ? kLayoutPlain : kLayoutKrylov, H.x.p, H.ext.p, 1);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(xj, H.ext.p, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    const double ms = ms_since();
    if (!k.amg) H.krylov_ms += ms;
    out.iters = t.total, out.relres = t.worst, out.converged = t.rc_all == FDAPDE_OK ? 1 : 0, out.method_used = k.amg ? ops.amg_method : FDAPDE_SOLVER_GMRES;
    out.persistent = 0, out.t_solve_ms = ms;
    c->info = out;
    if (info) *info = out;
    if (t.rc_all == FDAPDE_ENOCONV) {
        if (k.amg) c->err = t.broke ? ops.words.amg_broke : ops.words.amg_maxit;
        else c->err = t.broke ? "GMRES stagnated or broke down in at least one column" : "maxit reached in at least one column";
    }
    return t.rc_all;
}

}   // namespace fdapde_engine
#endif
