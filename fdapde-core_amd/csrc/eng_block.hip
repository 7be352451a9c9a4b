// eng_block.hip -- the 2 x 2 block handle: fdapde::SparseLU on a SparseBlockMatrix<double,2,2> whose four blocks lie on the FEM pattern (the
// smoothing system the downstream models factor once and solve for many columns: fdaPDE/linear_algebra/sparse_block_matrix.h:29-128,
// utils/symbols.h:133-160, linear_algebra/smw.h:38-59), and Psi^T W Psi on that pattern (kernels_block.h).
//   fdapde_block_compute   blocks -> block CSR in the internal order, D^-1 A folded into a second copy (left block-Jacobi)
//   fdapde_block_solve     restarted GMRES(m) on D^-1 A (kernels_gmres.h, buffers of the handle's own), or the dense inverse of the 2 n-row matrix, or
//                          (by name) flexible GMRES around the point-block multilevel cycle of eng_block_amg.hip.  The stages, the column loops and the
//                          ending are handle_solve's (eng_handle.h, shared with eng_kron.hip); here: the refusals and block_ops -- staging, operator, builds
//   fdapde_block_spmv      y = A x with the unscaled blocks
//   fdapde_gram_pointwise  Psi^T W Psi from what fdapde_eval_pointwise / fdapde_project hand out
//   fdapde_block_set_obs   the data term kept factored: the handle's matrix becomes A + scale [Psi^T W Psi, 0; 0, 0] with Psi a CSR matrix of any row length
//                          (areal designs: Psi^T Psi is far off the pattern); set-up in host_obs.cpp, the two products per application in kernels_obs.h
// Independent of the n x n handle of fdapde_lin_compute: nothing here writes a buffer one of the other solves reads back.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "amg_setup.h"
#include "context.h"
#include "engine.h"
#include "eng_handle.h"
#include "host_obs.h"
#include "kernels_block.h"
#include "kernels_dense.h"
#include "kernels_gmres.h"
#include "kernels_krylov.h"
#include "kernels_obs.h"

namespace fdapde_engine {

// the factored data term of the current matrix (fdapde_block_set_obs): Psi and Psi^T in the internal order on the device, the host copy for the dense stage
struct BlockObs {
    bool live = false;
    double scale = 0;
    int team_rows = 8, team_cols = 8;   // lanes per row of Psi (k_obs_gather) / of Psi^T (k_obs_scatter, k_obs_diag)
    int team_knob = 0;                  // the knob block_obs_team they were chosen under
    fdapde_hip::ObsHost host;
    DBuf<int32_t> rp, ci, trp, tci;
    DBuf<double> v, tv, w, t, g;        // t [n_obs]: W Psi x_1 between the two products; g [n]: the term's share of every diagonal block
};

struct BlockHandle : HandleCore {      // (the vectors at 2 n words, ext at least max(4 nnz, 2 n), the dense stage on 2 n rows)
    DBuf<double> raw, scaled, dinv;    // [4 nnz] unscaled / D^-1-scaled values, [4 n] the inverted diagonal blocks
    bool given[4] = {false, false, false, false};   // which of a11 a12 a21 a22 were handed over (not NULL)
    BlockAmg* amg = nullptr;           // FDAPDE_SOLVER_BLOCK_AMG's hierarchy of the current matrix (eng_block_amg.hip), built by its first solve
    BlockObs obs;
    ~BlockHandle() { block_amg_free(amg); }
};

void block_release(fdapde_ctx* c) {
    if (!c->block) return;
    if (c->has_device) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    delete c->block;
    c->block = nullptr;
}

void block_amg_forget(fdapde_ctx* c) {
    if (!c->block || !c->block->amg) return;
    if (c->has_device) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    block_amg_free(c->block->amg), c->block->amg = nullptr;
}
// fdapde_amg_hierarchy / _cols_trace / _aggregates / _order / _damping, which 2: the answers of eng_amg.hip on the hierarchy's base (rows 2 n_l, entries 4 nnz_l: per = 2)
static const AmgHierarchy* block_hierarchy(const fdapde_ctx* c) { return c->block ? c->block->amg : nullptr; }
int block_amg_describe_ctx(const fdapde_ctx* c, int32_t cap, int32_t* n_levels, int64_t* rows, int64_t* nnz, int32_t* absorbed, double* setup_ms) {
    return amg_describe(block_hierarchy(c), cap, n_levels, rows, nnz, absorbed, setup_ms);
}
int block_amg_cols_trace_ctx(const fdapde_ctx* c, int32_t* batches, int32_t* batched_cols, int32_t* single_cols) {
    return amg_cols_trace(block_hierarchy(c), batches, batched_cols, single_cols);
}
int block_amg_aggregates_ctx(fdapde_ctx* c, int32_t level, int64_t cap, int32_t* agg, int64_t* n_rows) { return amg_aggregates(c, block_hierarchy(c), level, cap, agg, n_rows); }
int block_amg_order_ctx(fdapde_ctx* c, int64_t cap, int32_t* order, int64_t* n_rows) { return amg_order(c, block_hierarchy(c), cap, order, n_rows); }
int block_amg_damping_ctx(const fdapde_ctx* c, int32_t cap, int32_t* n_levels, double* omega) { return amg_damping(block_hierarchy(c), cap, n_levels, omega); }

namespace {

constexpr HandleWords kBlockWords{
    "the 2 x 2 block handle takes one-GPU contexts, not a rank of a multi-GPU job",
    "call fdapde_block_compute first",
    "fdapde_block_solve runs FDAPDE_SOLVER_GMRES, FDAPDE_SOLVER_DENSE, FDAPDE_SOLVER_BLOCK_AMG or the open method",
    "FDAPDE_SOLVER_DENSE takes block systems of up to `dense_rows` (at most 8192) rows",
    "the block matrix",   // (dense_singular's `what`)
    "FDAPDE_SOLVER_BLOCK_AMG: the flexible GMRES broke down in at least one column",
    "FDAPDE_SOLVER_BLOCK_AMG: maxit reached in at least one column"};

void launch_block_spmv(fdapde_ctx* c, const double* vals, const double* x, double* y, const int32_t* stop) {
    const int64_t n = c->hs.n_dofs;
    constexpr int T = kBlockTeam;
    hipLaunchKernelGGL(k_block_spmv<T>, dim3(g1(n, 256 / T)), dim3(256), 0, c->stream, n, c->rowptr.p, c->colidx.p, vals, x, y, stop);
}

// y += D^-1 [scale Psi^T W Psi x_1; 0] (dinv = NULL: without D^-1) behind a launch_block_spmv that wrote y: two launches, team widths as chosen per matrix
void launch_obs_term(fdapde_ctx* c, BlockHandle& B, const double* dinv, const double* x, double* y, const int32_t* stop) {
    BlockObs& O = B.obs;
    const int64_t m = O.host.n_obs, n = B.n;
    hipStream_t st = c->stream;
    if (O.team_rows == 64) hipLaunchKernelGGL(k_obs_gather<64>, dim3(g1(m, 4)), dim3(256), 0, st, m, O.rp.p, O.ci.p, O.v.p, O.w.p, x, O.t.p, stop);
    else hipLaunchKernelGGL(k_obs_gather<8>, dim3(g1(m, 32)), dim3(256), 0, st, m, O.rp.p, O.ci.p, O.v.p, O.w.p, x, O.t.p, stop);
    if (O.team_cols == 64) hipLaunchKernelGGL(k_obs_scatter<64>, dim3(g1(n, 4)), dim3(256), 0, st, n, O.trp.p, O.tci.p, O.tv.p, O.t.p, O.scale, dinv, y, stop);
    else hipLaunchKernelGGL(k_obs_scatter<8>, dim3(g1(n, 32)), dim3(256), 0, st, n, O.trp.p, O.tci.p, O.tv.p, O.t.p, O.scale, dinv, y, stop);
}

// the Krylov stage's operator D^-1 (A + the term): one launch without a term, three with one
void launch_block_op(fdapde_ctx* c, BlockHandle& B, const double* x, double* y, const int32_t* stop) {
    launch_block_spmv(c, B.scaled.p, x, y, stop);
    if (B.obs.live) launch_obs_term(c, B, B.dinv.p, x, y, stop);
}

// D^-1 of every DOF (g: the data term's share of the (1,1) entries, or NULL), the singular-block flag and the scaled copy, from `raw`
int block_rescale(fdapde_ctx* c, BlockHandle& B, const double* g) {
    hipStream_t st = c->stream;
    const int64_t n = B.n;
    HIPCHK(c, hipMemsetAsync(B.flag.p, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_block_diag_inv, dim3(g1(n)), dim3(256), 0, st, n, c->rowptr.p, c->colidx.p, B.raw.p, g, B.dinv.p, B.flag.p);
    hipLaunchKernelGGL(k_block_scale, dim3(g1(n, 256 / kBlockTeam)), dim3(256), 0, st, n, c->rowptr.p, B.raw.p, B.dinv.p, B.scaled.p);
    HIPCHK(c, hipGetLastError());
    int32_t h_flag = 0;
    HIPCHK(c, hipMemcpyAsync(&h_flag, B.flag.p, sizeof h_flag, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    B.jacobi_ok = h_flag == 0;
    return FDAPDE_OK;
}

int block_dense_build(fdapde_ctx* c, BlockHandle& B) {
    const int64_t n = B.n;
    if (B.obs.live) {   // the term merged into the expanded matrix by the host (set-up): build and refinement see the true matrix
        hipStream_t st = c->stream;
        if (int rc = ensure_host(c, kHostPattern)) return rc;
        std::vector<double> raw((size_t)(4 * B.nnz));
        HIPCHK(c, hipMemcpyAsync(raw.data(), B.raw.p, sizeof(double) * raw.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        std::vector<int32_t> rp2, ci2;
        std::vector<double> v2;
        fdapde_hip::obs_merge_dense(c->hs.rowptr_i.data(), c->hs.colidx_i.data(), raw.data(), B.obs.host, B.obs.scale, &rp2, &ci2, &v2);
        B.expanded = false;   // (the buffers hold the merged matrix, not k_block_expand's)
        HIPCHK(c, B.rowptr2.upload(rp2.data(), rp2.size(), st));
        HIPCHK(c, B.colidx2.upload(ci2.data(), ci2.size(), st));
        HIPCHK(c, B.val2.upload(v2.data(), v2.size(), st));
        HIPCHK(c, hipStreamSynchronize(st));   // (the host vectors have been read)
        return dense_build_csr(c, 2 * n, B.rowptr2.p, B.colidx2.p, B.val2.p, nullptr, 0, B.dense);
    }
    if (!B.expanded) {
        HIPCHK(c, B.rowptr2.alloc((size_t)(2 * n + 1)));
        HIPCHK(c, B.colidx2.alloc((size_t)(4 * B.nnz)));
        HIPCHK(c, B.val2.alloc((size_t)(4 * B.nnz)));
        hipLaunchKernelGGL(k_block_expand, dim3(g1(n + 1)), dim3(256), 0, c->stream, n, c->rowptr.p, c->colidx.p, B.raw.p, B.rowptr2.p, B.colidx2.p, B.val2.p);
        HIPCHK(c, hipGetLastError());
        B.expanded = true;
    }
    return dense_build_csr(c, 2 * n, B.rowptr2.p, B.colidx2.p, B.val2.p, nullptr, 0, B.dense);
}

// what a change of the term invalidates: handle_matrix_changed's and the multilevel hierarchy
void block_matrix_changed(BlockHandle& B) {
    handle_matrix_changed(B);
    block_amg_free(B.amg), B.amg = nullptr;
}

// What handle_solve (eng_handle.h) and fdapde_block_spmv take from this handle.  Staging: one kernel under every layout -- D^-1 folded in for the Krylov stage,
// the dense stage's order is the internal one.  FDAPDE_SOLVER_BLOCK_AMG: the hierarchy built by the first such solve after fdapde_block_compute, the columns in
// batches side by side (knob amg_cols) on the UNSCALED system (stop rule: the true residual |b - A x| <= rtol |b| -- not the D^-1-scaled one of the GMRES stage)
auto block_ops(fdapde_ctx* c, BlockHandle& B) {
    const int64_t n = B.n, n2 = 2 * n;
    hipStream_t st = c->stream;
    return HandleOps{
        kBlockWords, FDAPDE_SOLVER_BLOCK_AMG, n2, std::max<int64_t>(4 * B.nnz, n2),
        [c, &B, n, st](HandleLayout layout, const double* ext, double* dst, int ncols) {
            hipLaunchKernelGGL(k_block_stage, dim3(g1(n), ncols), dim3(256), 0, st, n, c->dof_i2e.p, ext, layout == kLayoutKrylov ? B.dinv.p : nullptr, dst);
        },
        [c, n, st](HandleLayout, const double* src, double* ext, int ncols) {
            hipLaunchKernelGGL(k_block_unstage, dim3(g1(n), ncols), dim3(256), 0, st, n, c->dof_i2e.p, src, ext);
        },
        [c, &B](const double* x, double* y, const int32_t* stop) { launch_block_op(c, B, x, y, stop); },
        [c, &B] { return block_dense_build(c, B); },
        [c, &B] {
            if (B.amg) return (int)FDAPDE_OK;
            const int strength = B.given[2] ? 2 : B.given[1] ? 1 : B.given[3] ? 3 : 0;   // the (2,1) block, else (1,2), (2,2), (1,1)
            const BlockObs& O = B.obs;   // (live only under block_amg_obs = 1: the levels carry the term)
            const BlockAmgTerm term{&O.host, O.scale, O.team_rows, O.team_cols, O.team_knob, O.rp.p, O.ci.p, O.trp.p, O.tci.p, O.v.p, O.tv.p, O.w.p, O.g.p};
            return block_amg_build(c, &B.amg, B.raw.p, strength, O.live ? &term : nullptr);
        },
        [c, &B](const double* b, double* x, double rtol, int maxit, int* it, double* rel, bool* conv, bool* broke) {
            return block_amg_run(c, B.amg, B.raw.p, b, x, rtol, maxit, it, rel, conv, broke);
        },
        // batches of 8, then 4, then 2 columns side by side (knob amg_cols; one host <-> device copy per batch), a last single column as before
        [c, &B, n2, st](const double* b, double* x, int32_t left, double rtol, int maxit, HandleTally& t, int* took) -> int {
            const int Q = block_amg_width(c, B.amg, left, maxit);
            *took = Q > 1 ? Q : 0;
            if (Q == 1) return ++B.amg->single_cols, (int)FDAPDE_OK;
            const size_t cnt = (size_t)n2 * (size_t)Q;
            HIPCHK(c, hipMemcpyAsync(B.ext.p, b, sizeof(double) * cnt, hipMemcpyHostToDevice, st));
            bool not_conv = false;
            if (int rc = block_amg_batch(c, B.amg, B.raw.p, Q, B.ext.p, B.bt.p, B.x.p, rtol, maxit, &t.total, &t.worst, &not_conv, &t.broke)) return rc;
            if (not_conv) t.rc_all = FDAPDE_ENOCONV;
            HIPCHK(c, hipMemcpyAsync(x, B.ext.p, sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            return FDAPDE_OK;
        }};
}

}   // namespace

int e_block_compute(fdapde_ctx* c, const double* a11, const double* a12, const double* a21, const double* a22, int32_t symmetric) {
    if (!c) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kBlockWords)) return rc;
    if ((!a11 && !a12) || (!a21 && !a22)) return fail(c, FDAPDE_EINVAL, "fdapde_block_compute: a block row without a block (the matrix would be singular)");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const HostSpace& hs = c->hs;
    const int64_t n = hs.n_dofs, nnz = hs.nnz;
    if (!c->block) c->block = new BlockHandle();
    BlockHandle& B = *c->block;
    B.ready = false, B.n = n, B.nnz = nnz, B.symmetric = symmetric != 0;
    block_matrix_changed(B);                  // (the inverse and the hierarchy belonged to the previous matrix)
    B.obs.live = false;                       // (... and so did the data term)
    B.given[0] = a11 != nullptr, B.given[1] = a12 != nullptr, B.given[2] = a21 != nullptr, B.given[3] = a22 != nullptr;
    HIPCHK(c, B.ext.alloc((size_t)std::max<int64_t>(4 * nnz, 2 * n)));
    HIPCHK(c, B.raw.alloc((size_t)(4 * nnz)));
    HIPCHK(c, B.scaled.alloc((size_t)(4 * nnz)));
    HIPCHK(c, B.dinv.alloc((size_t)(4 * n)));
    HIPCHK(c, B.flag.alloc(1));
    HIPCHK(c, B.ctl.alloc(8));
    HIPCHK(c, B.sc.alloc(32));
    for (DBuf<double>* v : {&B.bt, &B.x, &B.r, &B.w, &B.t}) HIPCHK(c, v->alloc((size_t)(2 * n)));
    const double* blocks[4] = {a11, a12, a21, a22};
    for (int q = 0; q < 4; ++q) {
        if (blocks[q]) HIPCHK(c, hipMemcpyAsync(B.ext.p + (size_t)q * nnz, blocks[q], sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, st));
        else HIPCHK(c, hipMemsetAsync(B.ext.p + (size_t)q * nnz, 0, sizeof(double) * (size_t)nnz, st));
    }
    hipLaunchKernelGGL(k_block_pack, dim3(g1(nnz)), dim3(256), 0, st, nnz, c->slot_i2e.p, B.ext.p, B.raw.p);
    if (int rc = block_rescale(c, B, nullptr)) return rc;   // (synchronises: the caller's blocks have been read)
    B.ready = true;
    return FDAPDE_OK;
}

int e_block_set_obs(fdapde_ctx* c, int64_t n_obs, const int64_t* rowptr, const int32_t* colidx, const double* values, const double* weights, double scale) {
    if (!c) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kBlockWords)) return rc;
    if (int rc = handle_live(c, c->block, kBlockWords)) return rc;
    if (n_obs < 0) return fail(c, FDAPDE_EINVAL, "fdapde_block_set_obs: n_obs is negative");
    HIPCHK(c, hipSetDevice(c->device));
    BlockHandle& B = *c->block;
    BlockObs& O = B.obs;
    hipStream_t st = c->stream;
    const int64_t n = B.n;
    if (n_obs == 0 || !rowptr) {   // clears the term
        if (!O.live) return FDAPDE_OK;
        HIPCHK(c, hipStreamSynchronize(st));
        O.live = false;
        block_matrix_changed(B);
        return block_rescale(c, B, nullptr);
    }
    std::string why;
    if (!fdapde_hip::obs_validate(n, n_obs, rowptr, colidx, values, weights, scale, &why)) {   // (nothing launched, the previous term stays)
        c->err = why;
        return FDAPDE_EINVAL;
    }
    if (int rc = ensure_host(c, kHostPerm)) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    fdapde_hip::ObsHost& P = O.host;
    O.live = false;
    block_matrix_changed(B);
    fdapde_hip::obs_build(n, n_obs, rowptr, colidx, values, weights, c->hs.dof_e2i.data(), &P);
    O.scale = scale;
    O.team_knob = c->block_obs_team;
    O.team_rows = fdapde_hip::obs_team_width(P.n_obs, P.nnz, c->block_obs_team);
    O.team_cols = fdapde_hip::obs_team_width(P.n, P.nnz, c->block_obs_team);
    HIPCHK(c, O.rp.upload(P.rp.data(), P.rp.size(), st));
    HIPCHK(c, O.ci.upload(P.ci.data(), P.ci.size(), st));
    HIPCHK(c, O.v.upload(P.v.data(), P.v.size(), st));
    HIPCHK(c, O.trp.upload(P.trp.data(), P.trp.size(), st));
    HIPCHK(c, O.tci.upload(P.tci.data(), P.tci.size(), st));
    HIPCHK(c, O.tv.upload(P.tv.data(), P.tv.size(), st));
    HIPCHK(c, O.w.upload(P.w.data(), P.w.size(), st));
    HIPCHK(c, O.t.alloc((size_t)n_obs));
    HIPCHK(c, O.g.alloc((size_t)n));
    if (O.team_cols == 64) hipLaunchKernelGGL(k_obs_diag<64>, dim3(g1(n, 4)), dim3(256), 0, st, n, O.trp.p, O.tci.p, O.tv.p, O.w.p, scale, O.g.p, (const int32_t*)nullptr);
    else hipLaunchKernelGGL(k_obs_diag<8>, dim3(g1(n, 32)), dim3(256), 0, st, n, O.trp.p, O.tci.p, O.tv.p, O.w.p, scale, O.g.p, (const int32_t*)nullptr);
    if (int rc = block_rescale(c, B, O.g.p)) return rc;   // (synchronises: the uploads are done)
    O.live = true;
    return FDAPDE_OK;
}

int e_block_obs_info(fdapde_ctx* c, int64_t* n_obs, int64_t* nnz, int32_t* team_rows, int32_t* team_cols) {
    if (!c) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kBlockWords)) return rc;
    if (int rc = handle_live(c, c->block, kBlockWords)) return rc;
    const BlockObs& O = c->block->obs;
    if (!O.live) return fail(c, FDAPDE_ENOTINIT, "fdapde_block_obs_info: no data term is live (fdapde_block_set_obs)");
    if (n_obs) *n_obs = O.host.n_obs;
    if (nnz) *nnz = O.host.nnz;
    if (team_rows) *team_rows = O.team_rows;
    if (team_cols) *team_cols = O.team_cols;
    return FDAPDE_OK;
}

int e_block_amg_obs_levels(fdapde_ctx* c, int32_t cap, int32_t* n_levels, int64_t* nnz, int32_t* longest_row, int32_t* team_rows, int32_t* team_cols) {
    if (!c) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kBlockWords)) return rc;
    if (int rc = handle_live(c, c->block, kBlockWords)) return rc;
    if (!block_amg_has_term(c->block->amg))
        return fail(c, FDAPDE_ENOTINIT, "fdapde_block_obs_amg_levels: no live hierarchy carries a data term (knob block_amg_obs, fdapde_block_set_obs, a FDAPDE_SOLVER_BLOCK_AMG solve)");
    return block_amg_obs_levels(c->block->amg, cap, n_levels, nnz, longest_row, team_rows, team_cols, nullptr);
}

int e_block_spmv(fdapde_ctx* c, const double* x, double* y) {
    if (!c || !x || !y) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kBlockWords)) return rc;
    if (int rc = handle_live(c, c->block, kBlockWords)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    BlockHandle& B = *c->block;
    hipStream_t st = c->stream;
    const auto ops = block_ops(c, B);
    HIPCHK(c, hipMemcpyAsync(B.ext.p, x, sizeof(double) * (size_t)ops.rows, hipMemcpyHostToDevice, st));
    ops.stage(kLayoutPlain, B.ext.p, B.w.p, 1);
    launch_block_spmv(c, B.raw.p, B.w.p, B.t.p, nullptr);
    if (B.obs.live) launch_obs_term(c, B, nullptr, B.w.p, B.t.p, nullptr);
    ops.unstage(kLayoutPlain, B.t.p, B.ext.p, 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(y, B.ext.p, sizeof(double) * (size_t)ops.rows, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDAPDE_OK;
}

// times `reps` applications of the Krylov stage's operator with HIP events on the context's stream: k_block_spmv on the scaled values and, with a data term
// live, k_obs_gather and k_obs_scatter behind it.  Algorithmic bytes per application, every array once per pass: 36 nnz + 4 (n + 1) + 32 n for the block
// product; the term adds (kernels_obs.h), nz = nnz(Psi), m = n_obs: gather 12 nz + 4 (m + 1) + 8 m + 8 n + 8 m, scatter 12 nz + 4 (n + 1) + 8 m + 16 n + 32 n
int e_block_bench_spmv(fdapde_ctx* c, int32_t reps, double* avg_ms, double* algorithmic_bytes) {
    if (!c || reps < 1) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kBlockWords)) return rc;
    if (int rc = handle_live(c, c->block, kBlockWords)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    BlockHandle& B = *c->block;
    const int64_t n = B.n;
    hipLaunchKernelGGL(k_fill_f64, dim3(g1(2 * n)), dim3(256), 0, c->stream, 2 * n, 1.0, B.w.p);
    for (int i = 0; i < 3; ++i) launch_block_op(c, B, B.w.p, B.t.p, nullptr);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < reps; ++i) launch_block_op(c, B, B.w.p, B.t.p, nullptr);
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (avg_ms) *avg_ms = (double)ms / reps;
    if (algorithmic_bytes) {
        *algorithmic_bytes = 36.0 * (double)B.nnz + 4.0 * (double)(n + 1) + 32.0 * (double)n;
        if (B.obs.live) {
            const double nz = (double)B.obs.host.nnz, m = (double)B.obs.host.n_obs;
            *algorithmic_bytes += 24.0 * nz + 4.0 * (m + 1) + 4.0 * (double)(n + 1) + 24.0 * m + 56.0 * (double)n;
        }
    }
    return FDAPDE_OK;
}

int e_block_solve(fdapde_ctx* c, const fdapde_options* opt, const double* b, int32_t n_rhs, double* x, fdapde_info* info) {
    if (!c || !b || !x || n_rhs < 1) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kBlockWords)) return rc;
    if (int rc = handle_live(c, c->block, kBlockWords)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    BlockHandle& B = *c->block;
    HandleCall k;
    if (int rc = handle_call(c, kBlockWords, FDAPDE_SOLVER_BLOCK_AMG, 2 * B.n, opt, &k)) return rc;
    if (k.amg) {
        if (B.obs.live && !c->block_amg_obs)
            return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_BLOCK_AMG: a factored data term (fdapde_block_set_obs) is live; the hierarchy is built from pattern entries only unless the knob block_amg_obs is 1");
        if (!B.jacobi_ok)
            return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_BLOCK_AMG: a DOF's diagonal block is singular (|det| <= 1e-14 max|entry|^2): no block-Jacobi smoother");
    } else {
        if (!k.dense_named && !k.eligible && !B.jacobi_ok)
            return fail(c, FDAPDE_EUNSUPPORTED, "a DOF's diagonal block is singular: no block-Jacobi form for the Krylov stage, and the system is too large for the dense inverse");
        if (k.method == FDAPDE_SOLVER_GMRES && !B.jacobi_ok)
            return fail(c, FDAPDE_EUNSUPPORTED, "a DOF's diagonal block is singular (|det| <= 1e-14 max|entry|^2): no block-Jacobi form for the Krylov stage");
    }
    auto ops = block_ops(c, B);
    if (k.amg) ops.ext_words = std::max<int64_t>(4 * B.nnz, ops.rows * kAmgColsMax);   // (a batch of columns crosses at once)
    return handle_solve(c, B, ops, k, opt, b, n_rhs, x, info);
}

// Psi^T W Psi on the FEM pattern from the rows fdapde_eval_pointwise / fdapde_project hand out: Psi(i, dofs(cell_i, h)) = values[i nb + h]
int e_gram_pointwise(fdapde_ctx* c, int64_t n_locs, const int32_t* cell_ids, const double* values, const double* weights, double* out_values) {
    if (!c || n_locs < 1 || !cell_ids || !values || !out_values) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kBlockWords)) return rc;
    const HostSpace& hs = c->hs;
    for (int64_t k = 0; k < n_locs; ++k)
        if (cell_ids[k] < -1 || cell_ids[k] >= hs.n_cells) {
            c->err = "fdapde_gram_pointwise: location " + std::to_string(k) + " names cell " + std::to_string(cell_ids[k]) + ", which the mesh does not have";
            return FDAPDE_EINVAL;
        }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int nb = hs.nb;
    DBuf<int32_t> d_cells, d_e2i;
    DBuf<double> d_vals, d_w, d_out, d_ext;
    HIPCHK(c, d_cells.upload(cell_ids, (size_t)n_locs, st));
    HIPCHK(c, d_vals.upload(values, (size_t)n_locs * nb, st));
    if (weights) HIPCHK(c, d_w.upload(weights, (size_t)n_locs, st));
    HIPCHK(c, d_e2i.alloc((size_t)hs.n_cells));
    HIPCHK(c, d_out.alloc((size_t)hs.nnz));
    HIPCHK(c, d_ext.alloc((size_t)hs.nnz));
    HIPCHK(c, hipMemsetAsync(d_out.p, 0, sizeof(double) * (size_t)hs.nnz, st));
    hipLaunchKernelGGL(k_block_invert_perm, dim3(g1(hs.n_cells)), dim3(256), 0, st, hs.n_cells, c->cell_i2e.p, d_e2i.p);
    hipLaunchKernelGGL(k_gram_pointwise, dim3(g1(n_locs * nb * nb)), dim3(256), 0, st, n_locs, nb, d_cells.p, d_e2i.p, c->cdofs.p, d_vals.p, weights ? d_w.p : nullptr,
                       c->rowptr.p, c->colidx.p, d_out.p);
    hipLaunchKernelGGL(k_scatter_f64, dim3(g1(hs.nnz)), dim3(256), 0, st, hs.nnz, c->slot_i2e.p, d_out.p, d_ext.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_values, d_ext.p, sizeof(double) * (size_t)hs.nnz, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDAPDE_OK;
}

}   // namespace fdapde_engine
