// eng_kron.hip -- the Kronecker-sum handle: A = sum_k T_k (x) S_k with dense q x q time factors and spatial factors on the FEM pattern (the reference's
// Kronecker(A, B), fdaPDE/linear_algebra/kronecker_product.h:56-80, evaluated into an explicit sparse matrix and handed to SparseLU there): the space-time
// separable smoothing system and the monolithic parabolic system, kept as factors (kernels_kron.h).
//   fdapde_kron_compute      terms -> n_S distinct spatial factors interleaved per pattern entry in the internal order, the summed time factors, D_i^-1
//   fdapde_kron_solve        restarted GMRES(m) on D^-1 A (kernels_gmres.h, buffers of the handle's own), or the dense inverse of the q n-row matrix, or
//                            (by name) flexible GMRES around the point-block multilevel cycle of eng_kron_amg.hip.  The stages, the column loop and the
//                            ending are handle_solve's (eng_handle.h, shared with eng_block.hip); here: the refusals and kron_ops -- staging, operator, builds
//   fdapde_kron_spmv         y = A x
//   fdapde_kron_bench_spmv   HIP-event timing of the Krylov stage's operator
//   fdapde_kron_set_obs      the data term kept factored: the handle's matrix becomes A + scale (Phi (x) Psi)^T W (Phi (x) Psi) with Phi small and dense, Psi a
//                            CSR matrix of any row length, W diagonal (areal designs, missing observations, observation instants off the time nodes); set-up in
//                            host_kron_obs.cpp / host_obs.cpp, the two products per application in kernels_kron_obs.h
// Independent of the n x n handle of fdapde_lin_compute and of the 2 x 2 block handle: nothing here writes a buffer one of the other solves reads back.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "amg_setup.h"
#include "context.h"
#include "engine.h"
#include "eng_handle.h"
#include "host_kron.h"
#include "host_kron_obs.h"
#include "kernels_dense.h"
#include "kernels_gmres.h"
#include "kernels_kron.h"
#include "kernels_kron_obs.h"
#include "kernels_krylov.h"

namespace fdapde_engine {

// the factored data term of the current matrix (fdapde_kron_set_obs): Psi and Psi^T in the internal order on the device, host copies for the dense stage
struct KronObs {
    bool live = false;
    double scale = 0;
    int p = 0, QP = 2;                  // rows of Phi, team width of the term's kernels (the power of two >= max(p, q))
    int form_rows = 1, form_cols = 1;   // 1 narrow / 2 wide for Psi (k_kron_obs_gather) / for Psi^T (k_kron_obs_scatter, k_kron_obs_diag)
    fdapde_hip::ObsHost host;
    std::vector<double> h_phi, h_w;     // [p q] column-major, [n_obs p] interleaved per observation
    DBuf<int32_t> rp, ci, trp, tci;
    DBuf<double> v, tv, w, phi, t, g;   // t [n_obs p]: W (Phi (x) Psi) x between the two products; g [n p]: the term's share of every diagonal block
};

struct KronHandle : HandleCore {       // (the vectors at q n words, ext at least max(n_S nnz, q n), the dense stage on q n rows; jacobi_ok implies have_dinv)
    bool have_dinv = false;            // D^-1 fits the budget (knob kron_dinv_mb) and was built
    bool t_in_lds = false;             // the time factors are small enough to be copied into LDS by every workgroup of the product (kKronLdsFactorDoubles)
    int q = 0, ns = 0, Q = 2;          // unknowns per DOF, distinct spatial factors, team width
    DBuf<double> vals, tm, dinv;       // [n_S nnz] spatial values, [n_S q q] time factors, [q q n] inverted diagonal blocks
    DBuf<int32_t> band;                // [2 q] first / last non-zero column of every T-row
    int n_terms = 0, term_sg[kKronMaxTerms] = {};   // the spatial factor every term of the caller's went into
    double tnorm[kKronMaxTerms] = {};  // |T_sigma|_F of the summed time factors (entries in storage order)
    KronAmg* amg = nullptr;            // FDAPDE_SOLVER_KRON_AMG's hierarchy of the current matrix (eng_kron_amg.hip), built by its first solve
    KronObs obs;
    ~KronHandle() { kron_amg_free(amg); }
};

void kron_release(fdapde_ctx* c) {
    if (!c->kron) return;
    if (c->has_device) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    delete c->kron;
    c->kron = nullptr;
}

void kron_amg_forget(fdapde_ctx* c) {
    if (!c->kron || !c->kron->amg) return;
    if (c->has_device) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    kron_amg_free(c->kron->amg), c->kron->amg = nullptr;
}
// fdapde_kron_amg_hierarchy / _aggregates: the answers of eng_amg.hip on the hierarchy's base (rows q n_l, entries q^2 nnz_l: per = q)
int kron_amg_describe_ctx(const fdapde_ctx* c, int32_t cap, int32_t* n_levels, int64_t* rows, int64_t* nnz, int32_t* absorbed, double* setup_ms) {
    return amg_describe(c->kron ? c->kron->amg : nullptr, cap, n_levels, rows, nnz, absorbed, setup_ms);
}
int kron_amg_aggregates_ctx(fdapde_ctx* c, int32_t level, int64_t cap, int32_t* agg, int64_t* n_rows) {
    return amg_aggregates(c, c->kron ? c->kron->amg : nullptr, level, cap, agg, n_rows);
}

namespace {

constexpr HandleWords kKronWords{
    "the Kronecker-sum handle takes one-GPU contexts, not a rank of a multi-GPU job",
    "call fdapde_kron_compute first",
    "fdapde_kron_solve runs FDAPDE_SOLVER_GMRES, FDAPDE_SOLVER_DENSE, FDAPDE_SOLVER_KRON_AMG or the open method",
    "FDAPDE_SOLVER_DENSE takes Kronecker systems of up to `dense_rows` (at most 8192) rows",
    "the Kronecker matrix",   // (dense_singular's `what`)
    "FDAPDE_SOLVER_KRON_AMG: the flexible GMRES broke down in at least one column",
    "FDAPDE_SOLVER_KRON_AMG: maxit reached in at least one column"};

int team_width(int q) {
    int Q = 2;
    while (Q < q) Q *= 2;
    return Q;
}

// y = A x, or y = D^-1 A x with the inverse fused into the epilogue
void launch_kron_spmv(fdapde_ctx* c, const KronHandle& K, bool fuse, const double* x, double* y, const int32_t* stop) {
    const size_t lds = sizeof(double) * kron_spmv_lds_doubles(K.q, K.ns, fuse, K.t_in_lds);
    const dim3 grid(g1(K.n, 256 / K.Q)), block(256);
    by_team(K.Q, [&](auto t) {
        constexpr int QQ = decltype(t)::value;
        if (fuse)
            hipLaunchKernelGGL((k_kron_spmv<QQ, true>), grid, block, lds, c->stream, K.n, K.q, K.ns, c->rowptr.p, c->colidx.p, K.vals.p, K.tm.p, K.band.p, K.dinv.p, x, y, stop,
                               K.t_in_lds ? 1 : 0);
        else
            hipLaunchKernelGGL((k_kron_spmv<QQ, false>), grid, block, lds, c->stream, K.n, K.q, K.ns, c->rowptr.p, c->colidx.p, K.vals.p, K.tm.p, K.band.p,
                               (const double*)nullptr, x, y, stop, K.t_in_lds ? 1 : 0);
    });
}

// y_i = D_i^-1 x_i (y may be x)
void launch_kron_dinv(fdapde_ctx* c, const KronHandle& K, const double* x, double* y, const int32_t* stop) {
    const dim3 grid(g1(K.n, 256 / K.Q)), block(256);
    by_team(K.Q, [&](auto t) { hipLaunchKernelGGL(k_kron_dinv_apply<decltype(t)::value>, grid, block, 0, c->stream, K.n, K.q, K.dinv.p, x, y, stop); });
}

// (with a data term live: its share Phi^T diag(g_i) Phi joins D_i)
void launch_kron_diag_inv(fdapde_ctx* c, KronHandle& K) {
    const dim3 grid(g1(K.n, 64 / K.Q)), block(64);
    const double *g = K.obs.live ? K.obs.g.p : nullptr, *phi = K.obs.live ? K.obs.phi.p : nullptr;
    const int p = K.obs.live ? K.obs.p : 0;
    by_team(K.Q, [&](auto t) {
        hipLaunchKernelGGL(k_kron_diag_inv<decltype(t)::value>, grid, block, 0, c->stream, K.n, K.q, K.ns, c->rowptr.p, c->colidx.p, K.vals.p, K.tm.p, g, phi, p, K.dinv.p, K.flag.p);
    });
}

// y += [D^-1] scale (Phi (x) Psi)^T W (Phi (x) Psi) x (dinv = NULL: without D^-1) behind a product that wrote y: two launches, the forms as chosen per matrix
void launch_kron_obs(fdapde_ctx* c, const KronHandle& K, const double* dinv, const double* x, double* y, const int32_t* stop) {
    const KronObs& O = K.obs;
    const int64_t m = O.host.n_obs, n = K.n;
    hipStream_t st = c->stream;
    by_team(O.QP, [&](auto t) {
        constexpr int QP = decltype(t)::value;
        if (O.form_rows == 2)
            hipLaunchKernelGGL((k_kron_obs_gather<QP, true>), dim3((unsigned)m), dim3(256), 0, st, m, K.q, O.p, O.rp.p, O.ci.p, O.v.p, O.phi.p, O.w.p, x, O.t.p, stop);
        else
            hipLaunchKernelGGL((k_kron_obs_gather<QP, false>), dim3(g1(m, 256 / QP)), dim3(256), 0, st, m, K.q, O.p, O.rp.p, O.ci.p, O.v.p, O.phi.p, O.w.p, x, O.t.p, stop);
        if (O.form_cols == 2)
            hipLaunchKernelGGL((k_kron_obs_scatter<QP, true>), dim3((unsigned)n), dim3(256), 0, st, n, K.q, O.p, O.trp.p, O.tci.p, O.tv.p, O.phi.p, O.t.p, O.scale, dinv, y, stop);
        else
            hipLaunchKernelGGL((k_kron_obs_scatter<QP, false>), dim3(g1(n, 256 / QP)), dim3(256), 0, st, n, K.q, O.p, O.trp.p, O.tci.p, O.tv.p, O.phi.p, O.t.p, O.scale, dinv, y,
                               stop);
    });
}

// the Krylov stage's operator y = D^-1 A x: one launch with the inverse fused into the epilogue (knob kron_fuse = 1), or the product and the batched
// q x q matvec as two; with a data term live its two products behind either (D^-1 (A x) + D^-1 z: the same sums under both settings)
void launch_kron_op(fdapde_ctx* c, const KronHandle& K, const double* x, double* y, const int32_t* stop) {
    if (c->kron_fuse) {
        launch_kron_spmv(c, K, true, x, y, stop);
    } else {
        launch_kron_spmv(c, K, false, x, y, stop);
        launch_kron_dinv(c, K, y, y, stop);
    }
    if (K.obs.live) launch_kron_obs(c, K, K.dinv.p, x, y, stop);
}

// D^-1 of every DOF (with the live term's share) and the singular-block flag; synchronises
int kron_rediag(fdapde_ctx* c, KronHandle& K) {
    hipStream_t st = c->stream;
    K.jacobi_ok = false;
    if (!K.have_dinv) {
        HIPCHK(c, hipStreamSynchronize(st));
        return FDAPDE_OK;
    }
    HIPCHK(c, hipMemsetAsync(K.flag.p, 0, sizeof(int32_t), st));
    launch_kron_diag_inv(c, K);
    HIPCHK(c, hipGetLastError());
    int32_t h_flag = 0;
    HIPCHK(c, hipMemcpyAsync(&h_flag, K.flag.p, sizeof h_flag, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    K.jacobi_ok = h_flag == 0;
    return FDAPDE_OK;
}

int kron_dense_build(fdapde_ctx* c, KronHandle& K) {
    const int64_t nq = (int64_t)K.q * K.n, nnz2 = (int64_t)K.q * K.q * K.nnz;
    if (K.obs.live) {   // the term merged into the expanded matrix by the host (set-up): build and refinement see the true matrix
        hipStream_t st = c->stream;
        HIPCHK(c, K.rowptr2.alloc((size_t)(nq + 1)));
        HIPCHK(c, K.colidx2.alloc((size_t)nnz2));
        HIPCHK(c, K.val2.alloc((size_t)nnz2));
        hipLaunchKernelGGL(k_kron_expand, dim3(g1(nq + 1)), dim3(256), 0, st, K.n, K.q, K.ns, c->rowptr.p, c->colidx.p, K.vals.p, K.tm.p, K.rowptr2.p, K.colidx2.p, K.val2.p);
        HIPCHK(c, hipGetLastError());
        std::vector<int32_t> rp((size_t)(nq + 1)), ci((size_t)nnz2), rp2, ci2;
        std::vector<double> v((size_t)nnz2), v2;
        HIPCHK(c, hipMemcpyAsync(rp.data(), K.rowptr2.p, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(ci.data(), K.colidx2.p, sizeof(int32_t) * ci.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(v.data(), K.val2.p, sizeof(double) * v.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        fdapde_hip::kron_obs_merge_dense(K.q, rp.data(), ci.data(), v.data(), K.obs.host, K.obs.p, K.obs.h_phi.data(), K.obs.h_w.data(), K.obs.scale, &rp2, &ci2, &v2);
        K.expanded = false;   // (the buffers hold the merged matrix, not k_kron_expand's)
        HIPCHK(c, K.rowptr2.upload(rp2.data(), rp2.size(), st));
        HIPCHK(c, K.colidx2.upload(ci2.data(), ci2.size(), st));
        HIPCHK(c, K.val2.upload(v2.data(), v2.size(), st));
        HIPCHK(c, hipStreamSynchronize(st));   // (the host vectors have been read)
        return dense_build_csr(c, nq, K.rowptr2.p, K.colidx2.p, K.val2.p, nullptr, 0, K.dense);
    }
    if (!K.expanded) {
        HIPCHK(c, K.rowptr2.alloc((size_t)(nq + 1)));
        HIPCHK(c, K.colidx2.alloc((size_t)nnz2));
        HIPCHK(c, K.val2.alloc((size_t)nnz2));
        hipLaunchKernelGGL(k_kron_expand, dim3(g1(nq + 1)), dim3(256), 0, c->stream, K.n, K.q, K.ns, c->rowptr.p, c->colidx.p, K.vals.p, K.tm.p, K.rowptr2.p, K.colidx2.p,
                           K.val2.p);
        HIPCHK(c, hipGetLastError());
        K.expanded = true;
    }
    return dense_build_csr(c, nq, K.rowptr2.p, K.colidx2.p, K.val2.p, nullptr, 0, K.dense);
}

// what a change of the term invalidates: handle_matrix_changed's and the multilevel hierarchy
void kron_matrix_changed(KronHandle& K) {
    handle_matrix_changed(K);
    kron_amg_free(K.amg), K.amg = nullptr;
}

// What handle_solve (eng_handle.h) and fdapde_kron_spmv take from this handle.  Staging: a DOF's q unknowns together (strides q, 1) in the internal order, D^-1
// behind it in place for the Krylov stage; the dense stage's order is the expanded matrix's (strides 1, n).  FDAPDE_SOLVER_KRON_AMG: the hierarchy built by
// the first such solve after fdapde_kron_compute, the columns one after another on the UNSCALED system (stop rule: the true residual |b - A x| <= rtol |b|)
auto kron_ops(fdapde_ctx* c, KronHandle& K) {
    const int64_t n = K.n, nq = (int64_t)K.q * n;
    hipStream_t st = c->stream;
    return HandleOps{
        kKronWords, FDAPDE_SOLVER_KRON_AMG, nq, std::max<int64_t>((int64_t)K.ns * K.nnz, nq),
        [c, &K, n, nq, st](HandleLayout layout, const double* ext, double* dst, int ncols) {
            const bool dense = layout == kLayoutDense;
            hipLaunchKernelGGL(k_kron_stage, dim3(g1(nq), ncols), dim3(256), 0, st, n, K.q, c->dof_i2e.p, ext, dst, dense ? (int64_t)1 : (int64_t)K.q, dense ? n : (int64_t)1);
            if (layout == kLayoutKrylov) launch_kron_dinv(c, K, dst, dst, nullptr);
        },
        [c, &K, n, nq, st](HandleLayout layout, const double* src, double* ext, int ncols) {
            const bool dense = layout == kLayoutDense;
            hipLaunchKernelGGL(k_kron_unstage, dim3(g1(nq), ncols), dim3(256), 0, st, n, K.q, c->dof_i2e.p, src, ext, dense ? (int64_t)1 : (int64_t)K.q, dense ? n : (int64_t)1);
        },
        [c, &K](const double* x, double* y, const int32_t* stop) { launch_kron_op(c, K, x, y, stop); },
        [c, &K] { return kron_dense_build(c, K); },
        [c, &K] {
            if (K.amg) return (int)FDAPDE_OK;
            KronAmgSource src{K.q, K.ns, K.Q, K.t_in_lds, K.vals.p, K.tm.p, K.dinv.p, K.band.p, {}, c->kron_amg_term < 0 ? -1 : K.term_sg[c->kron_amg_term]};
            std::copy(K.tnorm, K.tnorm + kKronMaxTerms, src.tnorm);
            return kron_amg_build(c, &K.amg, src);
        },
        [c, &K](const double* b, double* x, double rtol, int maxit, int* it, double* rel, bool* conv, bool* broke) {
            return kron_amg_run(c, K.amg, b, x, rtol, maxit, it, rel, conv, broke);
        },
        nullptr};
}

}   // namespace

int e_kron_compute(fdapde_ctx* c, int32_t q, int32_t n_terms, const double* const* T, const double* const* S, int32_t symmetric) {
    if (!c) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kKronWords)) return rc;
    if (q < 1 || q > kKronMaxQ) return fail(c, FDAPDE_EINVAL, "fdapde_kron_compute: q must lie in 1 .. 64");
    if (n_terms < 1 || n_terms > kKronMaxTerms) return fail(c, FDAPDE_EINVAL, "fdapde_kron_compute: n_terms must lie in 1 .. 8");
    if (!T || !S) return fail(c, FDAPDE_EINVAL, "fdapde_kron_compute: a NULL factor");
    for (int k = 0; k < n_terms; ++k)
        if (!T[k] || !S[k]) return fail(c, FDAPDE_EINVAL, "fdapde_kron_compute: a NULL factor");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t n = c->hs.n_dofs, nnz = c->hs.nnz, nq = (int64_t)q * n;
    const double* s_of[kKronMaxTerms];
    std::vector<double> tm((size_t)n_terms * q * q);
    std::vector<int32_t> band(2 * (size_t)q);
    const int ns = fdapde_hip::kron_merge_terms(q, n_terms, T, S, s_of, tm.data(), band.data());
    if (!c->kron) c->kron = new KronHandle();
    KronHandle& K = *c->kron;
    if (K.amg) {   // (the hierarchy belonged to the previous matrix)
        HIPCHK(c, hipStreamSynchronize(st));
        kron_amg_free(K.amg), K.amg = nullptr;
    }
    K.n_terms = n_terms;
    for (int k = 0; k < n_terms; ++k) {
        int sg = 0;
        while (s_of[sg] != S[k]) ++sg;
        K.term_sg[k] = sg;
    }
    for (int sg = 0; sg < kKronMaxTerms; ++sg) {
        double s2 = 0.0;
        if (sg < ns)
            for (int e = 0; e < q * q; ++e) s2 += tm[(size_t)sg * q * q + e] * tm[(size_t)sg * q * q + e];
        K.tnorm[sg] = std::sqrt(s2);
    }
    if (K.q != q || K.ns != ns || K.n != n || K.nnz != nnz) {   // another shape: what was sized for the previous one goes (DBuf::alloc only grows -- 4 GB of D^-1 at q = 32 would stay)
        HIPCHK(c, hipStreamSynchronize(st));
        for (DBuf<double>* v : {&K.vals, &K.dinv, &K.ext, &K.bt, &K.x, &K.r, &K.w, &K.t, &K.gm_V, &K.val2, &K.dn_b, &K.dn_x, &K.dense.X}) v->release();
        K.rowptr2.release(), K.colidx2.release();
    }
    K.obs.live = false;   // (the data term belonged to the previous matrix)
    K.ready = false, K.n = n, K.nnz = nnz, K.q = q, K.ns = ns, K.Q = team_width(q), K.symmetric = symmetric != 0, K.jacobi_ok = false;
    handle_matrix_changed(K);
    K.t_in_lds = ns * q * q <= kKronLdsFactorDoubles;
    K.have_dinv = 8.0 * (double)q * (double)q * (double)n <= (double)c->kron_dinv_mb * 1048576.0;
    HIPCHK(c, K.ext.alloc((size_t)std::max<int64_t>((int64_t)ns * nnz, nq)));
    HIPCHK(c, K.vals.alloc((size_t)((int64_t)ns * nnz)));
    HIPCHK(c, K.tm.upload(tm.data(), (size_t)ns * q * q, st));
    HIPCHK(c, K.band.upload(band.data(), band.size(), st));
    if (K.have_dinv) HIPCHK(c, K.dinv.alloc((size_t)q * q * (size_t)n));
    else K.dinv.release();
    HIPCHK(c, K.flag.alloc(1));
    HIPCHK(c, K.ctl.alloc(8));
    HIPCHK(c, K.sc.alloc(32));
    for (DBuf<double>* v : {&K.bt, &K.x, &K.r, &K.w, &K.t}) HIPCHK(c, v->alloc((size_t)nq));
    for (int sg = 0; sg < ns; ++sg) HIPCHK(c, hipMemcpyAsync(K.ext.p + (size_t)sg * nnz, s_of[sg], sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(K.flag.p, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_kron_pack, dim3(g1(nnz * ns)), dim3(256), 0, st, nnz, ns, c->slot_i2e.p, K.ext.p, K.vals.p);
    if (K.have_dinv) launch_kron_diag_inv(c, K);
    HIPCHK(c, hipGetLastError());
    int32_t h_flag = 0;
    HIPCHK(c, hipMemcpyAsync(&h_flag, K.flag.p, sizeof h_flag, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));   // (the caller's factors and the host copies of the time factors have been read)
    K.jacobi_ok = K.have_dinv && h_flag == 0;
    K.ready = true;
    return FDAPDE_OK;
}

int e_kron_set_obs(fdapde_ctx* c, int32_t p, const double* Phi, int64_t n_obs, const int64_t* rowptr, const int32_t* colidx, const double* values,
                   const double* weights, double scale) {
    if (!c) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kKronWords)) return rc;
    if (int rc = handle_live(c, c->kron, kKronWords)) return rc;
    if (n_obs < 0) return fail(c, FDAPDE_EINVAL, "fdapde_kron_set_obs: n_obs is negative");
    HIPCHK(c, hipSetDevice(c->device));
    KronHandle& K = *c->kron;
    KronObs& O = K.obs;
    hipStream_t st = c->stream;
    const int64_t n = K.n;
    if (n_obs == 0 || !rowptr) {   // clears the term
        if (!O.live) return FDAPDE_OK;
        HIPCHK(c, hipStreamSynchronize(st));
        O.live = false;
        kron_matrix_changed(K);
        return kron_rediag(c, K);
    }
    std::string why;
    if (!fdapde_hip::kron_obs_validate(n, K.q, p, Phi, n_obs, rowptr, colidx, values, weights, scale, &why)) {   // (nothing launched, the previous term stays)
        c->err = why;
        return FDAPDE_EINVAL;
    }
    if (int rc = ensure_host(c, kHostPerm)) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    fdapde_hip::ObsHost& P = O.host;
    O.live = false;
    kron_matrix_changed(K);
    fdapde_hip::obs_build(n, n_obs, rowptr, colidx, values, nullptr, c->hs.dof_e2i.data(), &P);
    fdapde_hip::kron_obs_phi(K.q, p, Phi, &O.h_phi);
    fdapde_hip::kron_obs_weights(p, n_obs, weights, &O.h_w);
    O.scale = scale, O.p = p, O.QP = fdapde_hip::kron_obs_team_width(K.q, p);
    O.form_rows = fdapde_hip::kron_obs_form(P.n_obs, P.nnz, c->kron_obs_form);
    O.form_cols = fdapde_hip::kron_obs_form(P.n, P.nnz, c->kron_obs_form);
    HIPCHK(c, O.rp.upload(P.rp.data(), P.rp.size(), st));
    HIPCHK(c, O.ci.upload(P.ci.data(), P.ci.size(), st));
    HIPCHK(c, O.v.upload(P.v.data(), P.v.size(), st));
    HIPCHK(c, O.trp.upload(P.trp.data(), P.trp.size(), st));
    HIPCHK(c, O.tci.upload(P.tci.data(), P.tci.size(), st));
    HIPCHK(c, O.tv.upload(P.tv.data(), P.tv.size(), st));
    HIPCHK(c, O.w.upload(O.h_w.data(), O.h_w.size(), st));
    HIPCHK(c, O.phi.upload(O.h_phi.data(), O.h_phi.size(), st));
    HIPCHK(c, O.t.alloc((size_t)n_obs * p));
    HIPCHK(c, O.g.alloc((size_t)n * p));
    by_team(O.QP, [&](auto t) {
        constexpr int QP = decltype(t)::value;
        if (O.form_cols == 2)
            hipLaunchKernelGGL((k_kron_obs_diag<QP, true>), dim3((unsigned)n), dim3(256), 0, st, n, p, O.trp.p, O.tci.p, O.tv.p, O.w.p, scale, O.g.p, (const int32_t*)nullptr);
        else
            hipLaunchKernelGGL((k_kron_obs_diag<QP, false>), dim3(g1(n, 256 / QP)), dim3(256), 0, st, n, p, O.trp.p, O.tci.p, O.tv.p, O.w.p, scale, O.g.p,
                               (const int32_t*)nullptr);
    });
    O.live = true;
    if (int rc = kron_rediag(c, K)) {   // (synchronises: the uploads are done)
        O.live = false;
        return rc;
    }
    return FDAPDE_OK;
}

int e_kron_obs_info(fdapde_ctx* c, int32_t* p, int64_t* n_obs, int64_t* nnz, int32_t* form_rows, int32_t* form_cols) {
    if (!c) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kKronWords)) return rc;
    if (int rc = handle_live(c, c->kron, kKronWords)) return rc;
    const KronObs& O = c->kron->obs;
    if (!O.live) return fail(c, FDAPDE_ENOTINIT, "fdapde_kron_obs_info: no data term is live (fdapde_kron_set_obs)");
    if (p) *p = O.p;
    if (n_obs) *n_obs = O.host.n_obs;
    if (nnz) *nnz = O.host.nnz;
    if (form_rows) *form_rows = O.form_rows;
    if (form_cols) *form_cols = O.form_cols;
    return FDAPDE_OK;
}

int e_kron_spmv(fdapde_ctx* c, const double* x, double* y) {
    if (!c || !x || !y) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kKronWords)) return rc;
    if (int rc = handle_live(c, c->kron, kKronWords)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    KronHandle& K = *c->kron;
    hipStream_t st = c->stream;
    const auto ops = kron_ops(c, K);
    HIPCHK(c, hipMemcpyAsync(K.ext.p, x, sizeof(double) * (size_t)ops.rows, hipMemcpyHostToDevice, st));
    ops.stage(kLayoutPlain, K.ext.p, K.w.p, 1);
    launch_kron_spmv(c, K, false, K.w.p, K.t.p, nullptr);
    if (K.obs.live) launch_kron_obs(c, K, nullptr, K.w.p, K.t.p, nullptr);
    ops.unstage(kLayoutPlain, K.t.p, K.ext.p, 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(y, K.ext.p, sizeof(double) * (size_t)ops.rows, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDAPDE_OK;
}

// times `reps` launches of the Krylov stage's operator (D^-1 A, fused or as two launches: knob kron_fuse; the plain product where D^-1 is not there) with
// HIP events on the context's stream
int e_kron_bench_spmv(fdapde_ctx* c, int32_t reps, double* avg_ms, double* algorithmic_bytes) {
    if (!c || reps < 1) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kKronWords)) return rc;
    if (int rc = handle_live(c, c->kron, kKronWords)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    KronHandle& K = *c->kron;
    const int64_t n = K.n, nq = (int64_t)K.q * n;
    auto op = [&]() {
        if (K.have_dinv) launch_kron_op(c, K, K.w.p, K.t.p, nullptr);
        else {
            launch_kron_spmv(c, K, false, K.w.p, K.t.p, nullptr);
            if (K.obs.live) launch_kron_obs(c, K, nullptr, K.w.p, K.t.p, nullptr);
        }
    };
    hipLaunchKernelGGL(k_fill_f64, dim3(g1(nq)), dim3(256), 0, c->stream, nq, 1.0, K.w.p);
    for (int i = 0; i < 3; ++i) op();
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < reps; ++i) op();
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipGetLastError());
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (avg_ms) *avg_ms = (double)ms / reps;
    if (algorithmic_bytes) {
        *algorithmic_bytes = 8.0 * K.ns * (double)K.nnz + 4.0 * (double)K.nnz + 4.0 * (double)(n + 1) + 16.0 * (double)nq + (K.have_dinv ? 8.0 * K.q * (double)nq : 0.0);
        if (K.obs.live) {   // gather 12 nz + 4 (m + 1) + 8 q n + 16 p m, scatter 12 nz + 4 (n + 1) + 8 p m + 16 q n (+ 8 q^2 n in the Krylov stage)
            const double nz = (double)K.obs.host.nnz, m = (double)K.obs.host.n_obs, pm = K.obs.p * m;
            *algorithmic_bytes += 24.0 * nz + 4.0 * (m + 1) + 4.0 * (double)(n + 1) + 24.0 * pm + 24.0 * (double)nq + (K.have_dinv ? 8.0 * K.q * (double)nq : 0.0);
        }
    }
    return FDAPDE_OK;
}

int e_kron_solve(fdapde_ctx* c, const fdapde_options* opt, const double* b, int32_t n_rhs, double* x, fdapde_info* info) {
    if (!c || !b || !x || n_rhs < 1) return FDAPDE_EINVAL;
    if (int rc = handle_guard(c, kKronWords)) return rc;
    if (int rc = handle_live(c, c->kron, kKronWords)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    KronHandle& K = *c->kron;
    HandleCall k;
    if (int rc = handle_call(c, kKronWords, FDAPDE_SOLVER_KRON_AMG, (int64_t)K.q * K.n, opt, &k)) return rc;
    if (k.amg) {
        if (K.obs.live)
            return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_KRON_AMG: a factored data term (fdapde_kron_set_obs) is live; the hierarchy is built from pattern entries only");
        if (!K.have_dinv)
            return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_KRON_AMG: the inverted diagonal blocks (8 q^2 n bytes) exceed the budget `kron_dinv_mb`: no block-Jacobi smoother");
        if (!K.jacobi_ok)
            return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_KRON_AMG: a DOF's diagonal block is singular (a pivot <= 1e-14 max|entry|): no block-Jacobi smoother");
        if (!K.amg && c->kron_amg_term >= K.n_terms) return fail(c, FDAPDE_EINVAL, "FDAPDE_SOLVER_KRON_AMG: the knob `kron_amg_term` names a term the handle was not given");
    } else {
        if (k.method == FDAPDE_SOLVER_GMRES && !K.have_dinv)
            return fail(c, FDAPDE_EUNSUPPORTED, "the inverted diagonal blocks (8 q^2 n bytes) exceed the budget `kron_dinv_mb`: no Krylov stage for this Kronecker handle");
        if (k.method == FDAPDE_SOLVER_GMRES && !K.jacobi_ok)   // (the record names the method first)
            return bare_answer(c, FDAPDE_SOLVER_GMRES, 0.0, info, fail(c, FDAPDE_ENOCONV, "a DOF's diagonal block is singular (a pivot <= 1e-14 max|entry|): no block-Jacobi form for the Krylov stage"));
        if (k.open && !k.eligible && !K.jacobi_ok)
            return fail(c, FDAPDE_EUNSUPPORTED, K.have_dinv ? "a DOF's diagonal block is singular: no block-Jacobi form for the Krylov stage, and the system is too large for the dense inverse"
                                                            : "the inverted diagonal blocks exceed the budget `kron_dinv_mb`, and the system is too large for the dense inverse");
    }
    return handle_solve(c, K, kron_ops(c, K), k, opt, b, n_rhs, x, info);
}

}   // namespace fdapde_engine
