// eng_block_amg.hip -- FDAPDE_SOLVER_BLOCK_AMG: flexible GMRES around a K-cycle over an aggregation hierarchy of POINT-BLOCK unknowns, for the 2 x 2 block
// handle of eng_block.hip (the smoothing system [ -Psi^T W Psi, lambda R1^T ; lambda R1, lambda R0 ]).
//
// Why: above the dense limit the handle's only stage is GMRES(50) on the block-Jacobi-scaled system, whose iterations grow like 1 / h and each of which
// costs ten operator applications in Gram-Schmidt.  Short recurrences break down on this symmetric indefinite system; the scheme of
// FDAPDE_SOLVER_AMG (eng_amg.hip) with the two unknowns of a DOF kept together does not.
//
// What:
//   set-up    level 0 is the handle's unscaled block CSR.  The aggregates come from eng_amg.hip's level step (amg_next_level: two pairwise passes, with
//             their absorption of the rows left single under the knob amg_absorb) on a SCALAR strength matrix on the same pattern: the (2,1) block as
//             given -- (1,2), (2,2), (1,1) where it was NULL --, whose Galerkin product is the next level's pattern and strength matrix.  The four block
//             values ride along as the step's payload: summed per coarse entry with the same keys in ascending fine-slot order (k_bamg_gsum):
//             P = P_scalar (x) I_2, unknowns interleaved on every level, no float atomics.  Levels until one has at most `amg_coarse_rows` rows (counted
//             in 2 n_l); that one goes through k_block_expand + dense_build_csr.
//   cycle     0.7 D^-1 (D the 2 x 2 diagonal blocks), the coarse correction, 0.7 D^-1 (kernels_block.h k_bamg_*).  Below the finest level the coarse
//             correction is always two GCR steps preconditioned by the next level's cycle -- GCR because the system is indefinite (flexible CG may divide
//             by zero), no early exit (it would need a host read-back inside the cycle).
//   outer     fgmres_outer (eng_pmg.hip) on the UNSCALED system, right-preconditioned by the cycle; the stop rule is the true residual |b - A x| <= rtol |b|.
//             The run of Q columns is amg_outer_cols (amg_setup.h, shared with eng_amg.hip and eng_kron_amg.hip) with this handle's product; the build pass is
//             amg_build_levels, amg_point_smoothers and amg_point_finish (amg_setup.h, shared with eng_kron_amg.hip) around this form's own steps; the loop over a call's columns is
//             handle_solve's (eng_handle.h), which takes block_amg_run and -- for batches -- block_amg_batch from eng_block.hip's callables.
//   the term  (knob block_amg_obs = 1) a live factored data term scale [Psi^T W Psi, 0; 0, 0] rides beside the pattern levels: P = P_s (x) I_2 with entries 1, so
//             its Galerkin product is the term of Psi_{l+1} = Psi_l P_s (host_obs.h obs_coarsen: the same rows, columns through agg).  The aggregates do not see
//             it.  Its diagonal share g_l joins D_l; the coarsest level is inverted with the term merged in (obs_merge_dense); the cycle's launches add the
//             term's products behind the pattern kernels, through Psi_l P_s = Psi_{l+1} never through P (block_pre_restrict, block_post, block_spmv_dots);
//             one column at a time.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "amg_setup.h"
#include "context.h"
#include "engine.h"
#include "host_obs.h"
#include "kernels_block.h"
#include "kernels_dense.h"
#include "kernels_obs.h"

namespace fdapde_engine {

namespace {
using namespace fdapde_hip;

constexpr double kBamgOmega = 0.7;   // the smoother's damping: fixed (the spectrum of D^-1 A is not one-sided: no power iteration)

// a level: the scalar level (n block rows; a = the strength matrix on the pattern; agg, mptr, midx; team, np; the work vectors at 2 n words) and its blocks
// a level's share of a carried data term: Psi_l and its transpose on the device (level 0: the handle's arrays; below: obs_coarsen's, kept on the host too)
struct BamgTerm {
    int64_t m = 0, nnz = 0;                       // n_obs, nnz(Psi_l)
    int32_t longest_row = 0;
    double scale = 0;
    int team_rows = 8, team_cols = 8;             // lanes per row of Psi_l / of Psi_l^T (obs_team_width per level, knob block_obs_team)
    const int32_t *rp = nullptr, *ci = nullptr, *trp = nullptr, *tci = nullptr;
    const double *v = nullptr, *tv = nullptr, *w = nullptr, *g = nullptr;   // (w: the handle's on every level; g: the term's share of D_l)
    fdapde_hip::ObsHost host;
    DBuf<int32_t> rp_own, ci_own, trp_own, tci_own;
    DBuf<double> v_own, tv_own, g_own;
    DBuf<double> t, t2, s;                        // t [n_obs]: W Psi_l zt between pre- and post-smoothing; t2 [n_obs], s [n_l]: the products of y = A x
};
struct BamgLevel : AmgLevel {                     // (pay: the four block values per entry; dinv: the inverted 2 x 2 diagonal blocks, four doubles per row)
    std::unique_ptr<BamgTerm> term;               // the carried data term, or none
};
inline BamgLevel& blk(AmgLevel& L) { return static_cast<BamgLevel&>(L); }

// the term's launches, one column: t = W Psi x_1 (acc: t += ...), y_i += D_i^-1 [scale Psi^T t; 0] (dinv NULL: without D^-1), s = scale Psi^T t
void term_gather(hipStream_t st, const BamgTerm& O, const double* x, double* t, bool acc) {
    if (acc) {
        if (O.team_rows == 64) hipLaunchKernelGGL(k_obs_gather_acc<64>, dim3(g1(O.m, 4)), dim3(256), 0, st, O.m, O.rp, O.ci, O.v, O.w, x, t);
        else hipLaunchKernelGGL(k_obs_gather_acc<8>, dim3(g1(O.m, 32)), dim3(256), 0, st, O.m, O.rp, O.ci, O.v, O.w, x, t);
    } else {
        if (O.team_rows == 64) hipLaunchKernelGGL(k_obs_gather<64>, dim3(g1(O.m, 4)), dim3(256), 0, st, O.m, O.rp, O.ci, O.v, O.w, x, t, (const int32_t*)nullptr);
        else hipLaunchKernelGGL(k_obs_gather<8>, dim3(g1(O.m, 32)), dim3(256), 0, st, O.m, O.rp, O.ci, O.v, O.w, x, t, (const int32_t*)nullptr);
    }
}
void term_scatter(hipStream_t st, const BamgTerm& O, int64_t n, const double* t, double scale, const double* dinv, double* y) {
    if (O.team_cols == 64) hipLaunchKernelGGL(k_obs_scatter<64>, dim3(g1(n, 4)), dim3(256), 0, st, n, O.trp, O.tci, O.tv, t, scale, dinv, y, (const int32_t*)nullptr);
    else hipLaunchKernelGGL(k_obs_scatter<8>, dim3(g1(n, 32)), dim3(256), 0, st, n, O.trp, O.tci, O.tv, t, scale, dinv, y, (const int32_t*)nullptr);
}
void term_scatter_store(hipStream_t st, const BamgTerm& O, int64_t n, const double* t, double scale, double* s) {
    if (O.team_cols == 64) hipLaunchKernelGGL(k_obs_scatter_store<64>, dim3(g1(n, 4)), dim3(256), 0, st, n, O.trp, O.tci, O.tv, t, scale, s);
    else hipLaunchKernelGGL(k_obs_scatter_store<8>, dim3(g1(n, 32)), dim3(256), 0, st, n, O.trp, O.tci, O.tv, t, scale, s);
}
}   // namespace

void block_amg_free(BlockAmg* h) { delete h; }

namespace {
// D^-1 of a level's diagonal blocks (today's 1e-14 rule: k_block_diag_inv; with a carried term D is judged with its share g_l); flag: a block was singular
int level_dinv(fdapde_ctx* c, BamgLevel& L, int32_t* flag) {
    HIPCHK(c, L.dinv.alloc(4 * (size_t)L.n));
    hipLaunchKernelGGL(k_block_diag_inv, dim3(gn(L.n)), dim3(256), 0, c->stream, L.n, L.rp, L.ci, L.pay, L.term ? L.term->g : (const double*)nullptr, L.dinv.p, flag);
    return FDAPDE_OK;
}

// a level's team width and its grid of partials (its work vectors are amg_cols_prepare's)
void level_team(AmgLevel& L) {
    const double per_row = L.n > 0 ? (double)L.nnz / (double)L.n : 1.0;
    L.team = per_row <= 12.0 ? 8 : 16;
    L.np = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (L.n * L.team + 1023) / 1024));
}

// the block cycle's launches: 0.7 D^-1 with the 2 x 2 diagonal blocks as the smoother (kernels_block.h)
void block_pre_restrict(hipStream_t st, int Q, AmgLevel& L, AmgLevel& N, const double* r, double* rc, int64_t rs, int64_t cs) {
    by_team_cols<8>(L.team, Q, [&](auto t, auto q) {
        constexpr int T = decltype(t)::value, QC = decltype(q)::value;
        hipLaunchKernelGGL((k_bamg_pre_restrict<T, QC>), dim3(g1(N.n, 256 / T)), dim3(256), 0, st, N.n, L.mptr.p, L.midx.p, L.rp, L.ci, L.pay, L.dinv.p, kBamgOmega,
                           r, L.zt.p, rc, rs, cs);
    });
    if (BamgTerm* O = blk(L).term.get()) {   // (Q = 1, so rc[2 I] is the first unknown of aggregate I under either layout) rc -= P^T [scale Psi_l^T t; 0], t = W Psi_l zt
        term_gather(st, *O, L.zt.p, O->t.p, false);
        term_scatter(st, *blk(N).term, N.n, O->t.p, -O->scale, nullptr, rc);
    }
}
void block_post(hipStream_t st, int Q, AmgLevel& L, AmgLevel& N, const double* r, double* out) {
    by_team_cols<8>(L.team, Q, [&](auto t, auto q) {
        constexpr int T = decltype(t)::value, QC = decltype(q)::value;
        hipLaunchKernelGGL((k_bamg_post<T, QC>), dim3(g1(L.n, 256 / T)), dim3(256), 0, st, L.n, L.rp, L.ci, L.pay, L.dinv.p, kBamgOmega, L.agg.p, N.e.p, r,
                           L.zt.p, out);
    });
    if (BamgTerm* O = blk(L).term.get()) {   // t += W Psi_{l+1} e: t = W Psi_l (zt + P e); out -= om D^-1 [scale Psi_l^T t; 0]
        term_gather(st, *blk(N).term, N.e.p, O->t.p, true);
        term_scatter(st, *O, L.n, O->t.p, -kBamgOmega * O->scale, L.dinv.p, out);
    }
}
void block_spmv_dots(hipStream_t st, int Q, AmgLevel& L, const double* x, double* y, const double* p0, const double* q0, const double* p1, const double* q1,
                     const double* p2, const double* q2) {
    if (BamgTerm* O = blk(L).term.get()) {   // (Q = 1) the term is inside y before the dots: s = scale Psi_l^T W Psi_l x_1 joins the rows of k_bamg_spmv_dots
        term_gather(st, *O, x, O->t2.p, false);
        term_scatter_store(st, *O, L.n, O->t2.p, O->scale, O->s.p);
        if (L.team <= 8) hipLaunchKernelGGL((k_bamg_spmv_dots<8, 1, true>), dim3((unsigned)L.np), dim3(256), 0, st, L.n, L.rp, L.ci, L.pay, x, y, p0, q0, p1, q1, p2, q2, L.part.p, (const double*)O->s.p);
        else hipLaunchKernelGGL((k_bamg_spmv_dots<16, 1, true>), dim3((unsigned)L.np), dim3(256), 0, st, L.n, L.rp, L.ci, L.pay, x, y, p0, q0, p1, q1, p2, q2, L.part.p, (const double*)O->s.p);
        return;
    }
    by_team_cols<8>(L.team, Q, [&](auto t, auto q) {
        constexpr int T = decltype(t)::value, QC = decltype(q)::value;
        hipLaunchKernelGGL((k_bamg_spmv_dots<T, QC>), dim3((unsigned)L.np), dim3(256), 0, st, L.n, L.rp, L.ci, L.pay, x, y, p0, q0, p1, q1, p2, q2, L.part.p);
    });
}
constexpr AmgCycleOps kBlockOps{block_pre_restrict, block_post, block_spmv_dots};

// The handle's data term beside the pattern levels: Psi_{l+1} = Psi_l P_s through every level's agg on the host, uploaded; g_l by k_obs_diag; the work vectors
int block_amg_attach_term(fdapde_ctx* c, BlockAmg& H, const BlockAmgTerm& src) {
    hipStream_t st = c->stream;
    const fdapde_hip::ObsHost* fine = src.host;
    for (size_t l = 0; l < H.lv.size(); ++l) {
        BamgLevel& L = blk(*H.lv[l]);
        L.term.reset(new BamgTerm());
        BamgTerm& O = *L.term;
        O.m = src.host->n_obs, O.scale = src.scale, O.w = src.w;
        if (l == 0) {
            O.nnz = src.host->nnz, O.longest_row = src.host->longest_row, O.team_rows = src.team_rows, O.team_cols = src.team_cols;
            O.rp = src.rp, O.ci = src.ci, O.trp = src.trp, O.tci = src.tci, O.v = src.v, O.tv = src.tv, O.g = src.g;
        } else {
            std::vector<int32_t> agg;
            HIPCHK(c, hipStreamSynchronize(st));
            if (int rc = fetch(c, H.lv[l - 1]->agg.p, (size_t)H.lv[l - 1]->n, agg)) return rc;
            fdapde_hip::obs_coarsen(*fine, agg.data(), L.n, &O.host);
            const fdapde_hip::ObsHost& P = O.host;
            O.nnz = P.nnz, O.longest_row = P.longest_row;
            O.team_rows = fdapde_hip::obs_team_width(P.n_obs, P.nnz, src.team_knob);
            O.team_cols = fdapde_hip::obs_team_width(P.n, P.nnz, src.team_knob);
            HIPCHK(c, O.rp_own.upload(P.rp.data(), P.rp.size(), st));
            HIPCHK(c, O.ci_own.upload(P.ci.data(), P.ci.size(), st));
            HIPCHK(c, O.v_own.upload(P.v.data(), P.v.size(), st));
            HIPCHK(c, O.trp_own.upload(P.trp.data(), P.trp.size(), st));
            HIPCHK(c, O.tci_own.upload(P.tci.data(), P.tci.size(), st));
            HIPCHK(c, O.tv_own.upload(P.tv.data(), P.tv.size(), st));
            HIPCHK(c, O.g_own.alloc((size_t)L.n));
            O.rp = O.rp_own.p, O.ci = O.ci_own.p, O.trp = O.trp_own.p, O.tci = O.tci_own.p, O.v = O.v_own.p, O.tv = O.tv_own.p, O.g = O.g_own.p;
            if (O.team_cols == 64) hipLaunchKernelGGL(k_obs_diag<64>, dim3(g1(L.n, 4)), dim3(256), 0, st, L.n, O.trp, O.tci, O.tv, O.w, O.scale, O.g_own.p, (const int32_t*)nullptr);
            else hipLaunchKernelGGL(k_obs_diag<8>, dim3(g1(L.n, 32)), dim3(256), 0, st, L.n, O.trp, O.tci, O.tv, O.w, O.scale, O.g_own.p, (const int32_t*)nullptr);
            HIPCHK(c, hipGetLastError());
            fine = &O.host;
        }
        HIPCHK(c, O.t.alloc((size_t)O.m));
        HIPCHK(c, O.t2.alloc((size_t)O.m));
        HIPCHK(c, O.s.alloc((size_t)L.n));
    }
    HIPCHK(c, hipStreamSynchronize(st));   // (the uploads have read the host arrays)
    H.term = true;
    return FDAPDE_OK;
}

// the coarsest level's 2 n-row matrix with the term merged in by the host (as block_dense_build does for level 0): pattern, blocks and Psi_L -> H.rp2 / ci2 / val2
int block_amg_merge_coarsest(fdapde_ctx* c, BlockAmg& H, const BlockAmgTerm& src) {
    hipStream_t st = c->stream;
    BamgLevel& C = blk(*H.lv.back());
    std::vector<int32_t> rp, ci, rp2, ci2;
    std::vector<double> bv, v2;
    HIPCHK(c, hipStreamSynchronize(st));
    if (int rc = fetch(c, C.rp, (size_t)C.n + 1, rp)) return rc;
    if (int rc = fetch(c, C.ci, (size_t)C.nnz, ci)) return rc;
    if (int rc = fetch(c, C.pay, 4 * (size_t)C.nnz, bv)) return rc;
    fdapde_hip::obs_merge_dense(rp.data(), ci.data(), bv.data(), H.lv.size() == 1 ? *src.host : C.term->host, src.scale, &rp2, &ci2, &v2);
    HIPCHK(c, H.rp2.upload(rp2.data(), rp2.size(), st));
    HIPCHK(c, H.ci2.upload(ci2.data(), ci2.size(), st));
    HIPCHK(c, H.val2.upload(v2.data(), v2.size(), st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDAPDE_OK;
}

constexpr AmgBuildWords kBlockBuildWords{
    "block ",
    "FDAPDE_SOLVER_BLOCK_AMG: coarsening stalled above the dense limit (a level kept more than 0.8 of its rows): the strength block has too few strong couplings for pairwise aggregation",
    nullptr,
    "FDAPDE_SOLVER_BLOCK_AMG: a DOF's diagonal block is singular (|det| <= 1e-14 max|entry|^2): no block-Jacobi smoother",
    "FDAPDE_SOLVER_BLOCK_AMG: a coarse level has a singular diagonal block and the level above it is too large for the dense inverse",
    "FDAPDE_SOLVER_BLOCK_AMG: the coarsest level is too large for the dense inverse",
    "FDAPDE_SOLVER_BLOCK_AMG: the coarsest level is singular to working precision"};

// the hierarchy with (absorb) or without absorption on every level, in the order amg_setup.h gives a point-block pass; *stalled: the answer is the "coarsening
// stalled above the dense limit" refusal.  This form's level 0: the strength matrix is the picked block, the four block values its payload
int block_amg_build_pass(fdapde_ctx* c, BlockAmg** slot, const double* raw, int strength_block, const BlockAmgTerm* term, int absorb, bool* stalled) {
    *stalled = false;
    hipStream_t st = c->stream;
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_ptr<BlockAmg> H(new BlockAmg());
    // (GCR, not flexible CG, because the system is indefinite)
    H->ops = &kBlockOps, H->per = 2, H->sym = false, H->absorbed = absorb;
    {
        std::unique_ptr<BamgLevel> L0(new BamgLevel());
        L0->n = c->hs.n_dofs, L0->nnz = c->hs.nnz, L0->rp = c->rowptr.p, L0->ci = c->colidx.p, L0->pay = raw;
        HIPCHK(c, L0->a_own.alloc((size_t)std::max<int64_t>(L0->nnz, 1)));
        hipLaunchKernelGGL(k_bamg_pick, dim3(gn(L0->nnz)), dim3(256), 0, st, L0->nnz, raw, strength_block, L0->a_own.p);
        HIPCHK(c, hipGetLastError());
        L0->a = L0->a_own.p;
        H->lv.push_back(std::move(L0));
    }
    if (int rc = amg_build_levels(c, *H, absorb, 4, amg_point_dense_limit(c), kBlockBuildWords, [] { return std::unique_ptr<AmgLevel>(new BamgLevel()); }, stalled)) return rc;
    if (term) {   // (the aggregates are the pattern's: the term follows them; before the smoothers, because g_l is part of D)
        const auto t1 = std::chrono::steady_clock::now();
        if (int rc = block_amg_attach_term(c, *H, *term)) return rc;
        H->term_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    }
    if (int rc = amg_point_smoothers(c, *H, 0, kBlockBuildWords, [&](AmgLevel& L, int32_t* flag) { return level_dinv(c, blk(L), flag); })) return rc;
    for (auto& L : H->lv) level_team(*L);
    auto expand = [&](AmgLevel& C) -> int {
        if (term) return block_amg_merge_coarsest(c, *H, *term);
        HIPCHK(c, H->rp2.alloc((size_t)(2 * C.n + 1)));
        HIPCHK(c, H->ci2.alloc((size_t)std::max<int64_t>(4 * C.nnz, 1)));
        HIPCHK(c, H->val2.alloc((size_t)std::max<int64_t>(4 * C.nnz, 1)));
        hipLaunchKernelGGL(k_block_expand, dim3(gn(C.n + 1)), dim3(256), 0, st, C.n, C.rp, C.ci, C.pay, H->rp2.p, H->ci2.p, H->val2.p);
        HIPCHK(c, hipGetLastError());
        return FDAPDE_OK;
    };
    if (int rc = amg_point_finish(c, *H, kBamgOmega, kBlockBuildWords, t0, expand)) return rc;
    if (std::getenv("FDAPDE_DEBUG_SETUP"))
        std::fprintf(stderr, "block amg: %zu levels, rows %s, set-up %.2f ms (the data term %.2f), absorbed %d\n", H->lv.size(), amg_rows_text(*H).c_str(), H->setup_ms, H->term_ms,
                     H->absorbed);
    *slot = H.release();
    return FDAPDE_OK;
}
}   // namespace

// the hierarchy of the handle's matrix: raw = the unscaled block CSR on the context's pattern, strength_block = which of its four blocks the aggregation reads.
// Knob amg_absorb: amg_build_retry (amg_setup.h).  term: the handle's live data term for the levels to carry (knob block_amg_obs), or NULL
int block_amg_build(fdapde_ctx* c, BlockAmg** slot, const double* raw, int strength_block, const BlockAmgTerm* term) {
    return amg_build_retry(c, slot, [&](int absorb, bool* stalled) { return block_amg_build_pass(c, slot, raw, strength_block, term, absorb, stalled); });
}

// fdapde_block_obs_amg_levels: the carried term level by level
int block_amg_obs_levels(const BlockAmg* H, int32_t cap, int32_t* n_levels, int64_t* nnz, int32_t* longest_row, int32_t* team_rows, int32_t* team_cols, double* term_ms) {
    if (!H || !H->term) return FDAPDE_ENOTINIT;
    if (n_levels) *n_levels = (int32_t)H->lv.size();
    for (size_t l = 0; l < H->lv.size() && (int64_t)l < (int64_t)cap; ++l) {
        const BamgTerm& O = *static_cast<const BamgLevel&>(*H->lv[l]).term;
        if (nnz) nnz[l] = O.nnz;
        if (longest_row) longest_row[l] = O.longest_row;
        if (team_rows) team_rows[l] = O.team_rows;
        if (team_cols) team_cols[l] = O.team_cols;
    }
    if (term_ms) *term_ms = H->term_ms;
    return FDAPDE_OK;
}
bool block_amg_has_term(const BlockAmg* H) { return H && H->term; }


namespace {
// Q columns side by side against the hierarchy: amg_outer_cols (amg_setup.h) under the point-block rules, with the product of the matrix the hierarchy was
// built from (raw, and the carried term).  block_amg_run is the call at Q = 1, block_amg_batch drives those at Q = 2, 4, 8
int block_amg_cols(fdapde_ctx* c, BlockAmg& H, const double* raw, int Q, const double* b, double* x, double* r, double* t, bool warm, double rtol, int maxit,
                   FgmresCols& S, double* rel) {
    hipStream_t st = c->stream;
    AmgLevel& L0 = *H.lv[0];
    const int64_t n = L0.n;
    const size_t nq = 2 * (size_t)n * (size_t)Q;
    auto spmv = [&](const double* in, double* out) {   // (one column: the block handle's own kernel)
        if (Q == 1) {
            hipLaunchKernelGGL(k_block_spmv<kBlockTeam>, dim3(g1(n, 256 / kBlockTeam)), dim3(256), 0, st, n, L0.rp, L0.ci, raw, in, out, (const int32_t*)nullptr);
            if (BamgTerm* O = blk(L0).term.get()) {   // ... and the term's two products behind it
                term_gather(st, *O, in, O->t2.p, false);
                term_scatter(st, *O, n, O->t2.p, O->scale, nullptr, out);
            }
            return;
        }
        by_cols(Q, [&](auto q) {
            constexpr int QC = decltype(q)::value;
            if constexpr (QC > 1)
                hipLaunchKernelGGL((k_block_spmv_cols<kBlockTeam, QC>), dim3(g1(n, 256 / kBlockTeam)), dim3(256), 0, st, n, L0.rp, L0.ci, raw, in, out);
        });
    };
    return amg_outer_cols(c, H, Q, amg_point_restart_len(c, maxit), kAmgRunPoint, spmv, amg_point_residual(st, spmv, nq, b, t), amg_point_start(c, nq, b, x, r, warm), warm,
                          x, r, rtol, maxit, S, rel);
}
}   // namespace

// one column: A x = b (both interleaved, internal order, on the device; x is written -- warm: x holds the iterate to start from)
int block_amg_run(fdapde_ctx* c, BlockAmg* hp, const double* raw, const double* b_dev, double* x_dev, double rtol, int maxit, int* iters, double* relres,
                  bool* converged_out, bool* broke_out, bool warm) {
    const size_t n2 = 2 * (size_t)hp->lv[0]->n;
    HIPCHK(c, hp->vec.alloc(2 * n2));
    FgmresCols S{};
    if (int rc = block_amg_cols(c, *hp, raw, 1, b_dev, x_dev, hp->vec.p, hp->vec.p + n2, warm, rtol, maxit, S, relres)) return rc;
    *iters = S.it[0], *converged_out = S.converged[0], *broke_out = S.broke[0];
    return FDAPDE_OK;
}

// the widest batch for `left` columns under the knob amg_cols and the basis budget (amg_cols_width); block_amg_run's restart length is kept
int block_amg_width(const fdapde_ctx* c, const BlockAmg* H, int32_t left, int maxit) {
    const int mk = amg_point_restart_len(c, maxit);
    if (H->term) return 1;   // (the term's launches are one column's)
    return amg_cols_width(std::min<int32_t>(left, c->amg_cols), 2 * H->lv[0]->n, mk);
}

// Q columns side by side: ext (device) holds them stacked in the reference numbering, column q at ext + 2 n q, and receives the solutions.  One run of
// block_amg_cols at width Q; a column handed back is finished by block_amg_run from its iterate (col_b, col_x: one column of scratch each).  iters is added to,
// worst / not_conv / broke_any follow block_amg_solve's rules
int block_amg_batch(fdapde_ctx* c, BlockAmg* hp, const double* raw, int Q, double* ext, double* col_b, double* col_x, double rtol, int maxit, int* iters, double* worst,
                    bool* not_conv, bool* broke_any) {
    BlockAmg& H = *hp;
    hipStream_t st = c->stream;
    const int64_t n = H.lv[0]->n, n2 = 2 * n;
    const size_t nq = (size_t)n2 * (size_t)Q;
    HIPCHK(c, H.qvec.alloc(4 * nq));
    double *b = H.qvec.p, *x = b + nq, *r = x + nq, *t = r + nq;
    hipLaunchKernelGGL(k_block_stage_cols, dim3(gn(n * Q)), dim3(256), 0, st, n, Q, c->dof_i2e.p, (const double*)ext, b);
    FgmresCols S{};
    double rels[kAmgColsMax];
    if (int rc = block_amg_cols(c, H, raw, Q, b, x, r, t, false, rtol, maxit, S, rels)) return rc;
    ++H.batches, H.batched_cols += Q;
    for (int q = 0; q < Q; ++q) {
        int it = S.it[q];
        bool conv = S.converged[q], broke = S.broke[q];
        double rel = rels[q];
        if (S.handed[q]) {   // the recurrence and the true residual disagreed: the rest of this column by block_amg_run, from its iterate
            hipLaunchKernelGGL(k_amg_col_get, dim3(gn(n2)), dim3(256), 0, st, n2, Q, q, (const double*)b, col_b);
            hipLaunchKernelGGL(k_amg_col_get, dim3(gn(n2)), dim3(256), 0, st, n2, Q, q, (const double*)x, col_x);
            int it1 = 0;
            if (int rc = block_amg_run(c, hp, raw, col_b, col_x, rtol, maxit - it, &it1, &rel, &conv, &broke, true)) return rc;
            hipLaunchKernelGGL(k_amg_col_put, dim3(gn(n2)), dim3(256), 0, st, n2, Q, q, (const double*)col_x, x);
            it += it1, ++H.single_cols;
        }
        if (!conv) *not_conv = true, *broke_any = *broke_any || broke;
        *iters += it, *worst = rel > *worst || std::isnan(rel) ? rel : *worst;
    }
    hipLaunchKernelGGL(k_block_unstage_cols, dim3(gn(n * Q)), dim3(256), 0, st, n, Q, c->dof_i2e.p, (const double*)x, ext);
    HIPCHK(c, hipGetLastError());
    return FDAPDE_OK;
}

}   // namespace fdapde_engine
