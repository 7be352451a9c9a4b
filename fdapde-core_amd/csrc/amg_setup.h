// amg_setup.h -- what FDAPDE_SOLVER_AMG (eng_amg.hip) and the block form of eng_block_amg.hip share: a level, a hierarchy, the level step of the set-up
// (pairwise handshake matching twice -- absorb: the rows it leaves single join the pair of their most strongly coupled paired neighbour --, the Galerkin
// products of piecewise-constant P, the members of every aggregate; compared with the host loops of host_amg.cpp under the knob amg_setup_check), the
// stall rule, the retry with absorption, the K-cycle's recursion, and the column run of the operator handles' point-block hierarchies (amg_point_cols).
#ifndef FDAPDE_AMG_SETUP_H
#define FDAPDE_AMG_SETUP_H

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <memory>
#include <vector>

#include "amg_rows.h"
#include "context.h"
#include "engine.h"
#include "kernels_block.h"

namespace fdapde_engine {

constexpr double kAmgStall = 0.8;   // a level that keeps more than this share of its rows ends the hierarchy (inverted if the dense limit allows: else unsupported)

struct AmgLevel {
    int64_t n = 0, nnz = 0;
    DBuf<int32_t> rp_own, ci_own;
    DBuf<double> a_own;
    const int32_t *rp = nullptr, *ci = nullptr;   // level 0: the context's pattern and the caller's values; below: the level's own arrays
    const double* a = nullptr;                    // (the block form: the scalar strength matrix on the level's pattern)
    const uint8_t* excl = nullptr;                // rows that belong to no aggregate (level 0's Dirichlet DOFs)
    DBuf<double> dinv;
    double om = 0.0;
    int team = 4, np = 1;
    DBuf<int32_t> agg, mptr, midx;                // row -> row of the next level (-1: none); members of each next-level row, ascending
    // work vectors (b: the restricted right-hand side; e: this level's correction), laid out for `cols` interleaved columns -- one from the build on, wider from
    // the first batch of that width (amg_cols_prepare: they only grow): cols times the words, sc 8 per column, part 3 np per column; on the coarsest level b / ecm
    // are column-major (what dense_apply takes), e the correction interleaved again
    DBuf<double> b, zt, cv, v, dv, w, rt, e, ecm, part, sc;
    int cols = 0;
    virtual ~AmgLevel() = default;                // (the block form's levels carry their block values: eng_block_amg.hip)
};

struct AmgHierarchy;
// the launches of a cycle that differ between the two solvers (L: the level, N: the next one),
// for Q in {1, 2, 4, 8} interleaved columns
struct AmgCycleOps {
    // L.zt = the smoothed r, rc = the restricted residual: word w of column q at rc[w * rs + q * cs] (interleaved, or column-major for the dense inverse of the
    // coarsest level)
    void (*pre_restrict)(hipStream_t st, int Q, AmgLevel& L, AmgLevel& N, const double* r, double* rc, int64_t rs, int64_t cs);
    void (*post)(hipStream_t st, int Q, AmgLevel& L, AmgLevel& N, const double* r, double* out);   // out = L.zt + P N.e, smoothed once more
    // y = A x, the partials of p_d . q_d: dot d of column q in L.part[(d Q + q) np ..]
    void (*spmv_dots)(hipStream_t st, int Q, AmgLevel& L, const double* x, double* y, const double* p0, const double* q0, const double* p1, const double* q1,
                      const double* p2, const double* q2);
};

struct AmgHierarchy {
    std::vector<std::unique_ptr<AmgLevel>> lv;
    fdapde_ctx::Dense D;                          // the coarsest level's inverse
    const AmgCycleOps* ops = nullptr;
    int per = 1;                                  // rows per node: vectors hold per * n_l words (the block form: 2, interleaved)
    bool sym = true;                              // the coarse corrections are flexible CG steps (false: GCR)
    int use_bnd = 0;
    const double* A = nullptr;
    int64_t key = -1;
    double setup_ms = 0.0, op_complexity = 0.0;
    int absorbed = 0;                             // its passes absorbed the rows the matching left single (knob amg_absorb)
    double discarded_ms = 0.0;                    // amg_absorb 2: what the build without absorption cost before it stalled (part of setup_ms)
    DBuf<double> vec, basis, part, dots;          // the outer iteration's vectors and flexible GMRES basis
    DBuf<double> qvec, qio;                       // a batch's iterate, residual, right-hand side (interleaved) and staging vectors; its columns in the reference numbering
    int64_t batches = 0, batched_cols = 0, single_cols = 0;   // fdapde_amg_cols_trace: Q-column runs, the columns they took, the columns solved one by one
    int np = 1, mk = 0;
    virtual ~AmgHierarchy() { D.X.release(); }
};

inline unsigned gn(int64_t n) { return (unsigned)((n + 255) / 256); }
template <typename T> int fetch(fdapde_ctx* c, const T* p, size_t n, std::vector<T>& h) {
    h.resize(n);
    if (n) HIPCHK(c, hipMemcpy(h.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost));
    return FDAPDE_OK;
}

// what a level step leaves besides the fine level's agg / mptr / midx and the coarse level
struct AmgCoarse {
    DBuf<int32_t> agg1, agg2;   // row -> pair-graph row (-1: excluded), pair-graph row -> coarse row
    int32_t n1 = 0, n2 = 0;
    AmgLevel T;                 // the pair graph: the Galerkin matrix of pass 1
    DBuf<double> payT;          // the payload on its entries
};
enum AmgVerdict { kAmgNext, kAmgEnd, kAmgStalled, kAmgNoFreeRows };
// One level step on the device.  F: the fine level (pattern, strength values F.a, F.excl or NULL); pay: `width` doubles per entry that follow the strength
// values through both Galerkin products, or NULL.  Pass 1 on F, pass 2 on the pair graph K.T: aggregates of at most four rows (any size if absorb).  Out:
// K, the coarse level N with payN, and F.agg / F.mptr / F.midx.  n1 == 0 (every row excluded): only K.agg1 is built.
int amg_coarsen(fdapde_ctx* c, AmgLevel& F, int absorb, const double* pay, int width, AmgCoarse& K, AmgLevel& N, DBuf<double>* payN);
// amg_coarsen, the comparison with host_coarsen under amg_setup_check (errors as "amg_setup_check: <tag>level <level>: ..."), and the stall rule: a step that
// keeps more than kAmgStall of F's rows (and more than coarse_rows) ends the hierarchy at F -- kAmgEnd, F.agg / mptr / midx released -- unless F is above
// dense_limit: kAmgStalled.  All three counts in rows, per of them to a node.  kAmgNoFreeRows: n1 == 0
int amg_next_level(fdapde_ctx* c, AmgLevel& F, int absorb, const double* pay, int width, int per, int64_t coarse_rows, int64_t dense_limit, const char* tag,
                   size_t level, AmgLevel& N, DBuf<double>* payN, AmgVerdict* verdict);
// The knob amg_absorb around a build `pass(absorb, &stalled)` that leaves its hierarchy in *slot: 0 pairs only, 1 absorbs on every level, 2 pairs only and --
// where that ends in the stall refusal -- builds again from level 0 with absorption on every level, the first attempt booked under discarded_ms
template <typename H, typename Pass> int amg_build_retry(fdapde_ctx* c, H** slot, Pass&& pass) {
    const auto t0 = std::chrono::steady_clock::now();
    bool stalled = false;
    int rc = pass(c->amg_absorb == 1 ? 1 : 0, &stalled);
    if (rc != FDAPDE_OK && stalled && c->amg_absorb == 2) {
        const double first = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        rc = pass(1, &stalled);
        if (rc == FDAPDE_OK) (*slot)->discarded_ms = first, (*slot)->setup_ms += first;
    }
    return rc;
}
// out = the cycle of level l on r (l < coarsest) for Q in {1, 2, 4, 8} interleaved columns: smoothing, the coarse correction -- below the finest level two
// flexible CG / GCR steps around the next level's cycle (the K-cycle), the dense inverse on the last level --, smoothing.  A column's arithmetic and order do
// not depend on Q.  The levels' work vectors must be laid out for Q: amg_cols_prepare (before a run's first cycle; it costs nothing while the width stays)
int amg_cols_prepare(fdapde_ctx* c, AmgHierarchy& H, int Q);
int amg_cycle(fdapde_ctx* c, AmgHierarchy& H, size_t l, int Q, const double* r, double* out);
// the coarsest level alone as the preconditioner: z = D^-1 v for Q interleaved columns (Q >= 2: through the column-major layout dense_apply takes)
int amg_dense_cols(fdapde_ctx* c, AmgHierarchy& H, int Q, const double* v, double* z);
// the restart length of FDAPDE_SOLVER_AMG's outer iteration on n unknowns: at most 50 vectors, at most ~16 GB of basis, never more than maxit.  The single-column
// run and a batch must use the same one (a batch's iterates are the single-column run's)
inline int amg_restart_len(int64_t n, int maxit) {
    const int mk = (int)std::min<int64_t>(50, std::max<int64_t>(5, (int64_t)(16e9 / (16.0 * (double)n))));
    return std::max(1, std::min(mk, std::max(maxit, 1)));
}
// the widest batch the basis budget allows: Q (2 mk + 1) n words within 16 GB, else 4, 2, 1 (the restart length is never shortened)
int amg_cols_width(int want, int64_t n_words, int mk);

// ---- the point-block hierarchies of the operator handles (eng_block_amg.hip, eng_kron_amg.hip): H.per unknowns of a DOF kept together
struct BlockAmg : AmgHierarchy {   // (D: 2 n_L rows; the coarse corrections are GCR steps)
    DBuf<int32_t> rp2, ci2;
    DBuf<double> val2;
    bool term = false;             // the levels carry the handle's factored data term (knob block_amg_obs): one column at a time
    double term_ms = 0.0;          // ... and what attaching it cost (part of setup_ms): the host's coarsening, the uploads, g_l
};
struct KronAmg : AmgHierarchy {    // (D: q n_L rows; the coarse corrections are GCR steps)
    DBuf<int32_t> rp2, ci2, flag;
    DBuf<double> val2;
};
// the restart length of their outer iteration: the knob gmres_m, never more than maxit nor than the 64 coefficients fgmres_outer's Gram-Schmidt kernels hold --
// one rule for a single-column run and for a batch
inline int amg_point_restart_len(const fdapde_ctx* c, int maxit) { return std::max(1, std::min(std::min(c->gmres_m, 64), std::max(maxit, 1))); }
// One run against such a hierarchy for Q columns side by side: A x = b per column (b, x: H.per n Q words, the columns interleaved as in kernels_cols.h, internal
// order, on the device; x is written -- warm: x holds the iterates to start from; r, t: scratch of the same size), spmv(in, out) = the level-0 product the
// hierarchy was built from.  The outer iteration is fgmres_outer at width Q on the UNSCALED system; what is handed out is judged by its own residual:
// S.converged, and rel = |b - A x| / |b| per column.  A template as handle_gmres is: the product is the caller's lambda
template <class Product> int amg_point_cols(fdapde_ctx* c, AmgHierarchy& H, int Q, Product&& spmv, const double* b, double* x, double* r, double* t, bool warm, double rtol, int maxit,
                   FgmresCols& S, double* rel) {
    hipStream_t st = c->stream;
    const int64_t n2 = H.per * H.lv[0]->n;
    const size_t nq = (size_t)n2 * (size_t)Q;
    const int np = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (n2 + 4095) / 4096));
    const int mk = amg_point_restart_len(c, maxit);
    if (int rc = amg_cols_prepare(c, H, Q)) return rc;
    HIPCHK(c, H.basis.alloc((size_t)(2 * mk + 1) * nq));
    HIPCHK(c, H.part.alloc((size_t)Q * ((size_t)(mk + 2) * (size_t)np + 3 * (size_t)np)));
    HIPCHK(c, H.dots.alloc((size_t)Q * (size_t)(mk + 4)));
    double h[kAmgColsMax];
    auto dots = [&](const double* a0) -> int {
        fixed_dots_cols(st, n2, np, Q, a0, a0, H.part.p, H.dots.p);
        HIPCHK(c, hipMemcpyAsync(h, H.dots.p, sizeof(double) * (size_t)Q, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        return FDAPDE_OK;
    };
    auto residual = [&](double* rr_out) -> int {   // the TRUE residuals of the iterates
        spmv(x, t);
        hipLaunchKernelGGL(k_bamg_residual, dim3(gn((int64_t)nq)), dim3(256), 0, st, (int64_t)nq, b, (const double*)t, r);
        if (int rc = dots(r)) return rc;
        std::copy(h, h + Q, rr_out);
        return FDAPDE_OK;
    };
    if (!warm) HIPCHK(c, hipMemsetAsync(x, 0, sizeof(double) * nq, st));
    HIPCHK(c, hipMemcpyAsync(r, b, sizeof(double) * nq, hipMemcpyDeviceToDevice, st));
    if (int rc = dots(r)) return rc;
    bool live = false;   // a column that starts (0 < |b|^2 < inf), and is judged by its own residual at the end
    for (int q = 0; q < Q; ++q) {
        S.bb[q] = S.rr[q] = h[q], S.converged[q] = !(h[q] > 0.0) && std::isfinite(h[q]), S.broke[q] = !std::isfinite(h[q]);
        live = live || (h[q] > 0.0 && std::isfinite(h[q]));
    }
    if (warm && live) {   // (a column a batch handed back: the residual of its iterate starts the first cycle)
        if (int rc = residual(S.rr)) return rc;
        for (int q = 0; q < Q; ++q)
            if (!std::isfinite(S.rr[q])) S.broke[q] = true;
    }
    const bool one_level = H.lv.size() == 1;
    auto precond = [&](const double* v, double* z, double* w, bool&) -> int {
        if (one_level) {
            if (int rc = amg_dense_cols(c, H, Q, v, z)) return rc;
        } else if (int rc = amg_cycle(c, H, 0, Q, v, z))
            return rc;
        spmv(z, w);
        return FDAPDE_OK;
    };
    FgmresSpace fs{n2, mk, H.basis.p, H.basis.p + (size_t)(mk + 1) * nq, H.part.p, H.dots.p, np};
    if (int rc = fgmres_outer(c, fs, Q, x, r, nullptr, rtol, maxit, precond, residual, S)) return rc;
    double rr[kAmgColsMax];
    if (live)   // what is handed out is judged by its own residual, whichever way the loop ended
        if (int rc = residual(rr)) return rc;
    for (int q = 0; q < Q; ++q) {
        if (S.bb[q] > 0.0 && std::isfinite(S.bb[q])) S.rr[q] = rr[q], S.converged[q] = std::isfinite(rr[q]) && rr[q] <= rtol * rtol * S.bb[q];
        rel[q] = S.bb[q] > 0.0 ? std::sqrt(S.rr[q] / S.bb[q]) : 0.0;
    }
    HIPCHK(c, hipGetLastError());
    return FDAPDE_OK;
}

}   // namespace fdapde_engine
#endif
