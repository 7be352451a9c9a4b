// amg_setup.h -- what FDAPDE_SOLVER_AMG (eng_amg.hip) and the point-block forms of eng_block_amg.hip and eng_kron_amg.hip share: a level, a hierarchy, the level
// step of the set-up (pairwise handshake matching twice -- absorb: the rows it leaves single join the pair of their most strongly coupled paired neighbour --,
// the Galerkin products of piecewise-constant P, the members of every aggregate; compared with the host loops of host_amg.cpp under the knob amg_setup_check),
// the stall rule, the retry with absorption, the K-cycle's recursion -- and, written once for all three: the level loop of a build pass (amg_build_levels), the
// rest of a point-block pass (amg_point_smoothers with the cut above a singular coarse block, amg_point_finish with the coarsest level's inverse) and the run of Q columns
// around fgmres_outer (amg_outer_cols).
#ifndef FDAPDE_AMG_SETUP_H
#define FDAPDE_AMG_SETUP_H

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "amg_rows.h"
#include "context.h"
#include "engine.h"
#include "kernels_block.h"
#include "kernels_dense.h"

namespace fdapde_engine {

constexpr double kAmgStall = 0.8;   // a level that keeps more than this share of its rows ends the hierarchy (inverted if the dense limit allows: else unsupported)

struct AmgLevel {
    int64_t n = 0, nnz = 0;
    DBuf<int32_t> rp_own, ci_own;
    DBuf<double> a_own;
    const int32_t *rp = nullptr, *ci = nullptr;   // level 0: the context's pattern and the caller's values; below: the level's own arrays
    const double* a = nullptr;                    // (the block form: the scalar strength matrix on the level's pattern)
    const uint8_t* excl = nullptr;                // rows that belong to no aggregate (level 0's Dirichlet DOFs)
    const double* pay = nullptr;                  // the point-block forms: what rides on the entries (level 0: the handle's), `width` doubles each
    DBuf<double> pay_own;
    DBuf<double> dinv;                            // D^-1: a double per row, or the inverted diagonal blocks of a point-block level
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
// A build into *slot (what it held is dropped first): the knob amg_absorb around `pass(absorb, &stalled)`, which leaves its hierarchy there: 0 pairs only, 1
// absorbs on every level, 2 pairs only and -- where that ends in the stall refusal -- builds again from level 0 with absorption on every level, the first
// attempt booked under discarded_ms
template <typename H, typename Pass> int amg_build_retry(fdapde_ctx* c, H** slot, Pass&& pass) {
    delete *slot;
    *slot = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
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
// the texts of a build pass, each solver's in its own words (whole literals: a message is found by searching for it); nullptr: an answer the form cannot give.
// tag: amg_setup_check's ("", "block ", "kron "); the level loop's two refusals; a singular diagonal block on level 0, and below it with the level above too
// large to end on; the coarsest level's two
struct AmgBuildWords {
    const char *tag, *stalled, *no_free_rows, *level0_block, *cut_too_large, *coarsest_too_large, *coarsest_singular;
};
// The level loop of every build pass: level steps (amg_next_level) from H's last level on, until one has at most `amg_coarse_rows` rows (counted in H.per n_l)
// or a step's verdict ends the hierarchy.  make_level(): an empty level of the solver's type; width: the doubles per entry of AmgLevel::pay that follow the
// strength values (0: none).  *stalled: the answer is the "coarsening stalled above the dense limit" refusal.
// dense_limit: FDAPDE_SOLVER_AMG refuses a stalled level above kDenseMaxRows whatever the knob dense_rows says; the point-block forms above
// min(dense_rows, kDenseMaxRows), counted in H.per n -- two rules nobody has decided between, hence a parameter
template <class MakeLevel>
int amg_build_levels(fdapde_ctx* c, AmgHierarchy& H, int absorb, int width, int64_t dense_limit, const AmgBuildWords& w, MakeLevel&& make_level, bool* stalled) {
    const int64_t coarse_rows = std::max<int64_t>(H.per, std::min<int64_t>(c->amg_coarse_rows, fdapde_hip::kDenseMaxRows));
    while (H.per * H.lv.back()->n > coarse_rows) {
        AmgLevel& F = *H.lv.back();
        auto N = make_level();
        AmgVerdict verdict;
        if (int rc = amg_next_level(c, F, absorb, F.pay, width, H.per, coarse_rows, dense_limit, w.tag, H.lv.size() - 1, *N, width ? &N->pay_own : nullptr, &verdict)) return rc;
        if (verdict == kAmgNoFreeRows && w.no_free_rows) return fail(c, FDAPDE_EUNSUPPORTED, w.no_free_rows);
        if (verdict == kAmgStalled) {
            *stalled = true;
            return fail(c, FDAPDE_EUNSUPPORTED, w.stalled);
        }
        if (verdict != kAmgNext) break;   // (the point-block forms: kAmgNoFreeRows does not arise, no row is excluded)
        if (width) N->pay = N->pay_own.p;
        H.lv.push_back(std::move(N));
    }
    return FDAPDE_OK;
}

// ---- the point-block hierarchies of the operator handles (eng_block_amg.hip, eng_kron_amg.hip): H.per unknowns of a DOF kept together, the coarse corrections
// GCR steps; D: H.per n_L rows, inverted from the coarsest level expanded to scalar CSR (rp2 / ci2 / val2)
struct PointAmg : AmgHierarchy {
    DBuf<int32_t> rp2, ci2;
    DBuf<double> val2;
};
struct BlockAmg : PointAmg {
    bool term = false;             // the levels carry the handle's factored data term (knob block_amg_obs): one column at a time
    double term_ms = 0.0;          // ... and what attaching it cost (part of setup_ms): the host's coarsening, the uploads, g_l
};
struct KronAmg : PointAmg {};
int amg_cols_prepare(fdapde_ctx* c, AmgHierarchy& H, int Q);   // (the levels' work vectors laid out for Q columns: see amg_cycle below)
// A point-block build pass is, in this order: its level 0 (pattern, payload, its strength matrix), amg_build_levels under amg_point_dense_limit, its own step
// between the levels and the smoothers (the block form attaches its data term, whose g_l is part of D; the Kronecker form checks the smoothers' budget),
// amg_point_smoothers, its teams (L.team, L.np), amg_point_finish, its FDAPDE_DEBUG_SETUP line (amg_rows_text)
inline int64_t amg_point_dense_limit(const fdapde_ctx* c) { return std::min<int64_t>(c->dense_rows, fdapde_hip::kDenseMaxRows); }
// The smoother of every level from `judge_from` on that has a next one.  level_dinv(L, flag): L.dinv = D^-1 of the level's diagonal blocks, the launch raising
// the device word `flag` where one is singular.  Such a block on level 0 is a refusal (the block form's: the Kronecker form's level-0 D^-1 is the handle's,
// judged there); below level 0 it ends the hierarchy one level above
template <class Dinv> int amg_point_smoothers(fdapde_ctx* c, AmgHierarchy& H, size_t judge_from, const AmgBuildWords& w, Dinv&& level_dinv) {
    DBuf<int32_t> flag;
    HIPCHK(c, flag.alloc(1));
    for (size_t l = judge_from; l + 1 < H.lv.size(); ++l) {
        int32_t bad = 0;
        HIPCHK(c, hipMemsetAsync(flag.p, 0, sizeof bad, c->stream));
        if (int rc = level_dinv(*H.lv[l], flag.p)) return rc;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&bad, flag.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!bad) continue;
        if (l == 0) return fail(c, FDAPDE_EUNSUPPORTED, w.level0_block);
        if (H.per * H.lv[l - 1]->n > amg_point_dense_limit(c)) return fail(c, FDAPDE_EUNSUPPORTED, w.cut_too_large);
        H.lv.resize(l);
        AmgLevel& E = *H.lv.back();
        E.agg.release(), E.mptr.release(), E.midx.release(), E.dinv.release();
        break;
    }
    return FDAPDE_OK;
}
// The ending: the damping the levels report (the kernels take the constant), the work vectors (one column until a batch asks for more), the coarsest level
// C within the dense inverse's size, expand(C) = C as scalar CSR into rp2 / ci2 / val2, its inverse, setup_ms since t0
template <class Expand> int amg_point_finish(fdapde_ctx* c, PointAmg& H, double omega, const AmgBuildWords& w, std::chrono::steady_clock::time_point t0, Expand&& expand) {
    for (size_t l = 0; l + 1 < H.lv.size(); ++l) H.lv[l]->om = omega;
    if (int rc = amg_cols_prepare(c, H, 1)) return rc;
    AmgLevel& C = *H.lv.back();
    if (H.per * C.n > fdapde_hip::kDenseMaxRows) return fail(c, FDAPDE_EUNSUPPORTED, w.coarsest_too_large);
    if (int rc = expand(C)) return rc;
    if (int rc = dense_build_csr(c, H.per * C.n, H.rp2.p, H.ci2.p, H.val2.p, nullptr, 0, H.D)) return rc;
    if (!H.D.ready) return fail(c, FDAPDE_ENOCONV, w.coarsest_singular);
    H.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FDAPDE_OK;
}
inline std::string amg_rows_text(const AmgHierarchy& H) {   // "578 / 150 / 40": the levels' rows, H.per to a node
    std::string rows;
    for (size_t l = 0; l < H.lv.size(); ++l) rows += (l ? " / " : "") + std::to_string(H.per * H.lv[l]->n);
    return rows;
}
// out = the cycle of level l on r (l < coarsest) for Q in {1, 2, 4, 8} interleaved columns: smoothing, the coarse correction -- below the finest level two
// flexible CG / GCR steps around the next level's cycle (the K-cycle), the dense inverse on the last level --, smoothing.  A column's arithmetic and order do
// not depend on Q.  The levels' work vectors must be laid out for Q: amg_cols_prepare (before a run's first cycle; it costs nothing while the width stays)
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

// the restart length of their outer iteration: the knob gmres_m, never more than maxit nor than the 64 coefficients fgmres_outer's Gram-Schmidt kernels hold --
// one rule for a single-column run and for a batch
inline int amg_point_restart_len(const fdapde_ctx* c, int maxit) { return std::max(1, std::min(std::min(c->gmres_m, 64), std::max(maxit, 1))); }

// ---- the outer run of all three solvers
// how a run starts and how what it hands out is judged
enum AmgRunRule {
    kAmgRunLifted,   // FDAPDE_SOLVER_AMG: the stop rule is relative to the residual of the Dirichlet lift (of x = 0 without one), whatever the run starts from
    kAmgRunPoint     // the operator handles: relative to |b|; a column with b = 0 is solved by x = 0, one with a non-finite |b|^2 cannot start
};
// One run against the hierarchy H for Q columns side by side: K x = rhs per column (x, r: H.per n Q words, the columns interleaved as in kernels_cols.h, internal
// order, on the device; x is written, r is scratch).  The callables launch on the context's stream:
//   product(in, out)    out = K in, the level-0 product the hierarchy was built from
//   residual(x, out)    out = rhs - K x
//   start(again)        false: x = where the stop rule's reference lies (the lift; 0; point-block and warm: the iterate that is there) and r = its residual
//                       (point-block: b); true (only if warm): x = the iterate to start from
// The outer iteration is fgmres_outer at width Q with restart length mk, right-preconditioned by the cycle (the dense inverse on a hierarchy of one level);
// rel: the TRUE relative residuals of what is handed out.  A template as handle_gmres is: the launches are the caller's lambdas
template <class Product, class Residual, class Start>
int amg_outer_cols(fdapde_ctx* c, AmgHierarchy& H, int Q, int mk, AmgRunRule rule, Product&& product, Residual&& residual, Start&& start, bool warm, double* x, double* r,
                   double rtol, int maxit, FgmresCols& S, double* rel) {
    hipStream_t st = c->stream;
    const int64_t n = H.per * H.lv[0]->n;
    const size_t nq = (size_t)n * (size_t)Q;
    const int np = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (n + 4095) / 4096));
    const bool point = rule == kAmgRunPoint;
    if (int rc = amg_cols_prepare(c, H, Q)) return rc;
    HIPCHK(c, H.basis.alloc((size_t)(2 * mk + 1) * nq));
    HIPCHK(c, H.part.alloc((size_t)Q * (size_t)(mk + 5) * (size_t)np));
    HIPCHK(c, H.dots.alloc((size_t)Q * (size_t)(mk + 4)));
    auto dots = [&](const double* a0, double* out) -> int {
        fixed_dots_cols(st, n, np, Q, a0, a0, H.part.p, H.dots.p);
        HIPCHK(c, hipMemcpyAsync(out, H.dots.p, sizeof(double) * (size_t)Q, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        return FDAPDE_OK;
    };
    auto true_rr = [&](double* rr_out) -> int {   // the TRUE residuals of the iterates
        residual((const double*)x, r);
        return dots(r, rr_out);
    };
    if (int rc = start(false)) return rc;
    if (int rc = dots(r, S.bb)) return rc;
    bool live = !point;   // a column that starts, and is judged by its own residual at the end (point-block: 0 < |b|^2 < inf)
    for (int q = 0; q < Q; ++q) {
        S.rr[q] = S.bb[q], S.converged[q] = S.broke[q] = false;
        if (point) S.converged[q] = !(S.bb[q] > 0.0) && std::isfinite(S.bb[q]), S.broke[q] = !std::isfinite(S.bb[q]), live = live || (S.bb[q] > 0.0 && std::isfinite(S.bb[q]));
    }
    if (warm && live) {   // (the parabolic stepper's x0; a column a batch handed back: the residual of its iterate starts the first cycle)
        if (int rc = start(true)) return rc;
        if (int rc = true_rr(S.rr)) return rc;
    }
    for (int q = 0; q < Q; ++q) {
        if (point) S.broke[q] = S.broke[q] || !std::isfinite(S.rr[q]);   // point-block: |b| decided whether the column runs; its iterate may still break it
        else S.converged[q] = S.rr[q] <= rtol * rtol * S.bb[q];          // lifted: a start that already meets the rule against the lift's residual is the answer
    }
    const bool one_level = H.lv.size() == 1;
    auto precond = [&](const double* v, double* z, double* w, bool&) -> int {
        if (one_level) {
            if (int rc = amg_dense_cols(c, H, Q, v, z)) return rc;
        } else if (int rc = amg_cycle(c, H, 0, Q, v, z))
            return rc;
        product(z, w);
        return FDAPDE_OK;
    };
    FgmresSpace fs{n, mk, H.basis.p, H.basis.p + (size_t)(mk + 1) * nq, H.part.p, H.dots.p, np};
    if (int rc = fgmres_outer(c, fs, Q, x, r, nullptr, rtol, maxit, precond, true_rr, S)) return rc;
    double rr[kAmgColsMax];
    if (live)
        if (int rc = true_rr(rr)) return rc;
    for (int q = 0; q < Q; ++q) {
        if (point) {   // what is handed out is judged by its own residual, whichever way the loop ended: the handles promise |b - A x| <= rtol |b|
            if (S.bb[q] > 0.0 && std::isfinite(S.bb[q])) S.rr[q] = rr[q], S.converged[q] = std::isfinite(rr[q]) && rr[q] <= rtol * rtol * S.bb[q];
            rel[q] = S.bb[q] > 0.0 ? std::sqrt(S.rr[q] / S.bb[q]) : 0.0;
        } else {       // the loop's own verdict stands unless the true residual is off by more than a digit: the recurrence of a lifted run is trusted that far
            rel[q] = S.bb[q] > 0.0 ? std::sqrt(rr[q] / S.bb[q]) : 0.0;
            if (S.converged[q] && !(rel[q] <= 10.0 * rtol)) S.converged[q] = false;
        }
    }
    HIPCHK(c, hipGetLastError());
    return FDAPDE_OK;
}
// the point-block callables over the caller's product spmv(in, out): b, x, r, t of H.per n Q words (x is written -- warm: x holds the iterates to start from)
template <class Product> auto amg_point_residual(hipStream_t st, Product& spmv, size_t nq, const double* b, double* t) {
    return [=, &spmv](const double* x, double* out) {
        spmv(x, t);
        hipLaunchKernelGGL(k_bamg_residual, dim3(gn((int64_t)nq)), dim3(256), 0, st, (int64_t)nq, b, (const double*)t, out);
    };
}
inline auto amg_point_start(fdapde_ctx* c, size_t nq, const double* b, double* x, double* r, bool warm) {
    return [=](bool again) -> int {
        if (again) return FDAPDE_OK;   // (x holds the iterate)
        if (!warm) HIPCHK(c, hipMemsetAsync(x, 0, sizeof(double) * nq, c->stream));
        HIPCHK(c, hipMemcpyAsync(r, b, sizeof(double) * nq, hipMemcpyDeviceToDevice, c->stream));
        return FDAPDE_OK;
    };
}

}   // namespace fdapde_engine
#endif
