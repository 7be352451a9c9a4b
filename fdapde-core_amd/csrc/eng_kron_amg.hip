// eng_kron_amg.hip -- FDAPDE_SOLVER_KRON_AMG: flexible GMRES around a K-cycle over an aggregation hierarchy of POINT-BLOCK unknowns (q per DOF), for the
// Kronecker-sum handle of eng_kron.hip (A = sum_sigma T_sigma (x) S_sigma).
//
// Why: above the dense limit the handle's only stage is GMRES(50) on the point-block-Jacobi-scaled system, whose iteration counts are mesh-bound
//  and each of whose iterations is dominated by Gram-Schmidt over up to 50 vectors of q n words.
//
// What: the scheme of eng_block_amg.hip with q unknowns of a DOF kept together.  The Kronecker structure survives aggregation: with P = P_scalar (x) I_q,
// P^T (sum T_sigma (x) S_sigma) P = sum T_sigma (x) (P_s^T S_sigma P_s) -- every level is a Kronecker sum with the SAME time factors, and stores n_S values
// per coarse entry in the handle's own layout vals[k n_S + sigma].
//   set-up    level 0 is the handle's pattern, values and D^-1.  The aggregates come from amg_next_level on a SCALAR strength matrix on the same pattern
//             (k_kamg_strength: -sum_sigma |T_sigma|_F |S_sigma[i,j]|, or -- knob kron_amg_term -- the spatial factor of a term as given); the n_S values
//             ride along as the step's payload (width n_S).  Levels until one has at most `amg_coarse_rows` rows (counted in q n_l); that one goes through
//             k_kron_expand_il + dense_build_csr.  D^-1 of every level that has a next one: k_kron_diag_inv on the level's arrays.
//   cycle     0.7 D^-1, the coarse correction (two GCR steps below the finest level: the systems are indefinite or non-symmetric), 0.7 D^-1
//             (kernels_kron.h k_kamg_*); amg_cycle / amg_correction unchanged.
//   outer     fgmres_outer (eng_pmg.hip) on the UNSCALED system, right-preconditioned by the cycle; the stop rule is the true residual |b - A x| <= rtol |b|.
//             The run of a column is amg_outer_cols (amg_setup.h, shared with eng_amg.hip and eng_block_amg.hip) with this handle's product; the build pass is
//             amg_build_levels, amg_point_smoothers and amg_point_finish (amg_setup.h, shared with eng_block_amg.hip) around this form's own steps; the loop over a call's columns is
//             handle_solve's (eng_handle.h).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "amg_setup.h"
#include "context.h"
#include "engine.h"
#include "kernels_dense.h"
#include "kernels_kron.h"

namespace fdapde_engine {

namespace {
using namespace fdapde_hip;

constexpr double kKamgOmega = 0.7;   // the smoother's damping: fixed, as the block form's

// a level: the scalar level (n DOFs; a = the strength matrix on the pattern; agg, mptr, midx; np; the work vectors at q n words) and its Kronecker sum
struct KamgLevel : AmgLevel {
    int q = 0, ns = 0, Q = 2, t_in_lds = 0;       // (the hierarchy's, on every level: the cycle's launches see levels only)
    const double *tm = nullptr;
    const int32_t* band = nullptr;
    const double* dq = nullptr;                   // the inverted q x q diagonal blocks (level 0: the handle's; below: dinv).  pay: n_S doubles per entry
};
inline KamgLevel& kl(AmgLevel& L) { return static_cast<KamgLevel&>(L); }

inline size_t lds_bytes(const KamgLevel& L) { return sizeof(double) * kamg_lds_doubles(L.q, L.ns, L.t_in_lds != 0); }
}   // namespace

void kron_amg_free(KronAmg* h) { delete h; }

namespace {
// the cycle's launches (one column): 0.7 D^-1 with the q x q diagonal blocks as the smoother
void kron_pre_restrict(hipStream_t st, int, AmgLevel& L0, AmgLevel& N, const double* r, double* rc, int64_t rs, int64_t) {
    KamgLevel& L = kl(L0);
    by_team(L.Q, [&](auto t) {
        constexpr int QQ = decltype(t)::value;
        hipLaunchKernelGGL(k_kamg_smooth<QQ>, dim3(g1(L.n, 256 / QQ)), dim3(256), 0, st, L.n, L.q, L.dq, kKamgOmega, r, L.zt.p);
        hipLaunchKernelGGL(k_kamg_pre_restrict<QQ>, dim3(g1(N.n, 256 / QQ)), dim3(256), lds_bytes(L), st, N.n, L.q, L.ns, L.mptr.p, L.midx.p, L.rp, L.ci, L.pay, L.tm,
                           L.band, r, (const double*)L.zt.p, rc, rs, L.t_in_lds);
    });
}
void kron_post(hipStream_t st, int, AmgLevel& L0, AmgLevel& N, const double* r, double* out) {
    KamgLevel& L = kl(L0);
    by_team(L.Q, [&](auto t) {
        constexpr int QQ = decltype(t)::value;
        hipLaunchKernelGGL(k_kamg_post<QQ>, dim3(g1(L.n, 256 / QQ)), dim3(256), lds_bytes(L), st, L.n, L.q, L.ns, L.rp, L.ci, L.pay, L.tm, L.band, L.dq, kKamgOmega,
                           L.agg.p, (const double*)N.e.p, r, (const double*)L.zt.p, out, L.t_in_lds);
    });
}
void kron_spmv_dots(hipStream_t st, int, AmgLevel& L0, const double* x, double* y, const double* p0, const double* q0, const double* p1, const double* q1,
                    const double* p2, const double* q2) {
    KamgLevel& L = kl(L0);
    by_team(L.Q, [&](auto t) {
        constexpr int QQ = decltype(t)::value;
        hipLaunchKernelGGL(k_kamg_spmv_dots<QQ>, dim3((unsigned)L.np), dim3(256), lds_bytes(L), st, L.n, L.q, L.ns, L.rp, L.ci, L.pay, L.tm, L.band, x, y, p0, q0, p1, q1,
                           p2, q2, L.part.p, L.t_in_lds);
    });
}
constexpr AmgCycleOps kKronOps{kron_pre_restrict, kron_post, kron_spmv_dots};

// D^-1 of a level's diagonal blocks (k_kron_diag_inv on the level's own arrays); flag: a block was singular
int level_dinv(fdapde_ctx* c, KamgLevel& L, int32_t* flag) {
    HIPCHK(c, L.dinv.alloc((size_t)L.q * L.q * (size_t)std::max<int64_t>(L.n, 1)));
    by_team(L.Q, [&](auto t) {
        constexpr int QQ = decltype(t)::value;
        hipLaunchKernelGGL(k_kron_diag_inv<QQ>, dim3(g1(L.n, 64 / QQ)), dim3(64), 0, c->stream, L.n, L.q, L.ns, L.rp, L.ci, L.pay, L.tm, (const double*)nullptr,
                           (const double*)nullptr, 0, L.dinv.p, flag);
    });
    L.dq = L.dinv.p;
    return FDAPDE_OK;
}

constexpr AmgBuildWords kKronBuildWords{
    "kron ",
    "FDAPDE_SOLVER_KRON_AMG: coarsening stalled above the dense limit (a level kept more than 0.8 of its rows): the strength matrix has too few strong couplings for pairwise aggregation",
    nullptr, nullptr,
    "FDAPDE_SOLVER_KRON_AMG: a coarse level has a singular diagonal block and the level above it is too large for the dense inverse",
    "FDAPDE_SOLVER_KRON_AMG: the coarsest level is too large for the dense inverse",
    "FDAPDE_SOLVER_KRON_AMG: the coarsest level is singular to working precision"};

// the hierarchy with (absorb) or without absorption on every level, in the order amg_setup.h gives a point-block pass; *stalled: the answer is the "coarsening
// stalled above the dense limit" refusal.  This form's level 0: the strength matrix of k_kamg_strength, the n_S spatial values its payload
int kron_amg_build_pass(fdapde_ctx* c, KronAmg** slot, const KronAmgSource& src, int absorb, bool* stalled) {
    *stalled = false;
    hipStream_t st = c->stream;
    const auto t0 = std::chrono::steady_clock::now();
    const int q = src.q, ns = src.ns;
    std::unique_ptr<KronAmg> H(new KronAmg());
    H->ops = &kKronOps, H->per = q, H->sym = false, H->absorbed = absorb;
    auto make_level = [&] {
        std::unique_ptr<KamgLevel> L(new KamgLevel());
        L->q = q, L->ns = ns, L->Q = src.Q, L->t_in_lds = src.t_in_lds ? 1 : 0, L->tm = src.tm, L->band = src.band;
        return L;
    };
    {
        std::unique_ptr<KamgLevel> L0 = make_level();
        L0->n = c->hs.n_dofs, L0->nnz = c->hs.nnz, L0->rp = c->rowptr.p, L0->ci = c->colidx.p, L0->pay = src.vals, L0->dq = src.dinv;
        DBuf<double> w;
        HIPCHK(c, w.upload(src.tnorm, (size_t)ns, st));
        HIPCHK(c, L0->a_own.alloc((size_t)std::max<int64_t>(L0->nnz, 1)));
        hipLaunchKernelGGL(k_kamg_strength, dim3(gn(L0->nnz)), dim3(256), 0, st, L0->nnz, ns, src.vals, (const double*)w.p, src.pick, L0->a_own.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(st));   // (w goes out of scope)
        L0->a = L0->a_own.p;
        H->lv.push_back(std::move(L0));
    }
    if (int rc = amg_build_levels(c, *H, absorb, ns, amg_point_dense_limit(c), kKronBuildWords, make_level, stalled)) return rc;
    // the smoothers count against the handle's budget together (level 0's is the handle's own)
    double dinv_bytes = 0.0;
    for (size_t l = 0; l + 1 < H->lv.size(); ++l) dinv_bytes += 8.0 * (double)q * (double)q * (double)H->lv[l]->n;
    if (dinv_bytes > (double)c->kron_dinv_mb * 1048576.0)
        return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_KRON_AMG: the inverted diagonal blocks of all levels (8 q^2 n_l bytes each) exceed the budget `kron_dinv_mb`");
    // (judged from level 1: level 0's D^-1 is the handle's)
    if (int rc = amg_point_smoothers(c, *H, 1, kKronBuildWords, [&](AmgLevel& L, int32_t* flag) { return level_dinv(c, kl(L), flag); })) return rc;
    for (auto& L : H->lv) L->team = src.Q, L->np = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (L->n * src.Q + 255) / 256));
    auto expand = [&](AmgLevel& C) -> int {
        const int64_t nq = (int64_t)q * C.n, nnz2 = (int64_t)q * q * C.nnz;
        HIPCHK(c, H->rp2.alloc((size_t)(nq + 1)));
        HIPCHK(c, H->ci2.alloc((size_t)std::max<int64_t>(nnz2, 1)));
        HIPCHK(c, H->val2.alloc((size_t)std::max<int64_t>(nnz2, 1)));
        hipLaunchKernelGGL(k_kron_expand_il, dim3(gn(nq + 1)), dim3(256), 0, st, C.n, q, ns, C.rp, C.ci, C.pay, kl(C).tm, H->rp2.p, H->ci2.p, H->val2.p);
        HIPCHK(c, hipGetLastError());
        return FDAPDE_OK;
    };
    if (int rc = amg_point_finish(c, *H, kKamgOmega, kKronBuildWords, t0, expand)) return rc;
    if (std::getenv("FDAPDE_DEBUG_SETUP"))
        std::fprintf(stderr, "kron amg: %zu levels, rows %s, set-up %.2f ms, absorbed %d\n", H->lv.size(), amg_rows_text(*H).c_str(), H->setup_ms, H->absorbed);
    *slot = H.release();
    return FDAPDE_OK;
}
}   // namespace

// the hierarchy of the handle's matrix (src: its arrays on the context's pattern).  Knob amg_absorb: amg_build_retry (amg_setup.h)
int kron_amg_build(fdapde_ctx* c, KronAmg** slot, const KronAmgSource& src) {
    return amg_build_retry(c, slot, [&](int absorb, bool* stalled) { return kron_amg_build_pass(c, slot, src, absorb, stalled); });
}

// one column: A x = b (both interleaved, internal order, on the device; x is written, from zero): amg_outer_cols (amg_setup.h) at one column under the
// point-block rules, with the handle's own product
int kron_amg_run(fdapde_ctx* c, KronAmg* hp, const double* b, double* x, double rtol, int maxit, int* iters, double* relres, bool* converged_out, bool* broke_out) {
    KronAmg& H = *hp;
    hipStream_t st = c->stream;
    KamgLevel& L0 = kl(*H.lv[0]);
    const int64_t n = L0.n;
    const size_t nq = (size_t)L0.q * (size_t)n;
    HIPCHK(c, H.vec.alloc(2 * nq));
    double *r = H.vec.p, *t = r + nq;
    FgmresCols S{};
    auto spmv = [&](const double* in, double* out) {
        const size_t lds = sizeof(double) * kron_spmv_lds_doubles(L0.q, L0.ns, false, L0.t_in_lds != 0);
        by_team(L0.Q, [&](auto tq) {
            constexpr int QQ = decltype(tq)::value;
            hipLaunchKernelGGL((k_kron_spmv<QQ, false>), dim3(g1(n, 256 / QQ)), dim3(256), lds, st, n, L0.q, L0.ns, L0.rp, L0.ci, L0.pay, L0.tm, L0.band,
                               (const double*)nullptr, in, out, (const int32_t*)nullptr, L0.t_in_lds);
        });
    };
    if (int rc = amg_outer_cols(c, H, 1, amg_point_restart_len(c, maxit), kAmgRunPoint, spmv, amg_point_residual(st, spmv, nq, b, t), amg_point_start(c, nq, b, x, r, false),
                                false, x, r, rtol, maxit, S, relres))
        return rc;
    *iters = S.it[0], *converged_out = S.converged[0], *broke_out = S.broke[0];
    return FDAPDE_OK;
}

}   // namespace fdapde_engine
