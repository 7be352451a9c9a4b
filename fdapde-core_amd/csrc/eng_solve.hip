// eng_solve.hip -- the multi-launch solve driver: SpMV dispatch, solver layouts (compact CSR pattern, blocked ELL), Jacobi scaling and
// Dirichlet reduction (solve_prepare), the Krylov driver (solve_run), elliptic / parabolic / factor-once entry points, result getters, SpMV
// benchmarks.  The three long paths are sequences of file-local stages (anonymous namespaces, in front of the function that calls them):
//   solve_run          resolve_method, then the stages of one SolveRun record (its member functions): start_up -> run_gmres | run_rowdist |
//                      single_launch (the hand-over to persist_engine.hip) -> run_chunks (one enqueue_* per method: fused-update / single-reduction /
//                      two-kernel CG, BiCGStab on one GPU and element-partitioned; chunk_graph for the captured chunk; read_outcome) -> finish
//   e_solve_parabolic  the dense loops, then step_loop around amg_run / pmg_run / the Krylov step; every path ends in stepper_end
//   e_lin_solve        the stages of one LinCall record: dense_stage, batches, direct_column, columns_side_by_side, columns_one_by_one advance
//                      its ColumnTally
// What fdapde_solve, the stepper and the handle say and decide alike (outcome_from, open_gmres_budget, cg_breakdown_agreed, the texts of
// FDAPDE_SOLVER_DENSE) stands once, in front of run_gmres.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>

#include <dlfcn.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>

#include "context.h"
#include "engine.h"
#include "kernels.h"

namespace fdapde_engine {

constexpr int64_t kBlockedShortRowsAbove = 3200000;   // short-row systems (P1) of more DOFs than this take the blocked-ELL SpMV on the multi-launch path

// the captured CG chunk bakes pointers and sizes in: drop it whenever a layout, buffer or knob may have changed
void drop_graph(fdapde_ctx* c) {
    if (c->cg_graph_exec) (void)hipGraphExecDestroy(c->cg_graph_exec);
    c->cg_graph_exec = nullptr;
}

// e0 / e1 (optional): HIP events attached to the dispatch itself (hipExtLaunchKernelGGL), i.e. the kernel's own begin / end
// timestamps on the stream it runs on -- the same interval rocprofv3 --kernel-trace reports, with no extra marker packet
// between the neighbouring kernels.
// y = (I + offdiag) x from the blocked-ELL layout of boundary variant v with the values its ell_val holds (k_spmv_blocked; y = x on the rows it leaves out)
void launch_spmv_blocked(fdapde_ctx* c, int v, const double* x, double* y, const double* w, double* partial, const int32_t* stop, hipEvent_t e0, hipEvent_t e1,
                         int dot2_ww) {
    {
        const fdapde_ctx::Blocked& bk = c->bk[v];
        BlockedSpmvArgs a{};
        a.G = bk.meta.G, a.nsl = bk.meta.nsl, a.imp_cap = bk.imp_cap, a.dot2_ww = dot2_ww;
        a.slot_dof = bk.slot_dof.p, a.ell_off = bk.ell_off.p, a.sl_off = bk.sl_off.p, a.ell_code = bk.ell_code.p, a.ell_val = bk.ell_val.p;
        a.imp_off = bk.imp_off.p, a.imp_dof = bk.imp_dof.p, a.drop_dof = bk.drop_dof.p, a.n_drop = (int32_t)bk.meta.n_drop, a.x = x, a.y = y, a.w = partial ? (w ? w : x) : nullptr, a.partial = partial, a.stop = stop;
        void (*k)(BlockedSpmvArgs) = bk.meta.R == 2 ? k_spmv_blocked<2> : bk.meta.R == 4 ? k_spmv_blocked<4> : bk.meta.R == 8 ? k_spmv_blocked<8> : k_spmv_blocked<16>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bk.lds_bytes);
        if (e0 || e1) hipExtLaunchKernelGGL(k, dim3(a.G), dim3(kPersistT), bk.lds_bytes, c->stream, e0, e1, 0, a);
        else hipLaunchKernelGGL(k, dim3(a.G), dim3(kPersistT), bk.lds_bytes, c->stream, a);
    }
}

// The instantiations of k_spmv_team2 that a size, a pattern or the platform selects, as tables indexed by the two run-time flags
// [implicit diagonal owner-masked (multi-GPU)][dot operand == x (CG: p.Ap; one row load serves both)].  WX_FORM = false: this team
// width has no dot-operand-is-x form, the general one serves.
using spmv_kernel_t = void (*)(SpmvArgs, int64_t, int64_t);
template <int T, int U, bool C16, bool WX_FORM, bool VROWS = false, bool NTV = false>
spmv_kernel_t spmv_form(bool dist, bool wx) {
    static const spmv_kernel_t form[2][2] = {
        {k_spmv_team2<T, U, C16, false, false, VROWS, NTV>, k_spmv_team2<T, U, C16, false, WX_FORM, VROWS, NTV>},
        {k_spmv_team2<T, U, C16, true, false, VROWS, NTV>, k_spmv_team2<T, U, C16, true, WX_FORM, VROWS, NTV>}};
    return form[dist][wx];
}
// ... with 16-bit column codes when the pattern has them
template <int T, int U, bool WX_FORM>
spmv_kernel_t spmv_plain_form(bool c16, bool dist, bool wx) {
    return c16 ? spmv_form<T, U, true, WX_FORM>(dist, wx) : spmv_form<T, U, false, WX_FORM>(dist, wx);
}

void launch_spmv(fdapde_ctx* c, const double* vals, const double* x, double* y, const double* w, double* partial,
                 const int32_t* stop, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, int dot2_ww = 0,
                 const uint8_t* owned = nullptr) {
    if (vals == c->sval.p && c->bk_cur >= 0 && owned == nullptr) {   // the solver's scaled matrix in blocked-ELL form (k_spmv_blocked)
        launch_spmv_blocked(c, c->bk_cur, x, y, w, partial, stop, e0, e1, dot2_ww);
        return;
    }
    SpmvArgs s{};
    s.rowptr = c->rowptr.p, s.colidx = c->colidx.p, s.vals = vals, s.x = x, s.y = y;
    s.nnz = (int32_t)c->hs.nnz;
    s.w = w, s.partial = partial, s.stop = stop, s.dot2_ww = dot2_ww, s.owned = owned, s.unit_diag = 0;
    s.n_cols = (int32_t)c->hs.n_dofs;
    // value-stream policy by size: x and y slices of a row band (16 bytes per row, 8 bands) against the 4 MB L2 of an XCD
    const bool ntv = c->spmv_ntv < 0 ? c->hs.n_dofs > kNtValsRows : c->spmv_ntv != 0;
    int64_t n = c->hs.n_dofs;   // rows of the CSR arrays the kernel walks (virtual rows for a segmented pattern)
    bool vrows = false;
    if (vals == c->sval.p && c->sp_cur >= 0) {   // the solver's scaled matrix lives in the compact pattern
        s.rowptr = c->sp_rowptr[c->sp_cur].p, s.colidx = c->sp_colidx[c->sp_cur].p, s.nnz = (int32_t)c->sp_nnz[c->sp_cur];
        if (c->spmv_c16) s.col16 = c->sp_col16[c->sp_cur].p, s.tbase = c->sp_tbase[c->sp_cur].p;
        if (c->sp_nv[c->sp_cur] > 0) {   // segmented: only the VROWS instantiations understand it (always with column codes)
            vrows = true, n = c->sp_nv[c->sp_cur], s.vrow = c->sp_vrow[c->sp_cur].p;
            s.col16 = c->sp_col16[c->sp_cur].p, s.tbase = c->sp_tbase[c->sp_cur].p;
        }
        s.unit_diag = 1;
        // multi-GPU: the local diagonals s_i^2 (A_p)_ii of an interface DOF sum to 1 over the ranks sharing it; the implicit
        // unit diagonal is therefore contributed by the DOF's owner only (any split of the entries among ranks is valid)
        if ((c->comm != nullptr || c->ar_fn != nullptr) && c->halo_ready) s.owned = c->owned.p;
    }
    // eight row bands (one per XCD); band starts on a multiple of 32 rows so that a wavefront tile lies in one code group
    const int64_t rpb = (((n + 7) / 8) + 31) & ~int64_t(31);
    // two entries per lane: team = lanes per row, covering 2 * team entries per pass
    const bool c16 = s.col16 != nullptr, dist = s.unit_diag && s.owned != nullptr;
    const bool wx = s.w == nullptr || s.w == s.x;
    spmv_kernel_t k;
    if (vrows)   // built for this team size (build_solver_pattern); T = 8 or 16
        k = c->sp_team == 8 ? spmv_form<8, 4, /*C16*/ true, /*WX_FORM*/ true, /*VROWS*/ true>(dist, wx)
                             : spmv_form<16, 4, /*C16*/ true, /*WX_FORM*/ true, /*VROWS*/ true>(dist, wx);
    else
        switch (c->spmv_team) {
        case 2: k = spmv_plain_form<2, 1, false>(c16, dist, wx); break;
        case 4: k = spmv_plain_form<4, 2, true>(c16, dist, wx); break;
        case 8:   // large matrix: hinted value stream (see load_pair)
            k = (ntv && c16) ? spmv_form<8, 4, /*C16*/ true, /*WX_FORM*/ true, /*VROWS*/ false, /*NTV*/ true>(dist, wx)
                             : spmv_plain_form<8, 4, true>(c16, dist, wx);
            break;
        case 16: k = spmv_plain_form<16, 4, true>(c16, dist, wx); break;
        default: k = spmv_plain_form<32, 4, false>(c16, dist, wx); break;
        }
    // dispatch-attached events only where a launch is timed; the plain launch can be captured into a hipGraph
    const dim3 grid(c->spmv_grid), block(256);
    if (e0 || e1) hipExtLaunchKernelGGL(k, grid, block, 0, c->stream, e0, e1, 0, s, n, rpb);
    else hipLaunchKernelGGL(k, grid, block, 0, c->stream, s, n, rpb);
}

// default iteration bound: 10 n capped at 100 000 -- but ONE number for all ranks of a row-distributed solve (the launches stop by it and
// advance their epoch tags by it: n is the rank's own DOF count there)
inline int default_maxit(const fdapde_ctx* c, int64_t n) { return c->rd.ready ? 100000 : (int)(10 * n < 100000 ? 10 * n : 100000); }

// compact solver pattern v (0: no Dirichlet reduction, 1: Dirichlet rows / columns dropped) + its 16-bit column codes; host work
// and uploads, done once per function space and boundary mask (fdapde_solver_prepare, or lazily by the first solve)
int build_solver_pattern(fdapde_ctx* c, int v) {
    if (c->sp_built[v]) return FDAPDE_OK;
    if (int rc = ensure_host(c, kHostPattern)) return rc;
    drop_graph(c);
    hipStream_t st = c->stream;
    std::vector<int32_t> rp, ci, map, vrow;
    // rows longer than a team pass (P2): segmented pattern, one team pass per chunk; else the plain compact pattern
    const int T = c->spmv_team;
    bool seg = false;
    if ((T == 8 || T == 16) && c->hs.max_row - 1 > 2 * T) {
        const int rc = host_build_solver_pattern_seg(c->hs, v == 1, 2 * T, (64 / T) * 4, rp, ci, map, vrow);
        if (rc == FDAPDE_OK) seg = true;
        else if (rc != FDAPDE_EUNSUPPORTED) return rc;
    }
    if (!seg)
        if (int rc = host_build_solver_pattern(c->hs, v == 1, rp, ci, map)) return rc;
    const int64_t n_csr = (int64_t)rp.size() - 1;   // rows of the CSR arrays (virtual rows when segmented)
    c->sp_nv[v] = seg ? n_csr : 0, c->sp_team = T;
    if (seg) HIPCHK(c, c->sp_vrow[v].upload(vrow.data(), vrow.size(), st));
    if ((size_t)rp.back() + 2 > c->sval.n) HIPCHK(c, c->sval.alloc((size_t)rp.back() + 2));   // pad entries may exceed nnz
    c->sval_layout = -2;
    HIPCHK(c, c->sp_rowptr[v].upload(rp.data(), rp.size(), st));
    HIPCHK(c, c->sp_colidx[v].upload(ci.data(), ci.size(), st));
    HIPCHK(c, c->sp_map[v].upload(map.data(), map.size(), st));
    {   // 16-bit column codes of the same pattern
        std::vector<uint16_t> code;
        std::vector<int32_t> tb;
        if (int rc = host_build_col16(n_csr, rp, ci, code, tb, &c->sp_wide[v])) return rc;
        HIPCHK(c, c->sp_col16[v].upload(code.data(), code.size(), st));
        HIPCHK(c, c->sp_tbase[v].upload(tb.data(), tb.size(), st));
        if (std::getenv("FDAPDE_DEBUG_SETUP"))
            std::fprintf(stderr, "solver pattern %d: %lld entries in %lld %srows, %lld of %lld row groups wide\n", v, (long long)rp.back(),
                         (long long)n_csr, seg ? "virtual " : "", (long long)c->sp_wide[v], (long long)((n_csr + kCodeRows - 1) / kCodeRows));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    c->sp_nnz[v] = rp.back(), c->sp_built[v] = true;
    return FDAPDE_OK;
}

// blocked-ELL layout of the multi-launch SpMV for boundary variant v (k_spmv_blocked), built on the device from the pattern
int build_blocked(fdapde_ctx* c, int v) {
    fdapde_ctx::Blocked& bk = c->bk[v];
    if (bk.tried) return FDAPDE_OK;
    bk.tried = true, bk.ok = false;
    const char* mode = std::getenv("FDAPDE_SETUP");
    if (mode && std::strcmp(mode, "host") == 0) return FDAPDE_OK;   // (no host builder for this layout: the compact CSR path serves)
    PersistLayout pl;
    DevPersist dp;
    // rows per block, measured on C5 (P2, 28 entries per row; CSR kernel 400 us per SpMV): 1024 -> 375 us, 2048 -> 367, 4096 -> 387, 8192 -> 439
    int rows = 2048;
    if (const char* e = std::getenv("FDAPDE_BLOCKED_ROWS")) rows = std::atoi(e);
    const int rc = dev_build_persist_layout(c->hs.n_dofs, c->hs.max_row, c->rowptr.p, c->colidx.p, c->bnd.p, v == 1, 1 << 19, 0, rows, nullptr, 0, false, c->stream, pl, &dp,
                                            c->err);
    if (rc == FDAPDE_EUNSUPPORTED) return FDAPDE_OK;
    if (rc) return rc;
    const int S = pl.R * kPersistT;
    bk.imp_cap = (pl.max_imp + 63) & ~63;
    bk.lds_bytes = 8 * (size_t)(S + bk.imp_cap) + 64;
    if (bk.lds_bytes > 150 * 1024) {
        dev_persist_release(&dp);
        return FDAPDE_OK;
    }
    const size_t n_alloc = (size_t)pl.n_entries + 256;
    adopt(bk.slot_dof, dp.slot_dof, (size_t)pl.G * S), adopt(bk.ell_off, dp.ell_off, (size_t)pl.G + 1), adopt(bk.sl_off, dp.sl_off, (size_t)pl.G * (pl.nsl + 1));
    adopt(bk.ell_code, dp.ell_code, n_alloc), adopt(bk.ell_src, dp.ell_src, n_alloc), adopt(bk.imp_off, dp.imp_off, (size_t)pl.G + 1);
    adopt(bk.imp_dof, dp.imp_pos, (size_t)(pl.n_imp ? pl.n_imp : 1)), adopt(bk.drop_dof, dp.drop_dof, (size_t)(pl.n_drop ? pl.n_drop : 1));
    dev_persist_release(&dp);
    HIPCHK(c, bk.ell_val.alloc(n_alloc));
    HIPCHK(c, hipMemsetAsync(bk.ell_val.p, 0, sizeof(double) * n_alloc, c->stream));
    if (2 * (size_t)pl.G > c->part_a.n) HIPCHK(c, c->part_a.alloc(2 * (size_t)pl.G));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (std::getenv("FDAPDE_DEBUG_SETUP"))
        std::fprintf(stderr, "blocked-ELL SpMV layout %d: %d workgroups x %d rows/thread, %lld interior rows, %lld entries (%lld stored, %.1f %% padding), "
                     "LDS %zu B, imports <= %d (%lld in all)\n", v, pl.G, pl.R, (long long)pl.n_int, (long long)pl.n_entries, (long long)pl.nnz,
                     100.0 * (double)(pl.n_entries - pl.nnz) / (double)(pl.n_entries > 0 ? pl.n_entries : 1), bk.lds_bytes, pl.max_imp, (long long)pl.n_imp);
    bk.meta = std::move(pl);
    bk.filled = false, bk.ok = true;
    c->drop_prepared("the blocked-ELL layout was built again");
    return FDAPDE_OK;
}

// Dirichlet reduction + Jacobi scaling of the system matrix A (internal slots): scale, sval = diag(s) A diag(s).
// Done once per matrix (once for all time steps of the parabolic problem; for the elliptic one once per assembled matrix: `reuse`, fdapde_solve's
// first prepare of a call, is served from the context's prepared-system record while nothing has made it stale -- fdapde_ctx::Prepared).
int solve_prepare(fdapde_ctx* c, const double* A, int use_bnd, SolveState* ss, bool symmetric, bool allow_defer = false, bool reuse = false) {
    const int64_t n = c->hs.n_dofs;
    hipStream_t st = c->stream;
    if (!reuse) c->drop_prepared("another solver, or a later stage of the same solve, prepared a system in the shared buffers");
    ss->dist = (c->comm != nullptr || c->ar_fn != nullptr) && c->halo_ready;   // multi-GPU: sub-assembled operator of this rank's cells
    ss->owned = ss->dist ? c->owned.p : nullptr;
    ss->use_bnd = use_bnd, ss->symmetric = symmetric;
    ss->rowdist = (c->comm != nullptr || c->ar_fn != nullptr) && c->rd.ready && !ss->dist;
    if (ss->rowdist) ss->owned = c->rd.owned.p;
    // small systems on one GPU (the sizes the reference is used at: a 289-DOF solve is a 130 us launch inside 250 us of wall time): no wait for
    // the "every interior diagonal is positive" flag -- it is raised at ctl[4] and read back with the solve's outcome; the solve goes ahead as if
    // the diagonal were positive (what an assembled elliptic operator has) and fdapde_solve repeats it the slow way in the rare other case
    ss->diag_deferred = allow_defer && !ss->dist && !ss->rowdist && c->small_rows > 0 && n <= c->small_rows && c->comm == nullptr && c->ar_fn == nullptr;
    int32_t* diag_flag = c->ctl.p + (ss->diag_deferred ? 4 : 3);
    ss->front_pending = false, ss->front_A = A;
    // ... and the smallest of them (one workgroup): flag reset, scale and fill are left to k_small_front (solve_run), if the layout turns out to be one it takes
    bool front_candidate = ss->diag_deferred && (symmetric || c->persist_bicg) && c->small_front_rows > 0 && n <= c->small_front_rows && A == c->vals[FDAPDE_MAT_STIFF].p &&
                           c->stiff_stat_valid && c->persist && !c->persist_broken;
    // the system the record describes, again: scale, the scaled copy and the filled layout are in place bit for bit, and its diagonal was seen positive
    const bool may_record = reuse && c->solve_reuse && !ss->dist && !ss->rowdist && c->comm == nullptr && c->ar_fn == nullptr && c->group == nullptr;
    if (reuse) {
        const fdapde_ctx::Prepared& pr = c->prep;
        const char* miss = nullptr;
        if (!c->solve_reuse) miss = "knob solve_reuse is 0";
        else if (!may_record) miss = "a rank of a multi-GPU job prepares with the others";
        else if (front_candidate) miss = "a one-workgroup system: its front kernel scales and fills";
        else if (c->persist_broken) miss = "the single launch is on hold after a timeout";   // (its retry countdown belongs to the full prepare)
        else if (!pr.valid) miss = pr.why;
        else if (pr.A != A || pr.init_count != c->init_count) miss = "the matrix was assembled again";
        else if (pr.use_bnd != use_bnd) miss = "Dirichlet data were set or removed";
        else if (pr.symmetric != symmetric) miss = "the Krylov stage changed (CG <-> BiCGStab)";
        if (std::getenv("FDAPDE_DEBUG_SETUP"))
            std::fprintf(stderr, "solve_prepare: prepared system %s%s%s\n", miss ? "MISS (" : "HIT", miss ? miss : "", miss ? ")" : "");
        if (!miss) {   // what a solve needs afresh: its control words
            HIPCHK(c, hipMemsetAsync(c->ctl.p, 0, 8 * sizeof(int32_t), st));
            c->h_ctl[3] = 0;
            ss->diag_deferred = false, ss->diag_positive = true;
            c->persist_plain = symmetric ? 0 : 1;   // (fdapde_solver_prepare may have set it from the operator in between)
            ++c->prep_hits;
            return FDAPDE_OK;
        }
        c->drop_prepared(miss);
    }
    c->sval_stale = false;
    if (!front_candidate) HIPCHK(c, hipMemsetAsync(c->ctl.p, 0, 8 * sizeof(int32_t), st));
    if (front_candidate) {
    } else if (ss->dist) {   // the diagonal is a sum over the ranks sharing a DOF
        hipLaunchKernelGGL(k_diag_extract, dim3(g1(n)), dim3(256), 0, st, n, c->diag.p, A, c->tmp_i.p);
        if (int rc = halo_sum(c, c->tmp_i.p, nullptr, 0)) return rc;
        hipLaunchKernelGGL(k_jacobi_scale_from_diag, dim3(g1(n)), dim3(256), 0, st, n, c->tmp_i.p, c->bnd.p, use_bnd, c->scale.p,
                           c->ctl.p + 3);
    } else {
        if (A == c->vals[FDAPDE_MAT_STIFF].p && c->stiff_stat_valid)   // (diagonal, row maximum) left by fdapde_init's sweep: same numbers, 16 B per row
            hipLaunchKernelGGL(k_jacobi_scale_stats, dim3(g1(n)), dim3(256), 0, st, n, c->stiff_stat.p, c->bnd.p, use_bnd, c->scale.p, diag_flag);
        else
            hipLaunchKernelGGL(k_jacobi_scale, dim3(g1(n * 16)), dim3(256), 0, st, n, c->rowptr.p, c->diag.p, A, c->bnd.p, use_bnd, c->scale.p, diag_flag);
    }
    if (ss->diag_deferred) {
        c->h_ctl[3] = 0;
    } else {
        HIPCHK(c, hipMemcpyAsync(c->h_ctl, c->ctl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    if (ss->dist || ss->rowdist) {   // "positive diagonal" (CG admissible) must be ONE decision for all ranks: sum the per-rank flags
        c->h_sc[8] = (double)c->h_ctl[3];
        HIPCHK(c, hipMemcpyAsync(c->sbuf.p + 2, c->h_sc + 8, sizeof(double), hipMemcpyHostToDevice, st));
        if (int rc = allreduce_sum(c, c->sbuf.p + 2, 1)) return rc;
        HIPCHK(c, hipMemcpyAsync(c->h_sc + 8, c->sbuf.p + 2, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->h_ctl[3] = c->h_sc[8] != 0.0 ? 1 : 0;
    }
    ss->diag_positive = c->h_ctl[3] == 0;
    if (ss->rowdist) {
        // row-distributed form: this rank's rows are complete (its sub-mesh holds every cell touching an owned DOF), the columns other
        // ranks own take their Jacobi scale from the owner; the whole CG then runs as one launch per rank on a layout of its own
        c->ps[0].filled = c->ps[1].filled = false, c->bk_cur = -1, c->bk[0].filled = c->bk[1].filled = false;
        if (!ss->diag_positive) return fail(c, FDAPDE_EUNSUPPORTED, "the row-distributed solve needs a positive diagonal (Jacobi scaling)");
        const int v = use_bnd ? 1 : 0;
        c->persist_plain = symmetric ? 0 : 1;
        if (int rc = build_rowdist(c, v)) return rc;
        if (c->rd.lay[v].ok && !symmetric && (c->rd.lay[v].ps.meta.sym || c->rd.lay[v].ps.meta.R > 8))
            return fail(c, FDAPDE_EUNSUPPORTED, "the row-distributed BiCGStab needs plain storage and at most 8 rows per thread (layout built for a symmetric operator? re-create the context)");
        if (!c->rd.lay[v].ok) return fail(c, FDAPDE_EUNSUPPORTED, "the row-distributed solve does not take this system (a rank's share needs more than 8 rows per thread, or its lists do not fit)");
        if (int rc = rowdist_import_ghosts(c, v, c->scale.p)) return rc;
        hipLaunchKernelGGL(k_scale_matrix, dim3(g1(n * 16)), dim3(256), 0, st, n, c->rowptr.p, c->colidx.p, A, c->scale.p, c->sval.p);
        c->sp_cur = -1, c->sval_layout = -2;
        if (int rc = fill_rowdist(c, v)) return rc;
        HIPCHK(c, hipGetLastError());
        return FDAPDE_OK;
    }
    // scaled matrix: compact (no diagonal, no Dirichlet rows / columns: ~12 % fewer entries on C3) when every interior
    // diagonal is positive, so that the scaled diagonal is exactly 1; else the full pattern
    // symmetric positive system on one GPU of at most ~2 M interior rows: the solve will run as ONE persistent launch on its own
    // resident layout (kernels_persist.h); the multi-launch kernels then only serve the lift, warm starts and the fall-back, and
    // take the plain full-pattern scaled matrix (no compact pattern / column codes are built for such a system)
    c->ps[0].filled = c->ps[1].filled = false;
    bool persist = false;
    if (c->persist_broken && --c->persist_retry_in <= 0) c->persist_broken = false;   // the contention that broke it may be over
    // symmetric: the single launch is a CG (kernels_persist.h); non-symmetric: a BiCGStab on the plain storage (kernels_persist_bicg.h: six
    // vectors in registers, so at most 8 rows per thread -- larger systems keep the multi-launch BiCGStab)
    c->persist_plain = symmetric ? 0 : 1;
    if ((symmetric || c->persist_bicg) && ss->diag_positive && !ss->dist && c->persist && !c->persist_broken) {
        if (int rc = build_persist(c, use_bnd ? 1 : 0)) return rc;
        const fdapde_ctx::Persist& ps = c->ps[use_bnd ? 1 : 0];
        persist = ps.ok && (symmetric || (!ps.meta.sym && ps.meta.R <= 8));
    }
    if (front_candidate) {
        const fdapde_ctx::Persist& ps = c->ps[use_bnd ? 1 : 0];
        if (persist && ps.meta.G == 1 && !ps.meta.sym && ps.ell_col.n >= (size_t)ps.meta.n_entries + 256) {
            ss->front_pending = true;
        } else {   // not this time (e.g. the layout's column table is made by its first fill): the separate launches after all
            front_candidate = false;
            HIPCHK(c, hipMemsetAsync(c->ctl.p, 0, 8 * sizeof(int32_t), st));
            hipLaunchKernelGGL(k_jacobi_scale_stats, dim3(g1(n)), dim3(256), 0, st, n, c->stiff_stat.p, c->bnd.p, use_bnd, c->scale.p, diag_flag);
        }
    }
    // one GPU, positive diagonal, not taken by the persistent CG (non-symmetric operator, or too many rows): the multi-launch
    // kernels apply the operator from the blocked-ELL layout (k_spmv_blocked); the compact CSR pattern is then not built either
    c->bk_cur = -1, c->bk[0].filled = c->bk[1].filled = false;
    bool blocked = false;
    // ... where it pays: long rows (P2).  On 14-entry rows (C3 with the persistent CG switched off) the CSR kernel's finer-grained,
    // software-pipelined workgroups win (45 us against 48-51 us per SpMV), so short-row systems keep the compact CSR pattern.
    // Round 6: ... up to the size where the single launch ends (3.1 M rows on 256 CUs).  Above it every operator application streams from HBM and the
    // blocked form wins on short rows too -- 3-D P1, 8.1 M DOFs: 238 us against 281 us per SpMV, 0.67 against 0.56 of the HBM peak on the layout's own
    // bytes (tools/large_ab.py, profiles/r6_large_ab.txt).
    const bool long_rows = (double)c->hs.nnz >= 20.0 * (double)n || c->blocked == 2 || n > kBlockedShortRowsAbove;
    if (!persist && ss->diag_positive && !ss->dist && c->blocked && long_rows) {
        if (int rc = build_blocked(c, use_bnd ? 1 : 0)) return rc;
        blocked = c->bk[use_bnd ? 1 : 0].ok;
    }
    const bool compact = !persist && !blocked && ss->diag_positive;
    if (compact) {
        const int v = use_bnd ? 1 : 0;
        if (int rc = build_solver_pattern(c, v)) return rc;
        if (c->sval_layout != v) {   // entries no full-pattern entry maps to (padding of a segmented pattern) must read 0
            HIPCHK(c, hipMemsetAsync(c->sval.p, 0, sizeof(double) * c->sval.n, st));
            c->sval_layout = v;
        }
        hipLaunchKernelGGL(k_scale_matrix_compact, dim3(g1(n * 16)), dim3(256), 0, st, n, c->rowptr.p, c->colidx.p, A, c->scale.p,
                           c->sp_map[v].p, c->sval.p);
        c->sp_cur = v;
    } else if (persist && (c->persist_fill_fused || ss->diag_deferred)) {   // the launch's blocks are filled straight from A (fill_persist_scaled): no scaled copy
                                                                           // now (small systems: one launch less in front of the solve; ensure_sval makes it on demand)
        c->sval_stale = true, c->sval_A = A;
        c->sp_cur = -1, c->sval_layout = -2;
    } else {
        hipLaunchKernelGGL(k_scale_matrix, dim3(g1(n * 16)), dim3(256), 0, st, n, c->rowptr.p, c->colidx.p, A, c->scale.p, c->sval.p);
        c->sp_cur = -1, c->sval_layout = -2;
    }
    if (blocked) {
        const int v = use_bnd ? 1 : 0;
        if (c->bk[v].meta.n_entries > 0)
            hipLaunchKernelGGL(k_persist_fill, dim3((unsigned)((c->bk[v].meta.n_entries + 1023) / 1024)), dim3(256), 0, st, c->bk[v].meta.n_entries, c->bk[v].ell_src.p,
                           c->sval.p, c->bk[v].ell_val.p, (unsigned long long*)nullptr);
        c->bk[v].filled = true, c->bk_cur = v;
    }
    if (persist && ss->front_pending) c->ps[use_bnd ? 1 : 0].filled = true;   // (by k_small_front, in stream order before the launch)
    else if (persist)
        if (int rc = c->sval_stale ? fill_persist_scaled(c, use_bnd ? 1 : 0, A) : fill_persist(c, use_bnd ? 1 : 0)) return rc;
    HIPCHK(c, hipGetLastError());
    if (may_record && !ss->front_pending && ss->diag_positive && !c->persist_broken) {   // (a non-positive diagonal is never kept)
        fdapde_ctx::Prepared& pr = c->prep;
        pr.A = A, pr.init_count = c->init_count, pr.use_bnd = use_bnd, pr.symmetric = symmetric;
        pr.pending = ss->diag_deferred, pr.valid = !ss->diag_deferred;   // (deferred: fdapde_solve confirms it once it has read the flag)
    }
    return FDAPDE_OK;
}

// the scaled full-pattern copy of the current system, if solve_prepare left it out (single-launch solve)
int ensure_sval(fdapde_ctx* c) {
    if (!c->sval_stale) return FDAPDE_OK;
    const int64_t n = c->hs.n_dofs;
    hipLaunchKernelGGL(k_scale_matrix, dim3(g1(n * 16)), dim3(256), 0, c->stream, n, c->rowptr.p, c->colidx.p, c->sval_A, c->scale.p, c->sval.p);
    HIPCHK(c, hipGetLastError());
    c->sval_stale = false;
    return FDAPDE_OK;
}

// "CG broke down" (p.Ap <= 0) can only be said of a CG: the breakdown word of a BiCGStab or GMRES stage that followed means something else
static inline bool is_cg_method(int m) { return m == FDAPDE_SOLVER_CG || m == FDAPDE_SOLVER_CG_SR || m == FDAPDE_SOLVER_CG_FUSED; }

namespace {

// ---- what fdapde_solve, the parabolic stepper and the handle's solve say and decide alike -------------------------------------------------

// (the outcome of a Krylov run -- Outcome, outcome_of, outcome_from -- and bare_answer / dense_singular: engine.h, shared with the operator handles)
// the scalars of the run into h_sc -- with the stop flag, the iteration count and the breakdown word into h_ctl unless h_ctl holds them already -- and the wait
int read_outcome(fdapde_ctx* c, bool ctl_too = true) {
    if (ctl_too) HIPCHK(c, hipMemcpyAsync(c->h_ctl, c->ctl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_sc, c->sc.p, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FDAPDE_OK;
}

// the GMRES stage of the open method (solve_run_restarting's gmres_budget): none for a method the caller named, what BiCGStab leaves of a budget the
// caller set, else the default budget of its own
inline int open_gmres_budget(const fdapde_ctx* c, const fdapde_options* opt, int64_t n) {
    const bool open_method = !opt || opt->method == FDAPDE_SOLVER_AUTO;
    return !open_method ? -1 : ((opt && opt->maxit > 0) ? 0 : default_maxit(c, n));
}

// "CG broke down where the method was left open" -- a turn the ranks of a multi-GPU job take TOGETHER: the breakdown word comes out of sums every rank
// holds bit for bit, and the ranks say so to each other before any of them re-prepares (a rank that disagreed would leave the others in the
// collectives of the second solve).  rc: what the CG stage returned; disagree: the caller's text for ranks that do not agree
int cg_breakdown_agreed(fdapde_ctx* c, const SolveState& ss, int rc, bool open_method, const char* disagree, bool* broke) {
    *broke = rc == FDAPDE_ENOCONV && c->h_ctl[2] != 0 && open_method && is_cg_method(c->info.method_used);
    if ((ss.dist || ss.rowdist) && open_method && (rc == FDAPDE_OK || rc == FDAPDE_ENOCONV)) {
        int yes = 0;
        if (int rc2 = ranks_saying_yes(c, *broke, &yes)) return rc2;
        if (yes != 0 && yes != c->world) return fail(c, FDAPDE_ERCCL, disagree);
        *broke = yes == c->world;
    }
    return FDAPDE_OK;
}

// FDAPDE_SOLVER_DENSE by name: the refusal of a system it does not take
constexpr const char* kDenseRefusal = "FDAPDE_SOLVER_DENSE takes one-GPU systems of up to `dense_rows` (at most 8192) DOFs";

}   // namespace

// Restarted GMRES(m) on the scaled system (kernels_gmres.h); x, r, sc, ctl as k_krylov_init / _fin left them, bt = the scaled right-hand side.
// Leaves x (scaled iterate), sc[0] / sc[3] (|b|^2, |b - A x|^2 TRUE) and ctl like the other methods; h_ctl / h_sc hold the last read-back.
int run_gmres(fdapde_ctx* c, double tol2, int maxit) {
    const int64_t n = c->hs.n_dofs;
    const int m = c->gmres_m;
    hipStream_t st = c->stream;
    HIPCHK(c, c->gm_V.alloc((size_t)(m + 1) * (size_t)n));
    HIPCHK(c, c->gm_s.alloc((size_t)gm_state_doubles(m) + (size_t)m + 2));
    const int vg = c->vec_grid;
    // [(m + 1) x kGmStripes stripes of V^T w | one |w|^2 partial per workgroup of the vector kernels]: vec_grid goes up to 1024 workgroups
    // (systems above 65 536 DOFs), the true-residual partials of k_gm_residual need as many from the start of the buffer
    const size_t gm_norm_at = (size_t)(m + 1) * kGmStripes;
    HIPCHK(c, c->gm_part.alloc(gm_norm_at + (size_t)std::max(vg, kGmStripes)));
    double* gm_norm = c->gm_part.p + gm_norm_at;
    double* gs = c->gm_s.p;
    double* h_pass = gs + gm_state_doubles(m);   // coefficients of the Gram-Schmidt pass in flight
    double* hcol = gs + 3 * m + 1;
    double* w = c->y.p;
    HIPCHK(c, hipMemsetAsync(c->ctl.p + 5, 0, sizeof(int32_t), st));   // the stall counter of k_gm_cycle_fin (a word of its own: ctl[3] belongs to the Jacobi scaling / the single launch)
    HIPCHK(c, hipMemcpyAsync(c->sc.p + 21, c->sc.p + 3, sizeof(double), hipMemcpyDeviceToDevice, st));   // |r|^2 at the start of the first cycle
    bool stop = false;
    HIPCHK(c, hipMemcpyAsync(c->h_ctl, c->ctl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    stop = c->h_ctl[0] != 0;   // (converged at the initial guess)
    while (!stop) {
        hipLaunchKernelGGL(k_gm_cycle_init, dim3(vg), dim3(256), 0, st, n, m, c->r.p, c->sc.p, gs, c->gm_V.p, c->ctl.p);
        for (int j = 0; j < m; ++j) {
            const double* vj = c->gm_V.p + (size_t)j * n;
            launch_spmv(c, c->sval.p, vj, w, nullptr, c->part_a.p, c->ctl.p);   // w = At v_j (leaves at once when the stop flag is up)
            for (int pass = 0; pass < 2; ++pass) {                              // classical Gram-Schmidt, twice
                hipLaunchKernelGGL(k_gm_dots, dim3(kGmStripes, j + 1), dim3(256), 0, st, n, c->gm_V.p, w, c->gm_part.p, c->ctl.p);
                hipLaunchKernelGGL(k_gm_reduce, dim3(j + 1), dim3(256), 0, st, c->gm_part.p, h_pass, hcol, pass, c->ctl.p);
                hipLaunchKernelGGL(k_gm_axpy, dim3(vg), dim3(256), 0, st, n, j + 1, c->gm_V.p, h_pass, w, gm_norm, pass, c->ctl.p);
            }
            hipLaunchKernelGGL(k_gm_hess, dim3(1), dim3(256), 0, st, j, m, gm_norm, vg, gs, c->sc.p, c->ctl.p, tol2, maxit);
            hipLaunchKernelGGL(k_gm_next, dim3(vg), dim3(256), 0, st, n, w, gs, m, c->gm_V.p + (size_t)(j + 1) * n, c->ctl.p);
            if (j % 10 == 9 && j + 1 < m) {   // a look at the stop flag every ten steps: the rest of a cycle whose estimate has converged (or whose
                                              // budget is spent) would be ~8 empty launches per step
                HIPCHK(c, hipMemcpyAsync(c->h_ctl, c->ctl.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
                if (c->h_ctl[0] != 0) break;
            }
        }
        // end of the cycle: y, x += V y, the true residual -- which decides whether another cycle follows
        hipLaunchKernelGGL(k_gm_solve_y, dim3(1), dim3(1), 0, st, m, gs);
        hipLaunchKernelGGL(k_gm_update_x, dim3(vg), dim3(256), 0, st, n, m, c->gm_V.p, gs, c->x.p);
        launch_spmv(c, c->sval.p, c->x.p, c->t.p, nullptr, nullptr, nullptr);
        hipLaunchKernelGGL(k_gm_residual, dim3(vg), dim3(256), 0, st, n, c->gm_b.p, c->t.p, c->r.p, c->gm_part.p);
        hipLaunchKernelGGL(k_gm_cycle_fin, dim3(1), dim3(256), 0, st, c->gm_part.p, vg, c->sc.p, c->ctl.p, tol2, maxit);
        HIPCHK(c, hipGetLastError());
        if (int rc = read_outcome(c)) return rc;
        stop = c->h_ctl[0] != 0;
    }
    return FDAPDE_OK;
}

// ---- the stages of solve_run: file-local, in the order solve_run calls them -------------------------------------------------------------------
namespace {

// Which method runs: what the caller asked for, resolved against what solve_prepare found and the platform -- or a refusal with its text
struct MethodChoice { int method, refusal; const char* why; };
MethodChoice resolve_method(int asked, const SolveState& ss, bool op_symmetric, int world) {
    int m = asked;
    if (ss.rowdist) {
        // (warm starts: the caller's initial guess must hold the owners' values at the ghost columns -- the parabolic stepper imports them
        //  after every step, rowdist_import_ghosts)
        if (m == FDAPDE_SOLVER_CG_SR) return {m, FDAPDE_EUNSUPPORTED, "the row-distributed solve runs the fused-update CG or BiCGStab"};
        m = (m == FDAPDE_SOLVER_BICGSTAB || !ss.symmetric) ? FDAPDE_SOLVER_BICGSTAB : FDAPDE_SOLVER_CG_FUSED;
    }
    if (m == FDAPDE_SOLVER_AUTO)   // symmetric + positive diagonal: CG (fused-update form on one GPU, single-reduction form on several)
        m = (op_symmetric && ss.diag_positive) ? (ss.dist ? FDAPDE_SOLVER_CG : FDAPDE_SOLVER_CG_FUSED) : FDAPDE_SOLVER_BICGSTAB;
    if (m == FDAPDE_SOLVER_CG && ss.dist && world > 1) m = FDAPDE_SOLVER_CG_SR;   // one all-reduce per iteration
    if (m == FDAPDE_SOLVER_CG_FUSED && ss.dist) m = FDAPDE_SOLVER_CG_SR;         // y.y of the assembled y would need its own all-reduce
    if (is_cg_method(m) && !ss.diag_positive) return {m, FDAPDE_ENOCONV, "CG needs a positive diagonal (operator not SPD?); use BiCGStab"};
    if (m == FDAPDE_SOLVER_GMRES && (ss.dist || ss.rowdist)) return {m, FDAPDE_EUNSUPPORTED, "GMRES runs on one-GPU contexts"};
    return {m, FDAPDE_OK, nullptr};
}

// Grid of the fused update kernels (k_cgf_update, V elements per lane; k_cgsr_update, kCgV): one workgroup per 256 V double2 elements -- with the
// XCD-aware mapping (knob cgf_band) of the elements of each of the SpMV's eight row bands, workgroup b serving band b % 8
struct UpdateGrid {
    int64_t band2;   // double2 elements of a row band; 0: no bands
    int grid;
};
inline UpdateGrid update_grid(int64_t n, int V, int cgf_band) {
    const int64_t band2 = cgf_band ? (((((n + 7) / 8) + 31) & ~int64_t(31)) >> 1) : 0, span = band2 > 0 ? band2 : (n >> 1);
    const int per = std::max(1, (int)((span + 256 * V - 1) / (256 * V)));
    return {band2, band2 > 0 ? 8 * per : per};
}

struct EventPair { hipEvent_t e0, e1; };
template <typename F> void by_cgf_v(int V, F&& f) {
    switch (V) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
    }
}
// Phase statistics of the single launch into c->info: stamps of every workgroup (s_memrealtime ticks of 10 ns).  The operator application of an
// iteration is complete when the SLOWEST workgroup has its rows: spmv_avg_ms = max over workgroups of their average operator phase (SpMV + import
// wait); the mean over workgroups is reported next to it; all-gather (which contains the wait for the slowest) and update: means
void persist_phase_stats(fdapde_ctx* c, int v) {
    if (c->persist_host_stats.empty() || !(c->persist_host_stats[0] > 0)) return;
    const size_t G = c->persist_host_stats.size() / 4;
    double mx = 0, mean = 0, gat = 0, upd = 0;
    for (size_t g = 0; g < G; ++g) {
        const double* st = &c->persist_host_stats[4 * g];
        const double n_it = st[0] > 0 ? st[0] : 1;
        mx = std::max(mx, st[1] / n_it), mean += st[1] / n_it, gat += st[2] / n_it, upd += st[3] / n_it;
    }
    if (std::getenv("FDAPDE_DEBUG_PERSIST")) {   // per-workgroup operator phases (us), with the workgroup's ELL entries
        std::vector<int64_t> eo(G + 1);
        std::vector<int32_t> io(G + 1), xo(G + 1);
        (void)hipMemcpy(eo.data(), c->ps[v].ell_off.p, sizeof(int64_t) * (G + 1), hipMemcpyDeviceToHost);
        (void)hipMemcpy(io.data(), c->ps[v].imp_off.p, sizeof(int32_t) * (G + 1), hipMemcpyDeviceToHost);
        (void)hipMemcpy(xo.data(), c->ps[v].exp_off.p, sizeof(int32_t) * (G + 1), hipMemcpyDeviceToHost);
        for (size_t g = 0; g < G; ++g)
            std::fprintf(stderr, "persist wg %zu: operator %.2f us gather %.2f us entries %lld imports %d exports %d\n", g,
                         c->persist_host_stats[4 * g + 1] / std::max(1.0, c->persist_host_stats[4 * g]) * 1e-2,
                         c->persist_host_stats[4 * g + 2] / std::max(1.0, c->persist_host_stats[4 * g]) * 1e-2, (long long)(eo[g + 1] - eo[g]),
                         io[g + 1] - io[g], xo[g + 1] - xo[g]);
    }
    c->info.spmv_avg_ms = mx * 1e-5, c->info.spmv_timed = (int32_t)c->persist_host_stats[0];
    c->info.spmv_mean_ms = mean / (double)G * 1e-5, c->info.gather_avg_ms = gat / (double)G * 1e-5, c->info.update_avg_ms = upd / (double)G * 1e-5;
}

// What the stages of one solve_run share
struct SolveRun {
    fdapde_ctx* c; int64_t n; hipStream_t st; double tol2;   // the context, its rows and stream, rtol^2
    int np_spmv;            // partial pairs the SpMV leaves for the vector kernels: one per workgroup of the kernel that applies the scaled operator
    const uint8_t* owned;
    bool dist, rowdist;
    UpdateGrid upd;         // of the method's fused update (fused-update CG: knob cgf_v elements per lane; single-reduction CG: kCgV)
    int bi_grid;            // of BiCGStab's vector kernels
    hipEvent_t* ev;         // event pairs of the timed iterations: n_timed of them, `timed` handed out so far
    int n_timed, timed;
    int launched;           // iterations enqueued so far (or run by a single launch, by GMRES)
    bool stop;              // the stop flag as last read back

    // the event pair of iteration `it` if it is a timed one (every kTimeStride-th, while pairs are left), else two nulls
    EventPair timed_pair(int it) {
        if (!(timed < n_timed && it % kTimeStride == kTimePhase)) return {nullptr, nullptr};
        const int k = timed++;
        return {ev[2 * k], ev[2 * k + 1]};
    }

    // Start-up: the Dirichlet lift g~ and A g~, the warm start, x / r / p and the scalars of iteration 0 -- as ONE one-workgroup kernel (or two around
    // A g~) for the smallest systems (`front`: solve_prepare's front_pending), with the ranks' sums in between on several GPUs, or as plain launches
    int start_up(const SolveState& ss, bool front, int method, const double* A, const double* f_dev, const double* g_dev, const double* u0_dev) {
        const bool bicg = method == FDAPDE_SOLVER_BICGSTAB, cgf = method == FDAPDE_SOLVER_CG_FUSED;
        const double* fvec = f_dev;
        if (dist) {   // the forcing vector is a sum over the ranks sharing a DOF
            HIPCHK(c, hipMemcpyAsync(c->tmp_e.p, f_dev, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
            if (int rc = halo_sum(c, c->tmp_e.p, nullptr, 0)) return rc;
            fvec = c->tmp_e.p;
        }
        // the lift is zero (no Dirichlet data, or homogeneous data on one GPU -- across ranks the data may differ, and every rank
        // must take the same path through the collectives): A g~ = 0, written by the lift kernel itself (no memset launch)
        const bool zero_lift = !ss.use_bnd || (!dist && !rowdist && g_dev == c->g.p && c->g_zero);
        SmallFrontArgs fa{};
        if (front) {
            const fdapde_ctx::Persist& ps = c->ps[ss.use_bnd ? 1 : 0];
            fa.n = n, fa.use_bnd = ss.use_bnd, fa.zero_y = zero_lift ? 1 : 0, fa.vec_grid = c->vec_grid;
            fa.stat = c->stiff_stat.p, fa.bnd = c->bnd.p, fa.scale = c->scale.p, fa.ctl = c->ctl.p;
            fa.nsl = ps.meta.nsl, fa.ell_off = ps.ell_off.p, fa.sl_off = ps.sl_off.p, fa.slot_dof = ps.slot_dof.p, fa.src = ps.ell_src.p, fa.col = ps.ell_col.p;
            fa.A = ss.front_A, fa.ell_val = ps.ell_val.p;
            fa.g = g_dev, fa.gt = c->gt.p, fa.y = c->y.p, fa.u = c->u.p;
            if (!zero_lift) {
                fa.phases = 1;
                hipLaunchKernelGGL(k_small_front, dim3(1), dim3(256), 0, st, fa);
            }
        } else
            hipLaunchKernelGGL(k_lift, dim3(g1(n)), dim3(256), 0, st, n, c->bnd.p, g_dev, ss.use_bnd, c->gt.p, zero_lift ? c->y.p : (double*)nullptr);
        if (!zero_lift) {
            launch_spmv(c, A, c->gt.p, c->y.p, nullptr, nullptr, nullptr);   // y = A g~
            if (dist)
                if (int rc = halo_sum(c, c->y.p, nullptr, 0)) return rc;
        }
        const double* ax = nullptr;
        if (u0_dev) {   // warm start: x = (u0 - g~) / s, r = b~ - At x
            if (int rc = ensure_sval(c)) return rc;
            hipLaunchKernelGGL(k_krylov_init, dim3(c->vec_grid), dim3(256), 0, st, n, fvec, c->y.p, c->scale.p, c->x.p, c->r.p, c->p.p,
                               (double*)nullptr, c->part_b.p, owned, u0_dev, c->gt.p, (const double*)nullptr, 1);
            launch_spmv(c, c->sval.p, c->x.p, c->t.p, nullptr, nullptr, nullptr);
            if (dist)
                if (int rc = halo_sum(c, c->t.p, nullptr, 0)) return rc;
            ax = c->t.p;
        }
        // fused-update CG: its launch 0 reads the explicit r.r from the second half of part_b (seeded by whichever kernel ends the start-up)
        double* seed = cgf ? c->part_b.p + upd.grid : (double*)nullptr;
        const int n_seed = cgf ? upd.grid : 0;
        if (front) {   // (one GPU, cold start: what the two launches of the other branches do)
            fa.phases = zero_lift ? 3 : 2;
            fa.f = fvec, fa.x = c->x.p, fa.r = c->r.p, fa.p = c->p.p, fa.r0 = bicg ? c->r0.p : (double*)nullptr, fa.partial = c->part_b.p, fa.sc = c->sc.p;
            fa.seed = seed, fa.n_seed = n_seed, fa.tol2 = tol2;
            hipLaunchKernelGGL(k_small_front, dim3(1), dim3(256), 0, st, fa);
        } else {
            hipLaunchKernelGGL(k_krylov_init, dim3(c->vec_grid), dim3(256), 0, st, n, fvec, c->y.p, c->scale.p, c->x.p, c->r.p, c->p.p,
                               bicg ? c->r0.p : (double*)nullptr, c->part_b.p, owned, u0_dev, c->gt.p, ax, 0);
            if (dist || rowdist) {
                hipLaunchKernelGGL(k_reduce_partials2, dim3(1), dim3(256), 0, st, c->part_b.p, c->vec_grid, c->sbuf.p);
                if (int rc = allreduce_sum(c, c->sbuf.p, 2)) return rc;
                hipLaunchKernelGGL(k_krylov_init_fin, dim3(1), dim3(256), 0, st, c->sbuf.p, 1, c->sc.p, c->ctl.p, tol2, (double*)nullptr, 0);
            } else
                hipLaunchKernelGGL(k_krylov_init_fin, dim3(1), dim3(256), 0, st, c->part_b.p, c->vec_grid, c->sc.p, c->ctl.p, tol2, seed, n_seed);
        }
        if (method == FDAPDE_SOLVER_GMRES) {   // the scaled right-hand side, for the true residual at the end of every restart cycle (c->y still holds A g~)
            HIPCHK(c, c->gm_b.alloc((size_t)n));
            hipLaunchKernelGGL(k_gm_rhs, dim3(g1(n)), dim3(256), 0, st, n, fvec, c->y.p, c->scale.p, c->gm_b.p);
        }
        if (method == FDAPDE_SOLVER_CG_SR) {   // p = s = 0 before the first update (beta = 0 there)
            HIPCHK(c, hipMemsetAsync(c->p.p, 0, sizeof(double) * (size_t)n, st));
            HIPCHK(c, hipMemsetAsync(c->s.p, 0, sizeof(double) * (size_t)n, st));
        }
        HIPCHK(c, hipGetLastError());
        return FDAPDE_OK;
    }

    // The whole iteration as ONE launch where the prepared layout takes it (kernels_persist.h: the fused-update CG; kernels_persist_bicg.h: BiCGStab on
    // plain storage of at most 8 rows per thread); it leaves sc / ctl as the chunk loop would.  *ran = false: not a system for it, or the launch gave up
    int single_launch(const SolveState& ss, bool bicg, int maxit, bool* ran) {
        const int v = ss.use_bnd ? 1 : 0;
        const fdapde_ctx::Persist& ps = c->ps[v];
        *ran = false;
        if (dist || rowdist || !c->persist || c->persist_broken || !ps.ok || !ps.filled) return FDAPDE_OK;
        if (bicg && (!c->persist_bicg || ps.meta.sym || ps.meta.R > 8)) return FDAPDE_OK;
        DebugClock clk;
        // the epilogue kernel (and, for fdapde_solve, the end-of-solve event) is enqueued BEHIND the launch before the host waits for it: one wait
        // for launch, outcome and solution together; if the launch gave up, the chunk loop's epilogue redoes it from its own iterate
        c->persist_tail = [this]() -> int {
            if (!c->tail_in_launch) hipLaunchKernelGGL(k_unscale, dim3(g1(n)), dim3(256), 0, st, n, c->scale.p, c->persist_x.p, c->gt.p, c->u.p);
            if (c->ev1_at_end) HIPCHK(c, hipEventRecord(c->ev1, st));
            return FDAPDE_OK;
        };
        const int rc = run_persist(c, v, tol2, maxit, ran, bicg);
        c->persist_tail = nullptr;
        if (rc) return rc;
        clk.mark("solve_run: run_persist");
        if (!*ran) c->drop_prepared("the single launch gave up (persist_broken) or its layout does not launch");   // (a retry goes through a full prepare)
        return FDAPDE_OK;
    }

    // ---- one iteration of each multi-launch method, enqueued; `it` counts from the start of this solve_run ---------------------------------------

    // fused-update CG: SpMV (p.y, y.y) + k_cgf_update; the arguments depend on the iteration's parity only (which a captured chunk relies on)
    void enqueue_cgf(int it, EventPair ev) {
        const int cg = upd.grid;
        launch_spmv(c, c->sval.p, c->p.p, c->y.p, c->p.p, c->part_a.p, c->ctl.p, ev.e0, ev.e1);   // p.y and y.y
        by_cgf_v(c->cgf_v, [&](auto v) {
            hipLaunchKernelGGL((k_cgf_update<decltype(v)::value>), dim3(cg), dim3(256), 0, st, n, c->y.p, c->p.p, c->x.p, c->r.p, c->part_a.p, np_spmv,
                               c->part_b.p + (size_t)((it + 1) & 1) * cg, cg, c->part_b.p + (size_t)(it & 1) * cg, c->sc.p, tol2, c->ctl.p, upd.band2, c->cgf_nt, c->cgf_lazy, it & 1);
        });
    }
    // ... and behind the last update of a chunk: its explicit r.r -> sc[3] / stop flag
    void enqueue_cgf_fin(int done) {
        hipLaunchKernelGGL(k_cgf_fin, dim3(1), dim3(256), 0, st, c->part_b.p + (size_t)((done - 1) & 1) * upd.grid, upd.grid, c->sc.p, tol2, c->ctl.p);
    }

    // single-reduction CG: w = At r with delta = r.(At r) and gamma = r.r (owned rows) fused; multi-GPU: ONE all-reduce carries the interface entries
    // of w and both partials
    int enqueue_cgsr(int it) {
        const EventPair ev = timed_pair(it);
        launch_spmv(c, c->sval.p, c->r.p, c->y.p, c->r.p, c->part_a.p, c->ctl.p, ev.e0, ev.e1, 1, owned);
        const double* part = c->part_a.p;
        int np = np_spmv;
        if (dist) {
            // pack -> all-reduce; the update kernel reads the summed interface rows straight from hbuf (no unpack launch)
            if (int rc = halo_sum(c, c->y.p, c->part_a.p, c->spmv_grid, /*unpack=*/false)) return rc;
            part = c->hbuf.p + c->n_if, np = 1;
        }
        hipLaunchKernelGGL(k_cgsr_update, dim3(upd.grid), dim3(256), 0, st, n, c->r.p, c->y.p, c->p.p, c->s.p, c->x.p, part, np, c->sc.p, it & 1,
                           it == 0 ? 1 : 0, tol2, c->ctl.p, dist ? c->if_slot.p : (const int32_t*)nullptr, dist ? c->hbuf.p : (const double*)nullptr, upd.band2);
        return FDAPDE_OK;
    }

    // CG in the two-kernel form.  Element-partitioned: one all-reduce carries the interface entries of A_p p and the rank's p.Ap partial; a second
    // one (a single double) carries r.r.  Every rank takes the same stop decision from the same numbers.
    int enqueue_cg(int it) {
        const int parity = it & 1, cg = c->cg_grid;
        const EventPair ev = timed_pair(it);
        launch_spmv(c, c->sval.p, c->p.p, c->y.p, c->p.p, c->part_a.p, c->ctl.p, ev.e0, ev.e1);
        if (dist)
            if (int rc = halo_sum(c, c->y.p, c->part_a.p, c->spmv_grid)) return rc;
        hipLaunchKernelGGL(k_cg_update_xr, dim3(cg), dim3(256), 0, st, n, c->y.p, c->r.p, dist ? c->hbuf.p + c->n_if : c->part_a.p, dist ? 1 : np_spmv, c->part_b.p, c->sc.p, parity, c->ctl.p, owned);
        if (dist) {
            hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, st, c->part_b.p, cg, c->sbuf.p);
            if (int rc = allreduce_sum(c, c->sbuf.p, 1)) return rc;
        }
        hipLaunchKernelGGL(k_cg_update_p, dim3(cg), dim3(256), 0, st, n, c->r.p, c->p.p, c->x.p, dist ? c->sbuf.p : c->part_b.p, dist ? 1 : cg, c->sc.p, parity, tol2, c->ctl.p);
        return FDAPDE_OK;
    }

    // BiCGStab on one GPU: the dots ride on the two SpMVs
    int enqueue_bicg(int it) {
        const int bg = bi_grid, np = np_spmv;
        hipLaunchKernelGGL(k_bicg_p, dim3(bg), dim3(256), 0, st, n, c->r.p, c->y.p, c->p.p, c->part_b.p, bg, c->sc.p, it == 0 ? 1 : 0, c->ctl.p);
        const EventPair ev = timed_pair(it);
        launch_spmv(c, c->sval.p, c->p.p, c->y.p, c->r0.p, c->part_a.p, c->ctl.p, ev.e0, ev.e1);   // v = At p, r0.v
        hipLaunchKernelGGL(k_bicg_s, dim3(bg), dim3(256), 0, st, n, c->r.p, c->y.p, c->s.p, c->part_a.p, np, c->sc.p, c->ctl.p);
        launch_spmv(c, c->sval.p, c->s.p, c->t.p, c->s.p, c->part_a.p, c->ctl.p);                 // t = At s, t.s, t.t
        hipLaunchKernelGGL(k_bicg_xr, dim3(bg), dim3(256), 0, st, n, c->p.p, c->s.p, c->t.p, c->r0.p, c->x.p, c->r.p, c->part_a.p, np, c->part_b.p, c->sc.p, c->ctl.p, (const uint8_t*)nullptr);
        hipLaunchKernelGGL(k_bicg_fin, dim3(1), dim3(256), 0, st, c->part_a.p, np, c->part_b.p, bg, c->sc.p, tol2, c->ctl.p);
        return FDAPDE_OK;
    }

    // BiCGStab element-partitioned: every operator application is followed by the interface sum, which also carries the dot fused into the SpMV
    // (w.(A x) needs no weighting); dots of assembled vectors (t.t, r0.r, r.r) count owned rows and cross in two small all-reduces.
    // sbuf: [0..1] = (r0.r, r.r), [4..5] = (t.s, t.t).
    int enqueue_bicg_dist(int it) {
        const int bg = bi_grid;
        hipLaunchKernelGGL(k_bicg_p, dim3(bg), dim3(256), 0, st, n, c->r.p, c->y.p, c->p.p, c->sbuf.p, 1, c->sc.p, it == 0 ? 1 : 0, c->ctl.p);
        const EventPair ev = timed_pair(it);
        launch_spmv(c, c->sval.p, c->p.p, c->y.p, c->r0.p, c->part_a.p, c->ctl.p, ev.e0, ev.e1);
        if (int rc = halo_sum(c, c->y.p, c->part_a.p, c->spmv_grid)) return rc;
        hipLaunchKernelGGL(k_bicg_s, dim3(bg), dim3(256), 0, st, n, c->r.p, c->y.p, c->s.p, c->hbuf.p + c->n_if, 1, c->sc.p, c->ctl.p);
        launch_spmv(c, c->sval.p, c->s.p, c->t.p, c->s.p, c->part_a.p, c->ctl.p);
        if (int rc = halo_sum(c, c->t.p, c->part_a.p, c->spmv_grid)) return rc;
        hipLaunchKernelGGL(k_sq_owned, dim3(c->vec_grid), dim3(256), 0, st, n, c->t.p, owned, c->part_b.p, c->ctl.p);
        hipLaunchKernelGGL(k_bicg_tt_fin, dim3(1), dim3(256), 0, st, c->part_b.p, c->vec_grid, c->hbuf.p + c->n_if, c->sbuf.p + 4);
        if (int rc = allreduce_sum(c, c->sbuf.p + 5, 1)) return rc;
        hipLaunchKernelGGL(k_bicg_xr, dim3(bg), dim3(256), 0, st, n, c->p.p, c->s.p, c->t.p, c->r0.p, c->x.p, c->r.p, c->sbuf.p + 4, 1, c->part_b.p, c->sc.p, c->ctl.p, owned);
        hipLaunchKernelGGL(k_reduce_partials2, dim3(1), dim3(256), 0, st, c->part_b.p, bg, c->sbuf.p);
        if (int rc = allreduce_sum(c, c->sbuf.p, 2)) return rc;
        hipLaunchKernelGGL(k_bicg_fin, dim3(1), dim3(256), 0, st, c->sbuf.p + 4, 1, c->sbuf.p, 1, c->sc.p, tol2, c->ctl.p);
        return FDAPDE_OK;
    }

    // The captured chunk of the fused-update CG (2 * chunk + 1 kernel nodes), made again when anything its launches bake in has changed: the arguments repeat
    // with period 2, so the graph captured for iterations 0 .. chunk-1 serves every even-aligned chunk.  True where c->cg_graph_exec can be replayed
    bool chunk_graph(int chunk) {
        GraphKey key;
        std::memset(&key, 0, sizeof key);   // padding bytes take part in the memcmp below
        key.sval = c->sval.p, key.rowptr = c->sp_cur >= 0 ? (const void*)c->sp_rowptr[c->sp_cur].p : (const void*)c->rowptr.p;
        key.n = n, key.tol2 = tol2, key.chunk = chunk, key.v = c->cgf_v, key.grid = c->spmv_grid, key.team = c->spmv_team;
        key.c16 = c->spmv_c16, key.sp_cur = c->sp_cur;
        // the blocked-ELL layout the captured SpMV nodes read from (its arrays and grid are baked into the graph)
        key.bk_cur = c->bk_cur, key.bk_G = c->bk_cur >= 0 ? c->bk[c->bk_cur].meta.G : 0;
        key.bk_val = c->bk_cur >= 0 ? (const void*)c->bk[c->bk_cur].ell_val.p : nullptr;
        if (c->cg_graph_exec && std::memcmp(&key, &c->cg_graph_key, sizeof key) == 0) return true;
        if (c->cg_graph_exec) (void)hipGraphExecDestroy(c->cg_graph_exec), c->cg_graph_exec = nullptr;
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            for (int it = 0; it < chunk; ++it) enqueue_cgf(it, {nullptr, nullptr});
            enqueue_cgf_fin(chunk);
            if (hipStreamEndCapture(st, &g) == hipSuccess && g && hipGraphInstantiate(&c->cg_graph_exec, g, nullptr, nullptr, 0) == hipSuccess)
                c->cg_graph_key = key;
            else
                c->cg_graph_exec = nullptr;
            if (g) (void)hipGraphDestroy(g);
        }
        (void)hipGetLastError();
        return c->cg_graph_exec != nullptr;
    }

    // The chunk loop of the multi-launch methods: up to check_every iterations enqueued (a full, untimed, even-aligned chunk of the fused-update CG as
    // one graph replay), then the outcome read back and waited for -- until the stop flag is up or maxit iterations are out
    int run_chunks(int method, int maxit, int check_every) {
        const bool cgf = method == FDAPDE_SOLVER_CG_FUSED;
        if (!stop && launched < maxit)   // the multi-launch kernels read the scaled full-pattern copy
            if (int rc = ensure_sval(c)) return rc;
        while (!stop && launched < maxit) {
            const int chunk = (maxit - launched) < check_every ? (maxit - launched) : check_every;
            bool graphed = false;
            if (cgf && c->use_graph && chunk == check_every && (chunk & 1) == 0 && (launched & 1) == 0 && timed >= n_timed)
                if (chunk_graph(chunk) && hipGraphLaunch(c->cg_graph_exec, st) == hipSuccess) launched += chunk, graphed = true, ++c->graph_replays;
            for (int it = 0; !graphed && it < chunk; ++it, ++launched) {
                int rc = FDAPDE_OK;
                switch (method) {
                case FDAPDE_SOLVER_CG_SR: rc = enqueue_cgsr(launched); break;
                case FDAPDE_SOLVER_CG_FUSED: enqueue_cgf(launched, timed_pair(launched)); break;
                case FDAPDE_SOLVER_BICGSTAB: rc = dist ? enqueue_bicg_dist(launched) : enqueue_bicg(launched); break;
                default: rc = enqueue_cg(launched); break;
                }
                if (rc) return rc;
            }
            if (cgf && launched > 0 && !graphed) enqueue_cgf_fin(launched);
            HIPCHK(c, hipGetLastError());
            if (int rc = read_outcome(c)) return rc;
            stop = c->h_ctl[0] != 0;
        }
        return FDAPDE_OK;
    }

    // The end: whatever the method still owes the iterate, u = g~ + s x behind it, the outcome and the timing figures into c->info
    int finish(const SolveState& ss, int method, bool persisted, bool unscaled) {
        if (method == FDAPDE_SOLVER_CG_SR && !stop && launched > 0 && !dist) {
            // single-reduction CG out of iterations: sc[3] is the gamma = r.r its last SpMV measured, the residual BEFORE the last update.  info.relres is
            // the residual of the x that is handed out: r.r of the last update, summed here (r vanishes on the Dirichlet rows).  A run whose LAST
            // permitted update meets rtol therefore reports converged = 1 (the stale gamma said 0: the next SpMV would have seen it).  One GPU only:
            // the element-partitioned form (dist) would need an all-reduce of its own for this and still reports the gamma of before its last update.
            hipLaunchKernelGGL(k_sq_norm, dim3(c->vec_grid), dim3(256), 0, st, n, c->r.p, c->part_b.p);
            hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, st, c->part_b.p, c->vec_grid, c->sc.p + 3);
            HIPCHK(c, hipGetLastError());
            if (int rc = read_outcome(c, /*ctl_too=*/false)) return rc;
        }
        if (launched == 0 && !persisted)   // already converged at the initial guess
            if (int rc = read_outcome(c)) return rc;
        if (method == FDAPDE_SOLVER_CG_FUSED && c->cgf_lazy && !persisted)   // an update of x may still be pending (convergence seen at a poll, or maxit)
            hipLaunchKernelGGL(k_cgf_flush, dim3(c->vec_grid), dim3(256), 0, st, n, c->p.p, c->r.p, c->x.p, c->sc.p, c->ctl.p);
        if (!unscaled) {   // (else c->u already holds the solution: the single launch's epilogue ran behind it)
            hipLaunchKernelGGL(k_unscale, dim3(g1(n)), dim3(256), 0, st, n, c->scale.p, persisted ? c->persist_x.p : c->x.p, c->gt.p, c->u.p);
            HIPCHK(c, hipGetLastError());
            if (c->ev1_at_end) HIPCHK(c, hipEventRecord(c->ev1, st));
            if (!c->defer_end_sync) HIPCHK(c, hipStreamSynchronize(st));   // (h_ctl / h_sc were read back behind a wait of their own)
        }
        const Outcome out = outcome_from(c->h_sc, c->h_ctl, tol2);
        c->info.iters = c->h_ctl[1];
        c->info.relres = out.relres, c->info.converged = out.converged;
        c->info.method_used = method;
        c->info.spmv_avg_ms = 0, c->info.spmv_timed = 0;
        {   // launches after the stop flag return at once; only iterations that really ran are averaged
            int real = 0;   // sample k was iteration k * kTimeStride
            while (real < timed && real * kTimeStride + kTimePhase < c->info.iters) ++real;
            double sum = 0;
            for (int i = 0; i < real; ++i) {
                float t = 0;
                HIPCHK(c, hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]));
                sum += t;
            }
            if (real > 0) c->info.spmv_avg_ms = sum / real, c->info.spmv_timed = real;
        }
        c->info.persistent = persisted ? 1 : 0;
        c->info.launch_ms = persisted ? c->persist_launch_ms : 0.0;
        c->info.gather_avg_ms = c->info.update_avg_ms = c->info.spmv_mean_ms = 0;
        if (persisted) persist_phase_stats(c, ss.use_bnd ? 1 : 0);
        if (!c->info.converged) {
            c->err = c->h_ctl[2] ? "Krylov breakdown (operator not SPD for CG, or BiCGStab rho/omega = 0)" : "maxit reached";
            return FDAPDE_ENOCONV;   // reference: success = false (fem_linear_elliptic_solver.h:42-45)
        }
        return FDAPDE_OK;
    }
};

}   // namespace

// Krylov solve of A u = f with u = g on the Dirichlet DOFs (if ss.use_bnd), on the system prepared by solve_prepare.
//   f_dev : right-hand side, internal order, sub-assembled (summed over ranks here when dist)
//   g_dev : Dirichlet values, internal order (read on boundary DOFs only)
//   u0_dev: initial guess in u-space or nullptr (cold start)
// Result in c->u.  Fills c->info (iters, relres, converged, method_used, spmv timing).
// A refusal (resolve_method: a method the platform or the diagonal does not admit) comes before anything is enqueued: c->gt, c->y and the
// Krylov vectors are left untouched, no collective is entered (every rank refuses alike), and front_pending is never set on a system that is refused.
int solve_run(fdapde_ctx* c, const SolveState& ss, const double* A, const double* f_dev, const double* g_dev, const double* u0_dev,
              int method, double rtol, int maxit, int check_every, int n_timed) {
    // nothing of an earlier solve may be read as this one's outcome by a caller that sees an early return (solve_run_restarting)
    c->h_ctl[0] = c->h_ctl[1] = c->h_ctl[2] = c->h_ctl[3] = 0, c->h_ctl_seen = 4;
    c->info.iters = 0, c->info.method_used = method, c->info.relres = 0, c->info.converged = 0;
    c->graph_replays = 0, c->front_used = false;
    const MethodChoice choice = resolve_method(method, ss, c->op_symmetric, c->world);
    if (choice.refusal) return fail(c, choice.refusal, choice.why);
    method = choice.method;
    const bool bicg = method == FDAPDE_SOLVER_BICGSTAB, cgf = method == FDAPDE_SOLVER_CG_FUSED;
    // the smallest systems (solve_prepare: front_pending): everything in front of the single launch as ONE one-workgroup kernel, or two around A g~
    const bool front = ss.front_pending;
    ss.front_pending = false;
    c->front_used = front;
    const int64_t n = c->hs.n_dofs;
    SolveRun R{};
    R.c = c, R.n = n, R.st = c->stream, R.tol2 = rtol * rtol;
    R.np_spmv = (c->bk_cur >= 0 && !ss.dist) ? c->bk[c->bk_cur].meta.G : c->spmv_grid;
    R.owned = ss.owned, R.dist = ss.dist, R.rowdist = ss.rowdist;
    R.upd = update_grid(n, method == FDAPDE_SOLVER_CG_SR ? kCgV : c->cgf_v, c->cgf_band);
    R.bi_grid = std::max(1, (int)(((n >> 1) + 256 * kBiV - 1) / (256 * kBiV)));
    if (int rc = R.start_up(ss, front, method, A, f_dev, g_dev, u0_dev)) return rc;
    R.n_timed = n_timed < 0 ? 0 : (n_timed > 256 ? 256 : n_timed);
    while ((int)c->ev_spmv.size() < 2 * R.n_timed) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        c->ev_spmv.push_back(e);
    }
    R.ev = c->ev_spmv.data();
    bool persisted = false;   // the iteration ran as one launch (per rank): the iterate is c->persist_x
    bool unscaled = false;    // ... and c->u already holds the solution (the launch's epilogue ran behind it)
    if (method == FDAPDE_SOLVER_GMRES) {
        if (int rc = ensure_sval(c)) return rc;
        if (int rc = run_gmres(c, R.tol2, maxit)) return rc;
        R.stop = true, R.launched = c->h_ctl[1];
        if (int rc = read_outcome(c, /*ctl_too=*/false)) return rc;
    } else if (ss.rowdist) {   // one launch per rank, the launches of all ranks acting as one grid (kernels_persist.h DIST)
        if (int rc = run_rowdist(c, ss.use_bnd ? 1 : 0, R.tol2, maxit, &persisted, bicg)) return rc;
        if (!persisted) return fail(c, FDAPDE_EUNSUPPORTED, "row-distributed solve: an in-kernel hand-off between the ranks' launches timed out (boards not visible across the devices, or a rank's launch could not be resident); use the element-partitioned exchange (fdapde_halo_setup_peers) instead");
        R.stop = true, R.launched = c->h_ctl[1];
    } else if (cgf || bicg) {
        if (int rc = R.single_launch(ss, bicg, maxit, &persisted)) return rc;
        if (persisted) R.stop = true, R.launched = c->h_ctl[1], unscaled = true;
    }
    if (int rc = R.run_chunks(method, maxit, check_every)) return rc;
    return R.finish(ss, method, persisted, unscaled);
}

// solve_run, with a BiCGStab that BROKE DOWN (rho, r0.v or omega exactly 0 -- on advection-dominated operators the recurrences get there --
// or an iterate that stopped being finite) started again from the iterate it had reached: new shadow residual, the stop rule still relative to
// the original right-hand side (solve_run's warm start).  Up to kBicgRestarts times; the iterations add up in info.iters.  One-GPU contexts.
constexpr int kBicgRestarts = 30;
int solve_run_restarting(fdapde_ctx* c, const SolveState& ss, const double* A, const double* f_dev, const double* g_dev, const double* u0_dev,
                         int method, double rtol, int maxit, int check_every, int n_timed, int gmres_budget = -1) {
    // gmres_budget: -1 no GMRES stage (the caller named a method); 0: what BiCGStab left of `maxit` (a budget the caller set is a budget for the whole
    // call); > 0: that many iterations of its own (the default budget, per stage)
    const int64_t n = c->hs.n_dofs;
    // Where the open method has a later stage for this system (the dense direct stage, GMRES) and no budget of the caller's, BiCGStab's own stage is
    // capped at 2 n + 200 iterations instead of the default 10 n: a BiCGStab that has not converged by then has stalled or diverged (cell Peclet numbers
    // of 10^2 - 10^3: relres 1e-3 ... 1e+10 after 10 n iterations, profiles/r5_gmres_probe.txt), and the budget it burnt was most of the call's time
    // (1 089 DOFs, Pe 150: 43 ms of BiCGStab in front of a 10 ms inversion).  CG stages and budgets the caller set are untouched.
    const bool will_bicg = method == FDAPDE_SOLVER_BICGSTAB || (method == FDAPDE_SOLVER_AUTO && !(c->op_symmetric && ss.diag_positive));
    const bool later_stage = gmres_budget > 0 && !ss.dist && !ss.rowdist && (c->auto_gmres || dense_eligible(c));
    if (will_bicg && later_stage) {
        int64_t cap = 2 * n + 200;
        // ... and where that later stage is the dense direct solve, rent or buy: BiCGStab may spend what the inversion will cost (its estimate over ~3 us +
        // n / 700 us per iteration of the single launch: 550 iterations at 1 089 DOFs, 2 100 at 4 225), not more -- a system it has not solved by then
        // is solved directly, and the call costs at most twice the inversion (1 089 DOFs, cell Peclet 150 - 1 000: 20 ms -> 5)
        if (dense_eligible(c)) cap = std::min<int64_t>(cap, std::max<int64_t>(200, (int64_t)(1e3 * dense_build_estimate_ms(n) / (3.0 + (double)n / 700.0))));
        maxit = (int)std::min<int64_t>(maxit, cap);
    }
    int rc = solve_run(c, ss, A, f_dev, g_dev, u0_dev, method, rtol, maxit, check_every, n_timed);
    int total = c->info.iters;
    const bool may_restart = method == FDAPDE_SOLVER_BICGSTAB || method == FDAPDE_SOLVER_AUTO;   // a method named explicitly is never replaced
    // (ranks of a multi-GPU job restart together: breakdown word, iteration count and residual come out of sums all of them hold bit for bit)
    for (int k = 0; k < kBicgRestarts && may_restart && rc == FDAPDE_ENOCONV && c->h_ctl[2] != 0 && c->info.method_used == FDAPDE_SOLVER_BICGSTAB &&
                    total < maxit && std::isfinite(c->info.relres) && c->info.relres < 1e3 && c->bicg_restart;   // (an iterate 1000 x worse than zero is no start)
         ++k) {
        if (ss.rowdist)   // the iterate at the columns other ranks own: the warm start reads them
            if (int rc2 = rowdist_import_ghosts(c, ss.use_bnd ? 1 : 0, c->u.p)) return rc2;
        HIPCHK(c, c->restart_u.alloc((size_t)n));
        HIPCHK(c, hipMemcpyAsync(c->restart_u.p, c->u.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        rc = solve_run(c, ss, A, f_dev, g_dev, c->restart_u.p, FDAPDE_SOLVER_BICGSTAB, rtol, maxit - total, check_every, 0);
        total += c->info.iters;
    }
    c->info.iters = total;
    // The last stage where the caller left the method open (FDAPDE_SOLVER_AUTO): BiCGStab gave up -- restarts exhausted, stalled until maxit, or an
    // iterate that stopped being finite -- on a system the reference's LU would have solved (fem_linear_elliptic_solver.h:38-47; typically an
    // advection-dominated operator): restarted GMRES(m) on the same scaled system, from BiCGStab's iterate if that was any closer than zero.
    // ... but first, for a system small enough to invert (kernels_dense.h): a DIRECT solve of the reference's own row-zeroed matrix -- what its
    // SparseLU does, in milliseconds where restarted GMRES needs 10^4 - 10^5 iterations (cell Peclet numbers of 10^3 on a few thousand DOFs)
    // (a budget the caller set -- maxit -- and BiCGStab spent is spent for this stage too: the call reports what its iterations reached)
    if (gmres_budget >= 0 && (gmres_budget > 0 || maxit - total > 0) && rc == FDAPDE_ENOCONV && c->info.method_used == FDAPDE_SOLVER_BICGSTAB && !ss.dist && !ss.rowdist &&
        dense_eligible(c)) {
        bool solved = false;
        if (int rc2 = dense_direct(c, A, ss.use_bnd, f_dev, g_dev, &solved)) return rc2;
        if (solved) {
            c->info.method_used = FDAPDE_SOLVER_DENSE, c->info.converged = 1, c->info.relres = c->solve_dense.check, c->info.persistent = 0;
            c->h_ctl[0] = 1, c->h_ctl[2] = 0;
            c->err.clear();
            if (c->ev1_at_end) HIPCHK(c, hipEventRecord(c->ev1, c->stream));
            return FDAPDE_OK;
        }
    }
    const int gm_maxit = gmres_budget > 0 ? gmres_budget : maxit - total;
    if (gmres_budget >= 0 && gm_maxit > 0 && c->auto_gmres && rc == FDAPDE_ENOCONV && c->info.method_used == FDAPDE_SOLVER_BICGSTAB && !ss.dist && !ss.rowdist) {
        const bool warm = std::isfinite(c->info.relres) && c->info.relres < 1.0;
        if (warm) {
            HIPCHK(c, c->restart_u.alloc((size_t)n));
            HIPCHK(c, hipMemcpyAsync(c->restart_u.p, c->u.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        }
        rc = solve_run(c, ss, A, f_dev, g_dev, warm ? c->restart_u.p : u0_dev, FDAPDE_SOLVER_GMRES, rtol, gm_maxit, check_every, 0);
        c->info.iters += total;
    }
    return rc;
}

// One-time preparation of the solver's compact matrix layout for the current boundary-DOF mask (part of set-up, like
// fdapde_dofs_build; the first solve does it lazily otherwise).  with_dirichlet: the layout used when Dirichlet data are set.
int e_solver_prepare(fdapde_ctx* c, int32_t with_dirichlet) {
    if (!c) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready) return fail(c, FDAPDE_ENOTINIT, "call fdapde_dofs_build first");
    HIPCHK(c, hipSetDevice(c->device));
    const int v = with_dirichlet ? 1 : 0;
    struct FilledGuard {   // a layout built again here no longer holds the prepared system's values
        fdapde_ctx* c;
        int v;
        bool ps_filled, bk_filled;
        ~FilledGuard() {
            if (c->ps[v].filled != ps_filled || c->bk[v].filled != bk_filled) c->drop_prepared("fdapde_solver_prepare built the solver's layout again");
        }
    } filled_guard{c, v, c->ps[v].filled, c->bk[v].filled};
    if (c->persist && !c->persist_broken && c->comm == nullptr && c->ar_fn == nullptr && (c->op_symmetric || c->persist_bicg)) {
        // single GPU: the single-launch solver's layout (CG for a symmetric operator, BiCGStab on the plain storage otherwise); when the
        // system qualifies for it, the compact pattern and the column codes of the multi-launch SpMV are not needed (a matrix that turns
        // out not to qualify at solve time falls back and builds them lazily)
        c->persist_plain = c->op_symmetric ? 0 : 1;
        if (int rc = build_persist(c, v)) return rc;
        if (c->ps[v].ok && (c->op_symmetric || (!c->ps[v].meta.sym && c->ps[v].meta.R <= 8))) return FDAPDE_OK;
    }
    if (c->blocked && c->comm == nullptr && c->ar_fn == nullptr &&
        ((double)c->hs.nnz >= 20.0 * (double)c->hs.n_dofs || c->blocked == 2 || c->hs.n_dofs > kBlockedShortRowsAbove)) {   // single GPU, long rows: the multi-launch kernels use the blocked-ELL layout
        if (int rc = build_blocked(c, v)) return rc;
        if (c->bk[v].ok) return FDAPDE_OK;
    }
    return build_solver_pattern(c, v);
}

// What the in-solve SpMV works on, for the roofline figures of bench.py: the interior block A_II as a plain CSR operator
// (rows / entries; algorithmic bytes = 12 nnz + 4 (n + 1) + 16 n on it) and the bytes one launch of the solver's kernel really
// streams from the compact coded layout (values 8 B + column codes 2 B per stored entry, row pointers, window bases, virtual-row
// table of a segmented pattern, x gathered once and y written once for every row of the full vector).
int e_solver_layout(fdapde_ctx* c, int32_t with_dirichlet, int64_t* n_interior, int64_t* nnz_interior, double* streamed_bytes) {
    if (!c) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready) return fail(c, FDAPDE_ENOTINIT, "call fdapde_dofs_build first");
    HIPCHK(c, hipSetDevice(c->device));
    const int v = with_dirichlet ? 1 : 0;
    const bool persist = c->persist && !c->persist_broken && c->ps[v].tried && c->ps[v].ok;
    const bool blocked = !persist && c->bk[v].tried && c->bk[v].ok;
    if (!persist && !blocked)
        if (int rc = build_solver_pattern(c, v)) return rc;
    if (int rc = ensure_host(c, kHostPattern)) return rc;
    const HostSpace& hs = c->hs;
    int64_t ni = 0, nz = 0;
    for (int64_t i = 0; i < hs.n_dofs; ++i) {
        if (v && hs.dof_bnd_i[(size_t)i]) continue;
        ++ni;
        for (int32_t k = hs.rowptr_i[(size_t)i]; k < hs.rowptr_i[(size_t)i + 1]; ++k)
            if (!(v && hs.dof_bnd_i[(size_t)hs.colidx_i[(size_t)k]])) ++nz;
    }
    if (n_interior) *n_interior = ni;
    if (nnz_interior) *nnz_interior = nz;
    if (streamed_bytes) {
        if (persist) {   // one iteration of the persistent CG: the ELL blocks (8 + 2 bytes per entry, padding included) + the exchanged
                         // entries of p (two 8-byte granules each, written once and read once)
            // (fdapde_solver_layout_kind tells whether the blocks stream at all: the resident form reads them from LDS)
            *streamed_bytes = 10.0 * (double)c->ps[v].meta.n_entries + 32.0 * (double)c->ps[v].meta.n_board +
                              (c->ps[v].meta.R > kPersistRmax ? 16.0 * (double)c->ps[v].meta.n_int : 0.0);   // (wide form: x read and written once per row)
        } else if (blocked) {   // ELL blocks + x staged once per block (own rows and imports) + y written once
            *streamed_bytes = 10.0 * (double)c->bk[v].meta.n_entries + 8.0 * (double)(c->bk[v].meta.n_int + c->bk[v].meta.n_imp) + 8.0 * (double)c->bk[v].meta.n_int;
        } else if (c->sp_built[v]) {
            const int64_t n_csr = c->sp_nv[v] > 0 ? c->sp_nv[v] : hs.n_dofs;
            *streamed_bytes = 10.0 * (double)c->sp_nnz[v] + 4.0 * (double)(n_csr + 1) + 16.0 * (double)((n_csr + kCodeRows - 1) / kCodeRows) +
                              (c->sp_nv[v] > 0 ? 8.0 * (double)n_csr : 0.0) + 16.0 * (double)hs.n_dofs +
                              4.0 * (double)c->sp_wide[v] * kCodeRows * ((double)c->sp_nnz[v] / (double)(n_csr > 0 ? n_csr : 1));
        } else
            *streamed_bytes = 12.0 * (double)hs.nnz + 4.0 * (double)(hs.n_dofs + 1) + 16.0 * (double)hs.n_dofs;
    }
    return FDAPDE_OK;
}

// which layout the solver holds for the boundary variant (after fdapde_solver_prepare / a solve): kind 0 compact CSR, 1 blocked ELL
// (multi-launch), 2 persistent launch with streaming blocks, 3 persistent launch with the blocks resident in LDS
int e_solver_layout_kind(fdapde_ctx* c, int32_t with_dirichlet, int32_t* kind, int32_t* symmetric_storage, int32_t* workgroups,
                              int32_t* rows_per_thread) {
    if (!c) return FDAPDE_EINVAL;
    if (!c->dev_ready) return fail(c, FDAPDE_ENOTINIT, "call fdapde_dofs_build first");
    const int v = with_dirichlet ? 1 : 0;
    const bool persist = c->persist && !c->persist_broken && c->ps[v].tried && c->ps[v].ok;
    const bool blocked = !persist && c->bk[v].tried && c->bk[v].ok;
    if (kind) *kind = persist ? (c->ps[v].stream ? 2 : 3) : blocked ? 1 : 0;
    if (symmetric_storage) *symmetric_storage = persist && c->ps[v].meta.sym ? 1 : 0;
    if (workgroups) *workgroups = persist ? c->ps[v].meta.G : blocked ? c->bk[v].meta.G : 0;
    if (rows_per_thread) *rows_per_thread = persist ? c->ps[v].meta.R : blocked ? c->bk[v].meta.R : 0;
    return FDAPDE_OK;
}

int e_solve(fdapde_ctx* c, const fdapde_options* opt, fdapde_info* info) {
    if (!c) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready || !c->assembled[0] || !c->force_ready)
        return fail(c, FDAPDE_ENOTINIT, "solver must be initialized first!");   // fem_linear_elliptic_solver.h:36
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->hs.n_dofs;
    const double rtol = (opt && opt->rtol > 0) ? opt->rtol : 1e-10;
    const int maxit = (opt && opt->maxit > 0) ? opt->maxit : default_maxit(c, n);
    const int check_every = (opt && opt->check_every > 0) ? opt->check_every : 32;
    const double* A = c->vals[FDAPDE_MAT_STIFF].p;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    // (a solve by another solver's name in between: the next Jacobi-Krylov solve prepares in full)
    if (opt && (opt->method == FDAPDE_SOLVER_PMG || opt->method == FDAPDE_SOLVER_AMG || opt->method == FDAPDE_SOLVER_DENSE))
        c->drop_prepared("a solve by the name of another solver came in between");
    if (opt && opt->method == FDAPDE_SOLVER_PMG) return e_solve_pmg(c, opt, info);   // the two-level solver of order-2 spaces (eng_pmg.hip), by name
    if (opt && opt->method == FDAPDE_SOLVER_AMG) return e_solve_amg(c, opt, info);   // the aggregation multilevel solver (eng_amg.hip), by name only
    if (opt && opt->method == FDAPDE_SOLVER_DENSE) {
        // the direct solve asked for by name (what the reference's SparseLU does, fem_linear_elliptic_solver.h:38-47): the reference's own row-zeroed matrix
        // inverted on the device, one product; no Krylov stage in front, no fall-back behind -- a singular matrix is reported (success = false)
        if (!dense_eligible(c)) return fail(c, FDAPDE_EUNSUPPORTED, kDenseRefusal);
        bool solved = false;
        c->scaled_owner = fdapde_ctx::kScaledNone;
        if (int rc = dense_direct(c, A, c->have_g ? 1 : 0, c->force.p, c->g.p, &solved)) return rc;
        HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        HIPCHK(c, hipEventSynchronize(c->ev1));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        const double t_asm = c->info.t_assemble_ms;   // (fdapde_init's figure stays with the record)
        c->info = fdapde_info{};
        c->info.t_assemble_ms = t_asm;
        c->info.method_used = FDAPDE_SOLVER_DENSE, c->info.converged = solved ? 1 : 0, c->info.relres = c->solve_dense.check, c->info.t_solve_ms = ms;
        c->solved = solved, c->dirichlet_applied = c->have_g;
        if (info) *info = c->info;
        if (!solved) {
            c->err = dense_singular("the matrix");
            return FDAPDE_ENOCONV;
        }
        return FDAPDE_OK;
    }
    // The open method on a LARGE order-2 system it qualifies for: the two-level solver first (eng_pmg.hip: ~19 iterations whatever the mesh size, where the
    // Jacobi-preconditioned stages below need O(1 / h) -- C5, 5.36 M DOFs: 64 ms against 617; the two meet near 200 - 300 k DOFs: 3-D 185 k 9.3 against 8.6 ms,
    // 389 k 13 against 21; 2-D, symmetric, 315 k 27 against 25).  Whatever it does not solve falls through to the stages below.
    // (rent-or-buy: below `pmg_auto_first_rows` the context's first open-method solve keeps the Jacobi stages -- the coarse level is built by the second)
    if ((!opt || opt->method == FDAPDE_SOLVER_AUTO) && c->pmg_auto && n >= c->pmg_auto_rows &&
        (n >= c->pmg_auto_first_rows || c->pmg.ready || c->open_solves >= 1) && pmg_eligible(c)) {
        fdapde_options po{};
        po.method = FDAPDE_SOLVER_PMG, po.rtol = rtol, po.maxit = (opt && opt->maxit > 0) ? std::min(opt->maxit, 60) : 60;   // (it converges in two dozen iterations or not at all)
        const int rc = e_solve_pmg(c, &po, info);
        if (rc == FDAPDE_OK) {
            ++c->open_solves;
            return rc;
        }
        if (rc != FDAPDE_ENOCONV && rc != FDAPDE_EUNSUPPORTED) return rc;
        c->err.clear();
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    }
    SolveState ss;
    if (c->scaled_owner != fdapde_ctx::kScaledSolve) c->drop_prepared("the shared buffers held another solver's system");
    c->scaled_owner = fdapde_ctx::kScaledSolve;
    DebugClock clk;
    const bool open_method = !opt || opt->method == FDAPDE_SOLVER_AUTO;
    const bool skip_cg = open_method && c->cg_broke_down;   // (this very matrix broke CG before: see below)
    const int gm_budget = open_gmres_budget(c, opt, n);
    if (int rc = solve_prepare(c, A, c->have_g ? 1 : 0, &ss, c->op_symmetric && !skip_cg, /*allow_defer=*/true, /*reuse=*/true)) return rc;
    clk.mark("fdapde_solve: solve_prepare");
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));   // (a solve that ends before its epilogue -- an early refusal -- still leaves a recorded event)
    c->ev1_at_end = true;
    struct Ev1Guard {
        fdapde_ctx* c;
        ~Ev1Guard() { c->ev1_at_end = false; }
    } ev1_guard{c};
    int rc = solve_run_restarting(c, ss, A, c->force.p, c->g.p, nullptr, skip_cg ? FDAPDE_SOLVER_BICGSTAB : (opt ? opt->method : FDAPDE_SOLVER_AUTO), rtol,
                                  maxit, check_every, opt ? opt->time_spmv : 0, gm_budget);
    clk.mark("fdapde_solve: solve_run");
    if (ss.diag_deferred) {   // the flag the solve did not wait for
        if (c->h_ctl_seen < 5) {   // (an outcome read-back that did not carry it: fetch it now)
            HIPCHK(c, hipMemcpyAsync(c->h_ctl + 4, c->ctl.p + 4, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        if (c->h_ctl[4] == 0 && c->prep.pending) c->prep.valid = true, c->prep.pending = false;   // (the host has seen the flag: the prepared system may be kept)
        if (c->h_ctl[4] != 0) {   // a non-positive interior diagonal after all: everything again with the decision taken up front
            c->drop_prepared("an interior diagonal entry is not positive");
            if (int rc2 = solve_prepare(c, A, c->have_g ? 1 : 0, &ss, c->op_symmetric && !skip_cg, false)) return rc2;
            rc = solve_run_restarting(c, ss, A, c->force.p, c->g.p, nullptr, skip_cg ? FDAPDE_SOLVER_BICGSTAB : (opt ? opt->method : FDAPDE_SOLVER_AUTO), rtol,
                                      maxit, check_every, opt ? opt->time_spmv : 0, gm_budget);
        }
    }
    bool cg_broke = false;
    if (int rc2 = cg_breakdown_agreed(c, ss, rc, open_method, "fdapde_solve: the ranks disagree on the outcome of the CG stage", &cg_broke)) return rc2;
    if (cg_broke) {
        // CG broke down (p.Ap <= 0): the operator is symmetric but not positive definite -- e.g. 3-D P2 with a large reaction term: the
        // reference's 5-point rule has a negative weight, its mass matrix is indefinite (integrator_tables.h:275-292).  The reference's LU solves
        // such a system all the same (fem_linear_elliptic_solver.h:38-47); so does BiCGStab.  Only where the caller left the method open.
        c->cg_broke_down = true;   // (until the matrix is assembled again)
        c->drop_prepared("CG broke down: the system is prepared again for BiCGStab");
        if (int rc2 = solve_prepare(c, A, c->have_g ? 1 : 0, &ss, false)) return rc2;
        rc = solve_run_restarting(c, ss, A, c->force.p, c->g.p, nullptr, FDAPDE_SOLVER_BICGSTAB, rtol, maxit, check_every, opt ? opt->time_spmv : 0, gm_budget);
        clk.mark("fdapde_solve: solve_run (BiCGStab after a CG breakdown)");
    }
    {
        if (rc == FDAPDE_OK && open_method && c->cg_broke_down && !ss.dist && !ss.rowdist) {
            // A symmetric operator that broke CG is indefinite -- or SINGULAR (a pure Neumann problem): on a matrix that is singular up to rounding
            // BiCGStab "converges" to a solution with a huge multiple of the null vector in it (-Lap u = 1 without Dirichlet data: |u| ~ 1e14, residual
            // 1e-11 by the recurrence -- a number that cannot be checked: the rounding error of A u alone is eps |A| |u| >> tol |b|).  The reference's LU
            // reports failure on such a matrix (fem_linear_elliptic_solver.h:42-45).  Guard: |x| / |b| of the scaled system (unit diagonal, |A~| ~ 1)
            // beyond 1e12 is reported as success = false, never handed out as a solution.
            const double* xs = c->info.persistent ? c->persist_x.p : c->x.p;
            hipLaunchKernelGGL(k_sq_norm, dim3(c->vec_grid), dim3(256), 0, c->stream, n, xs, c->part_b.p);
            hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(256), 0, c->stream, c->part_b.p, c->vec_grid, c->sc.p + 20);
            double xx = 0;
            HIPCHK(c, hipMemcpyAsync(&xx, c->sc.p + 20, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            const double bb = c->h_sc[0];
            if (!(xx <= 1e24 * bb)) {
                c->info.converged = 0;
                c->err = "operator numerically singular: the iterate grew beyond 1e12 |b| (e.g. no Dirichlet DOF and a right-hand side outside the range)";
                rc = FDAPDE_ENOCONV;
            }
        }
    }
    if (rc != FDAPDE_OK && rc != FDAPDE_ENOCONV) return rc;
    HIPCHK(c, hipEventSynchronize(c->ev1));   // (recorded by solve_run behind its epilogue kernel: already reached, its final wait came after it)
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->info.t_solve_ms = ms;
    c->solved = true, c->dirichlet_applied = c->have_g;
    if (open_method) ++c->open_solves;
    if (info) *info = c->info;
    return rc;
}

// The coarse level of the two-level solver (eng_pmg.hip) is solved ~50 times per fine solve, every time for the SAME matrix: what fdapde_solve does in front
// of its Krylov stage (Jacobi scale, scaled copy, the launch's layout filled: ~0.15 ms of kernels and two waits at 681 k rows) is done once per coarse
// operator, as the parabolic stepper does for its steps; a solve is then solve_run on the context's load vector.  Same method choice as fdapde_solve's open
// method (CG for a symmetric operator with a positive diagonal, BiCGStab after a CG breakdown or else), without its direct / GMRES stages.
int coarse_prepare(fdapde_ctx* c, SolveState* ss) {
    HIPCHK(c, hipSetDevice(c->device));
    c->scaled_owner = fdapde_ctx::kScaledSolve;
    return solve_prepare(c, c->vals[FDAPDE_MAT_STIFF].p, c->have_g ? 1 : 0, ss, c->op_symmetric && !c->cg_broke_down, false);
}

int coarse_solve(fdapde_ctx* c, SolveState* ss, double rtol, int maxit, fdapde_info* info) {
    const double* A = c->vals[FDAPDE_MAT_STIFF].p;
    int method = c->cg_broke_down ? FDAPDE_SOLVER_BICGSTAB : FDAPDE_SOLVER_AUTO;
    int rc = solve_run_restarting(c, *ss, A, c->force.p, c->g.p, nullptr, method, rtol, maxit, 32, 0, 0);
    if (rc == FDAPDE_ENOCONV && c->h_ctl[2] != 0 && method == FDAPDE_SOLVER_AUTO && is_cg_method(c->info.method_used)) {   // (see fdapde_solve)
        c->cg_broke_down = true;
        if (int rc2 = solve_prepare(c, A, c->have_g ? 1 : 0, ss, false, false)) return rc2;
        rc = solve_run_restarting(c, *ss, A, c->force.p, c->g.p, nullptr, FDAPDE_SOLVER_BICGSTAB, rtol, maxit, 32, 0, 0);
    }
    if (rc != FDAPDE_OK && rc != FDAPDE_ENOCONV) return rc;
    c->solved = true, c->dirichlet_applied = c->have_g;
    if (info) *info = c->info;
    return rc;
}

namespace {

// what the steps of an iterative stepper add up to: iterations, the worst relres, FDAPDE_ENOCONV if a step did not converge
struct StepTally {
    int iters = 0, rc = FDAPDE_OK;
    double worst = 0;
    bool gave_up = false;   // (give_up_on_first: the first step did not converge, nothing of the call is done)
};

// The time-stepping loop of the iterative solvers: rhs = (M / dt) u_i + f_{i+1}, the Dirichlet column i + 1 up and into the internal order (gcol),
// one solve -- step(i, rhs, gcol, uprev) leaves c->u and c->info and returns FDAPDE_OK, FDAPDE_ENOCONV or a hard error --, u_i <- u, the column
// down.  Everything is on the one stream; wait_each_step: the host waits for the column before the next step starts
template <typename Step>
int step_loop(fdapde_ctx* c, int32_t n_times, double inv_dt, const double* dirichlet, double* solution, double* rhs, double* gcol, double* uprev, bool wait_each_step,
              bool give_up_on_first, Step&& step, StepTally& tally) {
    const int64_t n = c->hs.n_dofs;
    hipStream_t st = c->stream;
    for (int32_t i = 0; i + 1 < n_times; ++i) {
        launch_spmv(c, c->vals[FDAPDE_MAT_MASS].p, uprev, c->s.p, nullptr, nullptr, nullptr);   // M u_i
        hipLaunchKernelGGL(k_parabolic_rhs, dim3(g1(n)), dim3(256), 0, st, n, c->s.p, inv_dt, c->force.p + (size_t)(i + 1) * n, rhs);
        if (dirichlet) {   // column i + 1 as handed over, brought into the internal order on the device (no wait here)
            HIPCHK(c, hipMemcpyAsync(c->tmp_i.p, dirichlet + (size_t)(i + 1) * n, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_gather_f64, dim3(g1(n)), dim3(256), 0, st, n, c->dof_i2e.p, c->tmp_i.p, gcol);
        }
        const int rc = step(i, rhs, gcol, uprev);
        if (rc != FDAPDE_OK && rc != FDAPDE_ENOCONV) return rc;
        if (rc == FDAPDE_ENOCONV && i == 0 && give_up_on_first) {
            tally.gave_up = true;
            c->err.clear();
            return FDAPDE_OK;
        }
        if (rc == FDAPDE_ENOCONV) tally.rc = rc;
        tally.iters += c->info.iters, tally.worst = std::max(tally.worst, c->info.relres);
        HIPCHK(c, hipMemcpyAsync(uprev, c->u.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_scatter_f64, dim3(g1(n)), dim3(256), 0, st, n, c->dof_i2e.p, c->u.p, c->tmp_e.p);
        HIPCHK(c, hipMemcpyAsync(solution + (size_t)(i + 1) * n, c->tmp_e.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
        if (wait_each_step) HIPCHK(c, hipStreamSynchronize(st));   // (tmp_e is reused by the next step)
    }
    return FDAPDE_OK;
}

// The end of every path of the stepper: the event behind the last download and the wait for it, the call's figures into the record.  method_used
// < 0: the record keeps what the last step ran (and its `persistent`); owner < 0: the shared buffers keep their owner
int stepper_end(fdapde_ctx* c, const StepTally& t, int method_used, int owner, int64_t open_steps, fdapde_info* info) {
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->info.t_solve_ms = ms, c->info.iters = t.iters, c->info.relres = t.worst, c->info.converged = t.rc == FDAPDE_OK ? 1 : 0;
    if (method_used >= 0) c->info.method_used = method_used, c->info.persistent = 0;
    if (owner >= 0) c->scaled_owner = owner;
    c->open_solves += open_steps;
    if (info) *info = c->info;
    return t.rc;
}

}   // namespace

// FEMLinearParabolicSolver::solve (fdaPDE/finite_elements/solvers/fem_linear_parabolic_solver.h:37-72): implicit Euler,
//   K = M / dt + A ; Dirichlet rows of K ; for i = 0 .. m-2:  rhs = (M / dt) u_i + f_{i+1} ; rhs[boundary] = g(., i+1) ;
//   u_{i+1} = K^{-1} rhs.   The reference factorises K once with SparseLU; here K is scaled once and every step is a
//   Jacobi-PCG (or BiCGStab) solve warm-started from u_i.  Forcing columns come from fdapde_set_forcing (n_times columns).
// Four solvers: a small K is inverted once (the dense loops, below); FDAPDE_SOLVER_AMG, the two-level solver and the Jacobi-Krylov stages go
// through step_loop, each with its own step.
int e_solve_parabolic(fdapde_ctx* c, const fdapde_options* opt, int32_t n_times, double delta_t, const double* initial_condition,
                           const double* dirichlet, double* solution, fdapde_info* info) {
    if (!c || n_times < 1 || !(delta_t > 0) || !initial_condition || !solution) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready || !c->assembled[0] || !c->assembled[1] || !c->force_ready)
        return fail(c, FDAPDE_ENOTINIT, "solver must be initialized first!");   // fem_linear_parabolic_solver.h:39
    if (c->fq_cols < n_times) return fail(c, FDAPDE_EINVAL, "forcing data needs one column per time point");
    HIPCHK(c, hipSetDevice(c->device));
    const HostSpace& hs = c->hs;
    const int64_t n = hs.n_dofs;
    hipStream_t st = c->stream;
    const double rtol = (opt && opt->rtol > 0) ? opt->rtol : 1e-10;
    const int maxit = (opt && opt->maxit > 0) ? opt->maxit : default_maxit(c, n);
    const int check_every = (opt && opt->check_every > 0) ? opt->check_every : 8;
    const double inv_dt = 1.0 / delta_t;
    const bool open_method = !opt || opt->method == FDAPDE_SOLVER_AUTO;
    const int use_bnd = dirichlet ? 1 : 0;
    DBuf<double> kmat, uprev, rhs, gcol;   // (released when the call returns)
    HIPCHK(c, kmat.alloc((size_t)hs.nnz + 2));
    HIPCHK(c, uprev.alloc((size_t)n));
    HIPCHK(c, rhs.alloc((size_t)n));
    HIPCHK(c, gcol.alloc((size_t)n));
    std::vector<double> tmp((size_t)n);
    if (int rc = ensure_host(c, kHostPerm)) return rc;
    // u_0 into the internal order and up (tmp is pageable: the wait), solution_.col(0) = initial condition (line 46)
    auto initial_up = [&]() -> int {
        for (int64_t i = 0; i < n; ++i) tmp[(size_t)i] = initial_condition[hs.dof_i2e[(size_t)i]];
        HIPCHK(c, hipMemcpyAsync(uprev.p, tmp.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
        std::memcpy(solution, initial_condition, sizeof(double) * (size_t)n);
        return FDAPDE_OK;
    };
    HIPCHK(c, hipEventRecord(c->ev0, st));
    hipLaunchKernelGGL(k_matrix_combine, dim3(g1(hs.nnz)), dim3(256), 0, st, hs.nnz, c->vals[FDAPDE_MAT_MASS].p,
                       c->vals[FDAPDE_MAT_STIFF].p, inv_dt, kmat.p);
    // K is fixed over the steps: the reference factorises it ONCE and back-substitutes per step (fem_linear_parabolic_solver.h:41,56-68).  A small K is
    // inverted once here (kernels_dense.h) and a step is two products -- M u_i and K^-1 rhs -- with nothing returning to the host inside the loop: every
    // Dirichlet column goes up in front, the solution stays on the device and comes down once.
    // (a warm-started Krylov step of such a system costs ~0.2 ms: worth it when the steps add up to half an inversion)
    const bool dense_named = opt && opt->method == FDAPDE_SOLVER_DENSE;
    if (dense_named && !dense_eligible(c)) return fail(c, FDAPDE_EUNSUPPORTED, kDenseRefusal);
    if ((open_method || dense_named) && dense_eligible(c) &&
        (dense_named || c->dense_after == 0 || (n_times - 1 > c->dense_after && 0.2 * (n_times - 1) >= 0.5 * dense_build_estimate_ms(n)))) {
        fdapde_ctx::Dense& D = c->step_dense;
        D.ready = D.failed = false;
        if (int rc = dense_build(c, kmat.p, use_bnd, D)) return rc;
        if (D.ready) {
            DBuf<double> d_dir, d_sol;
            const size_t cols = (size_t)n_times;
            HIPCHK(c, d_sol.alloc((size_t)n * cols));
            if (dirichlet) HIPCHK(c, d_dir.upload(dirichlet, (size_t)n * cols, st));
            if (int rc = initial_up()) return rc;
            if (!D.refine && c->dense_fold) {   // ONE product per step: u_{i+1} = (K^-1 M / dt) u_i + K^-1 (f_{i+1}, g_{i+1})
                if (int rc = dense_step_loop(c, D, n_times, inv_dt, dirichlet ? d_dir.p : nullptr, uprev.p, d_sol.p)) return rc;
            } else
                for (int32_t i = 0; i + 1 < n_times; ++i) {
                    launch_spmv(c, c->vals[FDAPDE_MAT_MASS].p, uprev.p, c->s.p, nullptr, nullptr, nullptr);   // M u_i
                    dense_step_rhs(c, c->s.p, inv_dt, c->force.p + (size_t)(i + 1) * n, dirichlet ? d_dir.p + (size_t)(i + 1) * n : nullptr, rhs.p);   // (+ rhs[boundary] = g(., i + 1), line 66)
                    if (int rc = dense_apply(c, D, 1, rhs.p, c->u.p)) return rc;
                    dense_step_out(c, c->u.p, uprev.p, d_sol.p + (size_t)(i + 1) * n);
                }
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(solution + (size_t)n, d_sol.p + (size_t)n, sizeof(double) * (size_t)n * (cols - 1), hipMemcpyDeviceToHost, st));
            StepTally t;
            t.iters = D.refine ? n_times - 1 : 0, t.worst = D.check;
            c->info.launch_ms = 0;
            const int rc = stepper_end(c, t, FDAPDE_SOLVER_DENSE, fdapde_ctx::kScaledNone, 0, info);
            D.X.release(), D.ready = false;   // (K belongs to this call)
            return rc;
        }
        if (dense_named) return c->err = dense_singular("M / dt + A"), bare_answer(c, FDAPDE_SOLVER_DENSE, D.check, info, FDAPDE_ENOCONV);
    }
    // FDAPDE_SOLVER_AMG by name: the hierarchy of K built once for the call, every step warm-started from the previous column (eng_amg.hip)
    if (opt && opt->method == FDAPDE_SOLVER_AMG) {
        if (!amg_eligible(c)) return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_AMG takes one-GPU contexts");
        const int am_maxit = (opt->maxit > 0) ? opt->maxit : 200;
        if (int rc = amg_build(c, &c->amg, kmat.p, use_bnd, c->op_symmetric)) return bare_answer(c, FDAPDE_SOLVER_AMG, 0.0, info, rc);
        if (int rc = initial_up()) return rc;
        StepTally t;
        auto step = [&](int32_t, const double* rhs_i, const double* g_i, const double* u_i) {
            return amg_run(c, c->amg, kmat.p, rhs_i, g_i, use_bnd, u_i, rtol, am_maxit);
        };
        if (int rc = step_loop(c, n_times, inv_dt, dirichlet, solution, rhs.p, gcol.p, uprev.p, /*wait_each_step=*/true, /*give_up_on_first=*/false, step, t)) return rc;
        if (t.rc != FDAPDE_OK) c->err = "FDAPDE_SOLVER_AMG: a step did not converge";
        const int rc = stepper_end(c, t, FDAPDE_SOLVER_AMG, -1, 0, info);
        amg_forget(c);   // (K belongs to this call; behind the event and its wait, so that t_solve_ms does not hold the teardown)
        return rc;
    }
    // Large order-2 systems (or FDAPDE_SOLVER_PMG by name): every step through the two-level solver (eng_pmg.hip) -- the coarse operator is the P1 assembly of
    // the same terms + M1 / dt, built once for the call; a step starts from the previous column.  A first step it does not solve sends the open method to
    // the Jacobi-preconditioned steps below, from the start.
    const bool pmg_named = opt && opt->method == FDAPDE_SOLVER_PMG;
    if (pmg_named && !pmg_eligible(c))
        return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_PMG takes one-GPU contexts and order-2 spaces");
    if (pmg_named || (open_method && c->pmg_auto && n >= c->pmg_auto_rows &&
                      (n >= c->pmg_auto_first_rows || c->pmg.ready || c->open_solves >= 1 || n_times > 5) && pmg_eligible(c))) {
        const int pm_maxit = pmg_named ? ((opt && opt->maxit > 0) ? opt->maxit : 400) : ((opt && opt->maxit > 0) ? std::min(opt->maxit, 60) : 60);
        if (int rc = initial_up()) return rc;
        StepTally t;
        auto step = [&](int32_t, const double* rhs_i, const double* g_i, const double* u_i) {
            return pmg_run(c, kmat.p, rhs_i, g_i, use_bnd, u_i, inv_dt, 2 * c->init_count + 1, rtol, pm_maxit);
        };
        if (int rc = step_loop(c, n_times, inv_dt, dirichlet, solution, rhs.p, gcol.p, uprev.p, /*wait_each_step=*/true, /*give_up_on_first=*/!pmg_named, step, t)) return rc;
        if (!t.gave_up) return stepper_end(c, t, FDAPDE_SOLVER_PMG, fdapde_ctx::kScaledNone, pmg_named ? 0 : n_times - 1, info);
    }
    // The Jacobi-Krylov stages (solve_run_restarting), K prepared once: a step's outcome is read inside solve_run and what follows it is ordered by the
    // stream, so the host does not wait between the steps
    SolveState ss;
    c->scaled_owner = fdapde_ctx::kScaledParabolic;
    if (int rc = solve_prepare(c, kmat.p, use_bnd, &ss, c->op_symmetric)) return rc;
    if (int rc = initial_up()) return rc;
    int step_method = opt ? opt->method : FDAPDE_SOLVER_AUTO;
    const int open_step = open_gmres_budget(c, opt, n);
    auto krylov_step = [&](int32_t, const double* rhs_i, const double* g_i, const double* u_i) -> int {
        c->defer_end_sync = true;
        int rc = solve_run_restarting(c, ss, kmat.p, rhs_i, g_i, u_i, step_method, rtol, maxit, check_every, 0, open_step);
        bool cg_broke = false;
        if (int rc2 = cg_breakdown_agreed(c, ss, rc, step_method == FDAPDE_SOLVER_AUTO,
                                          "fdapde_solve_parabolic: the ranks disagree on the outcome of the CG stage", &cg_broke))
            return rc2;
        if (cg_broke) {   // M / dt + A symmetric but not positive definite (see fdapde_solve): this step again and every later one with BiCGStab
            if (int rc2 = solve_prepare(c, kmat.p, use_bnd, &ss, false)) return rc2;
            step_method = FDAPDE_SOLVER_BICGSTAB;
            rc = solve_run_restarting(c, ss, kmat.p, rhs_i, g_i, u_i, step_method, rtol, maxit, check_every, 0, open_step);
        }
        c->defer_end_sync = false;
        if ((rc == FDAPDE_OK || rc == FDAPDE_ENOCONV) && ss.rowdist)   // u_{i+1} of the columns other ranks own: read by the next step's M u_i and warm start
            if (int rc2 = rowdist_import_ghosts(c, ss.use_bnd ? 1 : 0, c->u.p)) return rc2;
        return rc;
    };
    StepTally t;
    if (int rc = step_loop(c, n_times, inv_dt, dirichlet, solution, rhs.p, gcol.p, uprev.p, /*wait_each_step=*/false, /*give_up_on_first=*/false, krylov_step, t)) return rc;
    return stepper_end(c, t, -1, -1, open_method ? n_times - 1 : 0, info);
}

// Q columns of fdapde_lin_solve at once (kernels_multirhs.h): b_ext / x_ext are Q host columns of n, reference numbering
template <int Q>
int lin_solve_batch(fdapde_ctx* c, const double* b_ext, double* x_ext, double rtol, int maxit, int check_every, int* iters,
                    double* relres, bool* converged) {
    const HostSpace& hs = c->hs;
    const int64_t n = hs.n_dofs;
    hipStream_t st = c->stream;
    const double tol2 = rtol * rtol;
    DBuf<double> B, X, R, P, Y, part_spmm, part_rr, sc;
    const size_t nq = (size_t)n * Q;
    for (DBuf<double>* b : {&B, &X, &R, &P, &Y}) HIPCHK(c, b->alloc(nq));
    const int64_t nh = n * (Q / 2);
    const int grid_v = (int)std::min<int64_t>(std::max<int64_t>(1, (nh + 256 * kQV - 1) / (256 * kQV)), 1024);
    const int grid_m = (int)std::min<int64_t>((n + 31) / 32, 2048);
    HIPCHK(c, part_spmm.alloc((size_t)grid_m * 2 * Q));
    HIPCHK(c, part_rr.alloc((size_t)grid_v * Q));
    HIPCHK(c, sc.alloc(5 * Q));
    HIPCHK(c, hipMemcpyAsync(B.p, b_ext, sizeof(double) * nq, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_q_init<Q>, dim3(grid_v), dim3(256), 0, st, n, B.p, c->dof_i2e.p, c->scale.p, X.p, R.p, P.p, part_rr.p);
    hipLaunchKernelGGL(k_q_init_fin<Q>, dim3(1), dim3(256), 0, st, part_rr.p, grid_v, sc.p, c->ctl.p);
    int launched = 0;
    bool stop = false;
    std::vector<double> h_sc(5 * Q);
    while (!stop && launched < maxit) {
        const int chunk = (maxit - launched) < check_every ? (maxit - launched) : check_every;
        for (int it = 0; it < chunk; ++it, ++launched) {
            hipLaunchKernelGGL(k_spmm_full<Q>, dim3(grid_m), dim3(256), 0, st, n, c->rowptr.p, c->colidx.p, c->lin_sq.p, P.p, Y.p,
                               part_spmm.p, c->ctl.p);
            hipLaunchKernelGGL(k_q_scalars<Q>, dim3(1), dim3(256), 0, st, part_spmm.p, grid_m, part_rr.p, grid_v, sc.p, tol2, c->ctl.p);
            hipLaunchKernelGGL(k_q_update<Q>, dim3(grid_v), dim3(256), 0, st, n, Y.p, P.p, X.p, R.p, sc.p, part_rr.p, c->ctl.p);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->h_ctl, c->ctl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        stop = c->h_ctl[0] != 0;
    }
    if (!stop) {   // maxit: one more scalar pass so that sc holds the r.r of the last update
        hipLaunchKernelGGL(k_spmm_full<Q>, dim3(grid_m), dim3(256), 0, st, n, c->rowptr.p, c->colidx.p, c->lin_sq.p, P.p, Y.p, part_spmm.p,
                           c->ctl.p);
        hipLaunchKernelGGL(k_q_scalars<Q>, dim3(1), dim3(256), 0, st, part_spmm.p, grid_m, part_rr.p, grid_v, sc.p, tol2, c->ctl.p);
    }
    hipLaunchKernelGGL(k_q_unscale<Q>, dim3(g1(n)), dim3(256), 0, st, n, X.p, c->scale.p, c->dof_i2e.p, B.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(x_ext, B.p, sizeof(double) * nq, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_sc.data(), sc.p, sizeof(double) * 5 * Q, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(c->h_ctl, c->ctl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    // (the scalar pass behind an exhausted budget counts itself where no column has converged: iterations are what was applied to x)
    *iters = std::min<int>(c->h_ctl[1], launched), *converged = c->h_ctl[2] == 0, *relres = 0;
    for (int q = 0; q < Q; ++q) {
        const Outcome out = outcome_of(h_sc[(size_t)q], h_sc[(size_t)Q + q], c->h_ctl[2] != 0, tol2);
        *relres = out.relres > *relres ? out.relres : *relres;
        if (!out.converged) *converged = false;
    }
    return FDAPDE_OK;
}

// fdapde::SparseLU<SpMatrix<double>>::compute (fdaPDE/utils/symbols.h:142-146): "factorise" once.  Here: copy the matrix,
// Jacobi-scale it once; every later fdapde_lin_solve is a Krylov run on the prepared system.
int e_lin_compute(fdapde_ctx* c, int32_t which, const double* values, int32_t symmetric) {
    if (!c || which < 0 || which > 1) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready) return fail(c, FDAPDE_ENOTINIT, "call fdapde_dofs_build first");
    if (!values && !c->assembled[which]) return fail(c, FDAPDE_ENOTINIT, "matrix not assembled");
    HIPCHK(c, hipSetDevice(c->device));
    const HostSpace& hs = c->hs;
    HIPCHK(c, c->lin_mat.alloc((size_t)hs.nnz + 2));
    if (values) {   // reference slot order -> internal slots
        HIPCHK(c, hipMemcpyAsync(c->tmp_v.p, values, sizeof(double) * (size_t)hs.nnz, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_gather_f64, dim3(g1(hs.nnz)), dim3(256), 0, c->stream, hs.nnz, c->slot_i2e.p, c->tmp_v.p, c->lin_mat.p);
        HIPCHK(c, hipGetLastError());
        c->lin_symmetric = symmetric != 0;
    } else {
        HIPCHK(c, hipMemcpyAsync(c->lin_mat.p, c->vals[which].p, sizeof(double) * (size_t)hs.nnz, hipMemcpyDeviceToDevice, c->stream));
        c->lin_symmetric = which == FDAPDE_MAT_MASS ? true : c->op_symmetric;
    }
    if (!c->lin_state) c->lin_state = new SolveStateHolder();
    c->scaled_owner = fdapde_ctx::kScaledNone;
    if (int rc = solve_prepare(c, c->lin_mat.p, 0, &c->lin_state->ss, c->lin_symmetric)) return rc;
    c->scaled_owner = fdapde_ctx::kScaledLin;   // scale / sval now belong to the handle
    c->lin_ready = true, c->lin_sq_ready = false;
    c->lin_dense.ready = c->lin_dense.failed = false, c->lin_cols = 0, c->lin_krylov_ms = 0;   // (a dense inverse belongs to the matrix it was built from)
    ++c->amg_lin_epoch;   // (... and so does FDAPDE_SOLVER_AMG's hierarchy)
    return FDAPDE_OK;
}

// ---- the stages of fdapde_lin_solve: each takes the columns from t.j0 on that are its own and advances the tally ------------------------------
namespace {

struct ColumnTally {
    int total = 0, rc_all = FDAPDE_OK;   // iterations of all columns; FDAPDE_ENOCONV if a column did not converge
    double worst = 0;                    // the worst relres
    bool breakdown = false;              // a CG column stopped on p.Ap <= 0
    int32_t j0 = 0;                      // columns done
};
struct LinCall {   // one fdapde_lin_solve, as its stages see it
    fdapde_ctx* c; const double* b; double* x; int32_t n_rhs; int64_t n;   // the context, b and x as handed over, their columns and rows
    double rtol;
    int maxit, check_every, method, gm_budget;
    ColumnTally t;

    // "Factor once" that pays per solve (kernels_dense.h): a small system that has been asked for more than `dense_after` columns gets its dense
    // inverse -- built once, ~ms -- and every column from then on is ONE matrix-vector product, b and x through pinned memory.  Where the method was
    // left open; by name (dense_named) the inverse is built now, whatever the columns so far have cost.  *done: the call is answered (rc its answer)
    int dense_stage(bool dense_named, fdapde_info* info, bool* done) {
        fdapde_ctx::Dense& D = c->lin_dense;
        *done = false;
        if (!D.ready && (!D.failed || dense_named) && (dense_named || c->dense_after == 0 || (c->lin_cols + n_rhs > c->dense_after && c->lin_krylov_ms >= 0.5 * dense_build_estimate_ms(n))))
            if (int rc = dense_build(c, c->lin_mat.p, 0, D)) return rc;
        if (!D.ready && !dense_named) return FDAPDE_OK;
        *done = true;
        if (!D.ready) return c->err = dense_singular("the matrix"), bare_answer(c, FDAPDE_SOLVER_DENSE, D.check, info, FDAPDE_ENOCONV);
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = dense_solve_host(c, D, b, n_rhs, x)) return rc;
        c->lin_cols += n_rhs;
        c->info.iters = D.refine ? 1 : 0, c->info.converged = 1, c->info.relres = D.check, c->info.method_used = FDAPDE_SOLVER_DENSE, c->info.persistent = 0;
        c->info.launch_ms = 0, c->info.spmv_avg_ms = 0, c->info.spmv_timed = 0;
        c->info.t_solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (info) *info = c->info;
        return FDAPDE_OK;
    }

    // several columns against a symmetric positive system on one GPU: batches of 8 / 4 columns share every pass over the matrix (kernels_multirhs.h);
    // what is left goes column by column (pairs are faster that way: C3-size system, 77 ms against 92 ms batched)
    int batches() {
        if (!c->lin_sq_ready) {   // full-pattern scaled copy (explicit unit diagonal), once per prepared matrix
            HIPCHK(c, c->lin_sq.alloc((size_t)c->hs.nnz + 2));
            hipLaunchKernelGGL(k_scale_matrix, dim3(g1(n * 16)), dim3(256), 0, c->stream, n, c->rowptr.p, c->colidx.p, c->lin_mat.p, c->scale.p, c->lin_sq.p);
            c->lin_sq_ready = true;
        }
        while (n_rhs - t.j0 >= 4) {
            const int q = n_rhs - t.j0 >= 8 ? 8 : 4;
            int its = 0;
            double rel = 0;
            bool ok = true;
            const double* bq = b + (size_t)t.j0 * n;
            double* xq = x + (size_t)t.j0 * n;
            const int rc = q == 8 ? lin_solve_batch<8>(c, bq, xq, rtol, maxit, check_every, &its, &rel, &ok) : lin_solve_batch<4>(c, bq, xq, rtol, maxit, check_every, &its, &rel, &ok);
            if (rc != FDAPDE_OK) return rc;
            if (!ok) t.rc_all = FDAPDE_ENOCONV, t.breakdown = t.breakdown || c->h_ctl[2] != 0;   // (lin_solve_batch leaves h_ctl of its last read-back)
            t.total += its, t.worst = rel > t.worst ? rel : t.worst;
            c->info.method_used = method;
            t.j0 += q;
        }
        return FDAPDE_OK;
    }

    // ONE column against a system of one workgroup (a caller that cannot batch: 0.15 ms of wall time around a 50 us launch on the general path --
    // upload, two small kernels, the launch, two read-backs, three waits): the launch does it all (run_persist_direct).  *done: it ran, the record is
    // filled and the tally holds the column
    int direct_column(fdapde_info* info, bool* done) {
        const double tol2 = rtol * rtol;
        *done = false;
        if (int rc = run_persist_direct(c, 0, tol2, maxit, b, x, done)) return rc;
        if (!*done) return FDAPDE_OK;
        const Outcome out = outcome_from(c->h_sc, c->h_ctl, tol2);
        c->info.iters = c->h_ctl[1], c->info.relres = out.relres, c->info.converged = out.converged;
        c->info.method_used = method, c->info.persistent = 1, c->info.launch_ms = 0.0, c->info.t_solve_ms = 0.0;
        c->info.spmv_avg_ms = 0, c->info.spmv_timed = 0;
        if (info) *info = c->info;
        t.total = c->info.iters, t.worst = out.relres, t.breakdown = c->h_ctl[2] != 0, t.rc_all = out.converged ? FDAPDE_OK : FDAPDE_ENOCONV, t.j0 = 1;
        return FDAPDE_OK;
    }

    // several columns against a system the single-launch solver holds in few workgroups (the small systems the reference's users solve by the
    // thousand: one or two of 256 CUs busy per solve): Q columns side by side in ONE launch of G x Q workgroups, each column with boards of
    // its own; the same arithmetic per column as one by one, hence the same bits.  (A single column too: three small launches around the solve
    // instead of seven.)  Columns it leaves -- more workgroups than fit after all, a launch that gave up, a BiCGStab column that broke down (this
    // batch and what follows: solve_run_restarting restarts them) -- go one by one
    int columns_side_by_side(bool cols_bicg) {
        hipStream_t st = c->stream;
        fdapde_ctx::Persist& ps = c->ps[0];
        const int G = ps.meta.G;
        const int cap = (ps.per_cu > 0 ? ps.per_cu : 1) * c->n_cu / (G > 0 ? G : 1);   // columns whose workgroups are resident together
        const double tol2 = rtol * rtol;
        const int np = c->vec_grid;
        while (n_rhs - t.j0 >= 1 && cap >= 1) {
            const int Q = std::min(std::min<int>(n_rhs - t.j0, cap), 64);
            const size_t qn = (size_t)Q * (size_t)n;
            HIPCHK(c, c->cols_b.alloc(qn));
            HIPCHK(c, c->cols_r.alloc(qn));
            HIPCHK(c, c->cols_x.alloc(qn));
            HIPCHK(c, c->cols_sc.alloc(4 * (size_t)Q));
            HIPCHK(c, c->cols_ctl.alloc(4 * (size_t)Q));
            HIPCHK(c, c->cols_part.alloc(2 * (size_t)np * Q));
            HIPCHK(c, hipMemcpyAsync(c->cols_b.p, b + (size_t)t.j0 * n, sizeof(double) * qn, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_cols_init, dim3(np, Q), dim3(256), 0, st, n, c->cols_b.p, c->dof_i2e.p, c->scale.p, c->cols_r.p, c->cols_part.p);
            hipLaunchKernelGGL(k_cols_init_fin, dim3(Q), dim3(256), 0, st, c->cols_part.p, np, c->cols_sc.p, c->cols_ctl.p);
            HIPCHK(c, hipGetLastError());
            std::vector<int32_t> h_ctl(4 * (size_t)Q);
            std::vector<double> h_sc(4 * (size_t)Q);
            bool ran = false;
            if (int rc = run_persist_cols(c, 0, tol2, maxit, Q, c->cols_r.p, c->cols_x.p, c->cols_sc.p, c->cols_ctl.p, h_ctl.data(), h_sc.data(), &ran, cols_bicg))
                return rc;
            if (!ran) break;
            if (cols_bicg && c->bicg_restart) {
                bool broke = false;
                for (int k = 0; k < Q; ++k) broke = broke || h_ctl[4 * (size_t)k + 2] != 0;
                if (broke) break;
            }
            hipLaunchKernelGGL(k_cols_finish, dim3(g1(n), Q), dim3(256), 0, st, n, c->cols_x.p, c->scale.p, c->dof_i2e.p, c->cols_b.p);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(x + (size_t)t.j0 * n, c->cols_b.p, sizeof(double) * qn, hipMemcpyDeviceToHost, st));
            for (int k = 0; k < Q; ++k) {
                const Outcome out = outcome_from(&h_sc[4 * (size_t)k], &h_ctl[4 * (size_t)k], tol2);
                if (!out.converged) t.rc_all = FDAPDE_ENOCONV;
                t.breakdown = t.breakdown || h_ctl[4 * (size_t)k + 2] != 0;
                t.total += h_ctl[4 * (size_t)k + 1], t.worst = out.relres > t.worst ? out.relres : t.worst;
            }
            c->info.method_used = method, c->info.persistent = 1, c->info.launch_ms = c->persist_launch_ms;
            t.j0 += Q;
        }
        return FDAPDE_OK;
    }

    // column by column through the Krylov stages (solve_run_restarting): upload + gather, the solve, scatter + download, all on the one stream
    int columns_one_by_one(DebugClock& clk) {
        hipStream_t st = c->stream;
        for (int32_t j = t.j0; j < n_rhs; ++j) {
            HIPCHK(c, hipMemcpyAsync(c->tmp_e.p, b + (size_t)j * n, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_gather_f64, dim3(g1(n)), dim3(256), 0, st, n, c->dof_i2e.p, c->tmp_e.p, c->lin_rhs.p);
            clk.mark("lin_solve: upload + gather issued");
            c->defer_end_sync = true;
            const int rc = solve_run_restarting(c, c->lin_state->ss, c->lin_mat.p, c->lin_rhs.p, c->g.p, nullptr, method, rtol, maxit, check_every, 0, gm_budget);
            c->defer_end_sync = false;
            clk.mark("lin_solve: solve_run");
            if (rc != FDAPDE_OK && rc != FDAPDE_ENOCONV) return rc;
            if (rc == FDAPDE_ENOCONV) t.rc_all = rc, t.breakdown = t.breakdown || (c->h_ctl[2] != 0 && is_cg_method(c->info.method_used));
            t.total += c->info.iters, t.worst = c->info.relres > t.worst ? c->info.relres : t.worst;
            hipLaunchKernelGGL(k_scatter_f64, dim3(g1(n)), dim3(256), 0, st, n, c->dof_i2e.p, c->u.p, c->tmp_e.p);
            HIPCHK(c, hipMemcpyAsync(x + (size_t)j * n, c->tmp_e.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
            clk.mark("lin_solve: solution download issued");
        }
        return FDAPDE_OK;
    }
};

}   // namespace

// fdapde::SparseLU::solve(b) (fdaPDE/utils/symbols.h:148-155), dense right-hand sides: b, x column-major n_dofs x n_rhs
int e_lin_solve(fdapde_ctx* c, const fdapde_options* opt, const double* b, int32_t n_rhs, double* x, fdapde_info* info) {
    if (!c || !b || !x || n_rhs < 1) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->lin_ready) return fail(c, FDAPDE_ENOTINIT, "call fdapde_lin_compute first");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = c->hs.n_dofs;
    {   // in-place solves (x overlapping b: Eigen's x = lu.solve(x) idiom): finished columns are written to x while later columns and a
        // BiCGStab retry still read b -- work from a private copy of the right-hand sides
        const double *b0 = b, *b1 = b + (size_t)n * n_rhs, *x0 = x, *x1 = x + (size_t)n * n_rhs;
        if (b0 < x1 && x0 < b1) {
            std::vector<double> b_copy(b0, b1);
            return e_lin_solve(c, opt, b_copy.data(), n_rhs, x, info);
        }
    }
    if (opt && opt->method == FDAPDE_SOLVER_AMG) return amg_lin_solve(c, opt, b, n_rhs, x, info);   // (eng_amg.hip; after the in-place copy above)
    const SolveState& ss = c->lin_state->ss;
    const bool open_method = !opt || opt->method == FDAPDE_SOLVER_AUTO;
    LinCall L{c, b, x, n_rhs, n};   // (the rest below; the tally starts at zero)
    L.rtol = (opt && opt->rtol > 0) ? opt->rtol : 1e-10;
    L.maxit = (opt && opt->maxit > 0) ? opt->maxit : default_maxit(c, n);
    L.check_every = (opt && opt->check_every > 0) ? opt->check_every : 32;
    L.gm_budget = open_gmres_budget(c, opt, n);
    L.method = opt ? opt->method : FDAPDE_SOLVER_AUTO;
    if (L.method == FDAPDE_SOLVER_AUTO) L.method = (c->lin_symmetric && ss.diag_positive) ? FDAPDE_SOLVER_CG_FUSED : FDAPDE_SOLVER_BICGSTAB;
    const bool dense_named = opt && opt->method == FDAPDE_SOLVER_DENSE;
    if (dense_named && !dense_eligible(c)) return fail(c, FDAPDE_EUNSUPPORTED, kDenseRefusal);
    if ((open_method || dense_named) && dense_eligible(c)) {
        bool done = false;
        const int rc = L.dense_stage(dense_named, info, &done);
        if (rc || done) return rc;
    }
    c->lin_cols += n_rhs;
    struct KrylovClock {   // host time of this call's Krylov columns, towards the handle's rent-or-buy decision
        fdapde_ctx* c;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~KrylovClock() { c->lin_krylov_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    } krylov_clock{c};
    if (c->scaled_owner != fdapde_ctx::kScaledLin) {   // an elliptic / parabolic solve in between has overwritten scale and the scaled copy
        c->scaled_owner = fdapde_ctx::kScaledNone;      // (whatever init / set_* calls followed it): prepare again (cheap)
        if (int rc = solve_prepare(c, c->lin_mat.p, 0, &c->lin_state->ss, c->lin_symmetric)) return rc;
        c->scaled_owner = fdapde_ctx::kScaledLin;
    }
    c->solved = false;   // c->u is about to hold the handle's solutions, not PDE::solution()
    HIPCHK(c, c->lin_rhs.alloc((size_t)n));
    DebugClock clk;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    ColumnTally& t = L.t;
    // the handle was told "symmetric" and CG broke down: the matrix is not positive definite (3-D P2 mass matrices are not: negative quadrature
    // weight).  The reference's SparseLU does not care (utils/symbols.h:133-160): prepare the plain storage and solve every column with BiCGStab.
    auto retry_as_bicgstab = [&]() -> int {
        c->lin_symmetric = false, c->scaled_owner = fdapde_ctx::kScaledNone;
        if (int rc = solve_prepare(c, c->lin_mat.p, 0, &c->lin_state->ss, false)) return rc;
        c->scaled_owner = fdapde_ctx::kScaledLin, c->lin_sq_ready = false;
        const int spent = t.total;   // the CG iterations before the breakdown count
        c->lin_cols -= n_rhs;        // (the same columns again: counted once)
        const int rc = e_lin_solve(c, opt, b, n_rhs, x, info);
        c->info.iters += spent;
        if (info) info->iters = c->info.iters;
        return rc;
    };
    const bool one_gpu = !ss.dist && !ss.rowdist;
    const bool cgf = L.method == FDAPDE_SOLVER_CG_FUSED;
    const bool may_retry = c->lin_symmetric && open_method && cgf && one_gpu;
    // (a system the persistent CG takes is faster column by column -- one launch each, no vector traffic -- than batched through
    // the multi-launch SpMM: C3-size, 22.5 ms per column against 32 ms per column in a batch of 8)
    const bool persist_cols = c->persist && !c->persist_broken && c->ps[0].ok && c->ps[0].filled && c->ps[0].meta.R <= kPersistRmax;   // (the wide form: one column)
    if (c->multi_rhs && n_rhs >= 4 && cgf && one_gpu && !persist_cols)
        if (int rc = L.batches()) return rc;
    const bool side_by_side = persist_cols && c->persist_cols && one_gpu && !ss.use_bnd;
    if (n_rhs == 1 && side_by_side && c->persist_direct && cgf && c->ps[0].meta.G == 1) {
        bool done = false;
        if (int rc = L.direct_column(info, &done)) return rc;
        if (done) {
            if (t.rc_all == FDAPDE_OK) return FDAPDE_OK;
            if (t.breakdown && may_retry) return retry_as_bicgstab();
            c->err = t.breakdown ? "Krylov breakdown (operator not SPD for CG)" : "maxit reached";
            return FDAPDE_ENOCONV;
        }
    }
    const bool cols_bicg = L.method == FDAPDE_SOLVER_BICGSTAB && c->persist_bicg && !c->ps[0].meta.sym && c->ps[0].meta.R <= 8;   // (the single-launch BiCGStab's own limits)
    if (side_by_side && (cgf || cols_bicg))
        if (int rc = L.columns_side_by_side(cols_bicg)) return rc;
    if (int rc = L.columns_one_by_one(clk)) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    if (t.rc_all == FDAPDE_ENOCONV && t.breakdown && may_retry) return retry_as_bicgstab();
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->info.t_solve_ms = ms, c->info.iters = t.total, c->info.relres = t.worst, c->info.converged = t.rc_all == FDAPDE_OK ? 1 : 0;
    if (t.rc_all == FDAPDE_ENOCONV)
        c->err = t.breakdown ? "Krylov breakdown in at least one column (matrix not positive definite for CG, or BiCGStab rho / omega = 0)" : "maxit reached in at least one column";
    if (info) *info = c->info;
    return t.rc_all;
}

int e_matrix_values(fdapde_ctx* c, int32_t which, double* values) {
    if (!c || !values || which < 0 || which > 1) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready || !c->assembled[which]) return fail(c, FDAPDE_ENOTINIT, "matrix not assembled");
    HIPCHK(c, hipSetDevice(c->device));
    const HostSpace& hs = c->hs;
    const int zero_rows = (which == FDAPDE_MAT_STIFF && c->dirichlet_applied) ? 1 : 0;
    hipLaunchKernelGGL(k_export_values, dim3(g1(hs.n_dofs * 16)), dim3(256), 0, c->stream, hs.n_dofs, c->rowptr.p, c->colidx.p,
                       c->vals[which].p, c->slot_i2e.p, c->bnd.p, zero_rows, c->tmp_v.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(values, c->tmp_v.p, sizeof(double) * (size_t)hs.nnz, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FDAPDE_OK;
}

// lump(stiff() | mass()) (fdaPDE/linear_algebra/lumping.h:30-41): the diagonal of the row-sum lumped matrix, reference numbering
int e_lump(fdapde_ctx* c, int32_t which, double* diag) {
    if (!c || !diag || which < 0 || which > 1) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready || !c->assembled[which]) return fail(c, FDAPDE_ENOTINIT, "matrix not assembled");
    HIPCHK(c, hipSetDevice(c->device));
    const HostSpace& hs = c->hs;
    hipLaunchKernelGGL(k_row_sums, dim3(g1(hs.n_dofs * 16)), dim3(256), 0, c->stream, hs.n_dofs, c->rowptr.p, c->vals[which].p, c->tmp_i.p);
    hipLaunchKernelGGL(k_scatter_f64, dim3(g1(hs.n_dofs)), dim3(256), 0, c->stream, hs.n_dofs, c->dof_i2e.p, c->tmp_i.p, c->tmp_e.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(diag, c->tmp_e.p, sizeof(double) * (size_t)hs.n_dofs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FDAPDE_OK;
}

int e_force(fdapde_ctx* c, double* force) {
    if (!c || !force) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready || !c->force_ready) return fail(c, FDAPDE_ENOTINIT, "force not assembled");
    HIPCHK(c, hipSetDevice(c->device));
    const HostSpace& hs = c->hs;
    const int cols = c->fq_cols > 0 ? c->fq_cols : 1;
    for (int col = 0; col < cols; ++col) {
        HIPCHK(c, hipMemcpyAsync(c->tmp_i.p, c->force.p + (size_t)col * hs.n_dofs, sizeof(double) * (size_t)hs.n_dofs,
                                 hipMemcpyDeviceToDevice, c->stream));
        if (col == 0 && c->dirichlet_applied)
            hipLaunchKernelGGL(k_force_bc, dim3(g1(hs.n_dofs)), dim3(256), 0, c->stream, hs.n_dofs, c->bnd.p, c->g.p, c->tmp_i.p);
        hipLaunchKernelGGL(k_scatter_f64, dim3(g1(hs.n_dofs)), dim3(256), 0, c->stream, hs.n_dofs, c->dof_i2e.p, c->tmp_i.p, c->tmp_e.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(force + (size_t)col * hs.n_dofs, c->tmp_e.p, sizeof(double) * (size_t)hs.n_dofs,
                                 hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return FDAPDE_OK;
}

int e_solution(fdapde_ctx* c, double* solution) {
    if (!c || !solution) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->solved) return fail(c, FDAPDE_ENOTINIT, "no solution: call fdapde_solve first");
    HIPCHK(c, hipSetDevice(c->device));
    const HostSpace& hs = c->hs;
    hipLaunchKernelGGL(k_scatter_f64, dim3(g1(hs.n_dofs)), dim3(256), 0, c->stream, hs.n_dofs, c->dof_i2e.p, c->u.p, c->tmp_e.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(solution, c->tmp_e.p, sizeof(double) * (size_t)hs.n_dofs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FDAPDE_OK;
}

int e_spmv(fdapde_ctx* c, int32_t which, const double* x, double* y) {
    if (!c || !x || !y || which < 0 || which > 1) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready || !c->assembled[which]) return fail(c, FDAPDE_ENOTINIT, "matrix not assembled");
    HIPCHK(c, hipSetDevice(c->device));
    const HostSpace& hs = c->hs;
    const size_t bytes = sizeof(double) * (size_t)hs.n_dofs;
    HIPCHK(c, hipMemcpyAsync(c->tmp_e.p, x, bytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_gather_f64, dim3(g1(hs.n_dofs)), dim3(256), 0, c->stream, hs.n_dofs, c->dof_i2e.p, c->tmp_e.p, c->tmp_i.p);
    launch_spmv(c, c->vals[which].p, c->tmp_i.p, c->t.p, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(k_scatter_f64, dim3(g1(hs.n_dofs)), dim3(256), 0, c->stream, hs.n_dofs, c->dof_i2e.p, c->t.p, c->tmp_e.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(y, c->tmp_e.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FDAPDE_OK;
}

int e_bench_spmv(fdapde_ctx* c, int32_t reps, double* avg_ms, double* algorithmic_bytes) {
    if (!c || reps < 1) return FDAPDE_EINVAL;
    if (int rc = need_device(c)) return rc;
    if (!c->dev_ready || !c->assembled[0]) return fail(c, FDAPDE_ENOTINIT, "matrix not assembled");
    HIPCHK(c, hipSetDevice(c->device));
    const HostSpace& hs = c->hs;
    // the launch timed here is the one inside CG: scaled matrix stream, fused p.Ap partials
    const double* A = (c->solved && c->scaled_owner == fdapde_ctx::kScaledSolve) ? c->sval.p : c->vals[0].p;
    if (A == c->sval.p)
        if (int rc = ensure_sval(c)) return rc;
    hipLaunchKernelGGL(k_fill_f64, dim3(g1(hs.n_dofs)), dim3(256), 0, c->stream, hs.n_dofs, 1.0, c->tmp_i.p);
    for (int i = 0; i < 3; ++i) launch_spmv(c, A, c->tmp_i.p, c->t.p, c->tmp_i.p, c->part_a.p, nullptr);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < reps; ++i) launch_spmv(c, A, c->tmp_i.p, c->t.p, c->tmp_i.p, c->part_a.p, nullptr);
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (avg_ms) *avg_ms = (double)ms / reps;
    if (algorithmic_bytes) *algorithmic_bytes = 12.0 * (double)hs.nnz + 4.0 * (double)(hs.n_dofs + 1) + 16.0 * (double)hs.n_dofs;
    return FDAPDE_OK;
}


// the unit's code object is loaded when one of its kernels is first looked up (HIP defers it): done at context creation, so that the
// first solve of a process does not pay for it (6 ms for the smoke problem after the library was split into units)
void preload_solve() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&k_jacobi_scale));
    (void)hipGetLastError();
}

}   // namespace fdapde_engine
