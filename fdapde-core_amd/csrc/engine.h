// engine.h -- what the translation units of libfdapde_hip.so share besides the context: small helpers and the entry points of the
// internal engines.  capi.hip holds the C ABI and the multi-launch solve driver; persist_engine.hip the single-launch solver
// (layouts, launches, the row-distributed multi-GPU form).  Internal to the library.
#ifndef FDAPDE_ENGINE_H
#define FDAPDE_ENGINE_H

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

#include "context.h"

namespace fdapde_hip {
struct ObsHost;   // host_obs.h
}
namespace fdapde_engine {

// FDAPDE_DEBUG_TIMING=1: wall-clock marks of the host side of a solve on stderr (where a first solve spends its time)
struct DebugClock {
    bool on = std::getenv("FDAPDE_DEBUG_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void mark(const char* what) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[timing] %-34s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

inline int fail(fdapde_ctx* c, int code, const char* msg) {
    c->err = msg;
    return code;
}
inline int need_device(fdapde_ctx* c) {
    if (!c->has_device) return fail(c, FDAPDE_ENODEVICE, "this context has no HIP device (host-only); there is no CPU fallback");
    return FDAPDE_OK;
}

// ---- what fdapde_solve, the parabolic stepper, fdapde_lin_solve and the operator handles (eng_handle.h) say and decide alike
// the outcome of a Krylov run as its kernels leave it: sc[0] = |b|^2, sc[3] = |r|^2, ctl[2] = the breakdown word
struct Outcome { double relres; int converged; };
inline Outcome outcome_of(double bb, double rr, bool broke, double tol2) { return {bb > 0 ? std::sqrt(rr / bb) : 0.0, (rr <= tol2 * bb && !broke) ? 1 : 0}; }
inline Outcome outcome_from(const double* h_sc, const int32_t* h_ctl, double tol2) { return outcome_of(h_sc[0], h_sc[3], h_ctl[2] != 0, tol2); }
// FDAPDE_SOLVER_DENSE's report of a matrix (`what`) it could not invert
inline std::string dense_singular(const std::string& what) {
    return "FDAPDE_SOLVER_DENSE: " + what + " is singular to working precision (no usable pivot, or max |I - A X| beyond 1e-6)";
}
// a call that ends before any solve: the record names the method (and the inverse's check), nothing of an earlier solve stays in it
inline int bare_answer(fdapde_ctx* c, int method, double check, fdapde_info* info, int rc) {
    c->info = fdapde_info{};
    c->info.method_used = method, c->info.relres = check;
    if (info) *info = c->info;
    return rc;
}

// a DBuf takes over a device array built elsewhere (dev_setup.hip)
template <typename T> void adopt(DBuf<T>& b, T*& p, size_t n) {
    b.release();
    b.p = p, b.n = n, p = nullptr;
}


inline unsigned grid1(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// big host-side index arrays of a device-built space, fetched the first time host code needs them (capi.hip)
// kHostPerm: the permutations (dof_i2e, dof_e2i, cell_i2e) and the boundary flags in internal order (dof_bnd_i); implied by kHostPattern
enum { kHostPattern = 1, kHostCells = 2, kHostRefPattern = 4, kHostDofs = 8, kHostPerm = 16 };
int ensure_host(fdapde_ctx* c, int what);

inline unsigned g1(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

#define RCCLCHK(ctx, expr)                                                                   \
    do {                                                                                     \
        ncclResult_t r__ = (expr);                                                           \
        if (r__ != ncclSuccess) {                                                            \
            (ctx)->err = std::string(#expr) + ": " + g_rccl.GetErrorString(r__);             \
            return FDAPDE_ERCCL;                                                             \
        }                                                                                    \
    } while (0)

// ---- helpers one engine unit offers the others ---------------------------------------------------------------------------------------
int ensure_sval(fdapde_ctx* c);                                            // eng_solve.hip: the scaled full-pattern copy, if a solve skipped it
void drop_graph(fdapde_ctx* c);                                            // eng_solve.hip: the captured CG chunk bakes pointers and sizes in
int ranks_saying_yes(fdapde_ctx* c, bool mine, int* yes);                // eng_dist.hip: how many ranks of the job answer yes (COLLECTIVE)
int allreduce_sum(fdapde_ctx* c, double* buf, size_t count);               // eng_dist.hip: device buffer summed over the ranks
int halo_sum(fdapde_ctx* c, double* v, const double* part, int np, bool unpack = true);   // eng_dist.hip: interface entries summed over the sharing ranks

int ensure_eval_grid(fdapde_ctx* c);                                       // eng_assembly.hip: the bin grid of point location and projection, once per mesh

// ---- the bodies behind the C ABI (capi.hip forwards to them; each unit's header comment says what it holds) ----------------------------
int e_ctx_clone(const fdapde_ctx* src, fdapde_ctx* dst);   // eng_clone.hip
int clone_state(const fdapde_ctx* src, fdapde_ctx* dst);   // ... its second half: problem data + assembled / solved state onto an identical space
int g_clone(const fdapde_ctx* src_root, fdapde_ctx** out);   // eng_group.hip
int e_dofs_build(fdapde_ctx* c, int order, int64_t* n_dofs);
int e_topology_build(fdapde_ctx* c, int64_t* n_facets, int64_t* n_edges);
int e_topology_get(fdapde_ctx* c, int32_t* neighbors, int32_t* cell_facets, int32_t* facet_nodes, int32_t* facet_cells, uint8_t* facet_boundary, int32_t* edge_nodes, uint8_t* edge_boundary, int32_t* face_edges);
int e_dofs_set_boundary(fdapde_ctx* c, const uint8_t* bnd);
int e_dofs_get(const fdapde_ctx* c, int32_t* dofs, uint8_t* bnd, double* coords);
int e_pattern_get(const fdapde_ctx* c, int32_t* rowptr, int32_t* colidx);
int e_quadrature_nodes(fdapde_ctx* c, double* out);
int e_set_operator(fdapde_ctx* c, int32_t n_terms, const fdapde_term* terms);
int e_set_forcing(fdapde_ctx* c, const double* f_q, int32_t n_cols);
int e_set_dirichlet(fdapde_ctx* c, const double* g);
int e_assemble_operator(fdapde_ctx* c, int32_t which, int32_t n_terms, const fdapde_term* terms, int32_t assembly);
int e_init(fdapde_ctx* c, const fdapde_options* opt);
int e_eval_pointwise(fdapde_ctx* c, int64_t n_locs, const double* locs_colmajor, int32_t* cell_ids, double* values);
int e_cell_integrals(fdapde_ctx* c, double* measure, double* psi_int);
int e_project(fdapde_ctx* c, int64_t n_pts, const double* pts_colmajor, int32_t* cell_ids, double* proj_colmajor, double* dist, double* values);   // eng_project.hip
int e_solver_prepare(fdapde_ctx* c, int32_t with_dirichlet);
int e_solver_layout(fdapde_ctx* c, int32_t with_dirichlet, int64_t* n_interior, int64_t* nnz_interior, double* streamed_bytes);
int e_solver_layout_kind(fdapde_ctx* c, int32_t with_dirichlet, int32_t* kind, int32_t* symmetric_storage, int32_t* workgroups, int32_t* rows_per_thread);
int e_solve(fdapde_ctx* c, const fdapde_options* opt, fdapde_info* info);
int e_solve_parabolic(fdapde_ctx* c, const fdapde_options* opt, int32_t n_times, double delta_t, const double* initial_condition, const double* dirichlet, double* solution, fdapde_info* info);
int e_lin_compute(fdapde_ctx* c, int32_t which, const double* values, int32_t symmetric);
int e_lin_solve(fdapde_ctx* c, const fdapde_options* opt, const double* b, int32_t n_rhs, double* x, fdapde_info* info);
int e_matrix_values(fdapde_ctx* c, int32_t which, double* values);
int e_lump(fdapde_ctx* c, int32_t which, double* diag);
int e_force(fdapde_ctx* c, double* force);
int e_solution(fdapde_ctx* c, double* solution);
int e_spmv(fdapde_ctx* c, int32_t which, const double* x, double* y);
int e_bench_spmv(fdapde_ctx* c, int32_t reps, double* avg_ms, double* algorithmic_bytes);
int e_comm_unique_id(void* out128);
int e_comm_init(fdapde_ctx* c, int32_t world, int32_t rank, const void* unique_id128);
int e_comm_allreduce(fdapde_ctx* c, double* host_inout, int32_t n, int32_t op);
int e_comm_count(fdapde_ctx* c, int32_t* ranks);
int e_comm_init_callback(fdapde_ctx* c, int32_t world, int32_t rank, fdapde_allreduce_fn fn, void* user);
int e_halo_setup(fdapde_ctx* c, int64_t n_if_global, int64_t n_if_local, const int32_t* local_dof, const int32_t* if_index, const uint8_t* owned);
int e_rowdist_setup(fdapde_ctx* c, const int64_t* dof_key, const int32_t* dof_owner);
int e_comm_set_exchange_callback(fdapde_ctx* c, fdapde_exchange_fn fn, void* user);
int e_halo_setup_peers(fdapde_ctx* c, int32_t n_peers, const int32_t* peer_rank, const int64_t* peer_off, const int32_t* peer_dof, const uint8_t* owned);

// ---- the device-side partitioner's public face and the multi-device context (eng_group.hip) ------------------------------------------------
int e_partition_build(fdapde_ctx* c, int32_t world, int32_t form);
int e_partition_sizes(const fdapde_ctx* c, int32_t rank, int64_t* n_nodes, int64_t* n_cells);
int e_partition_get(fdapde_ctx* c, int32_t rank, double* nodes_colmajor, int32_t* cells, uint8_t* boundary, int64_t* node_ids, int64_t* cell_ids, int32_t* node_owner);
int e_partition_whole(fdapde_ctx* c, int32_t* cell_rank, int32_t* node_owner, uint64_t* node_ranks);
int e_partition_peers(fdapde_ctx* c, int32_t rank, int32_t* n_peers, int32_t* peer_rank, int64_t* peer_off, int32_t* peer_node, uint8_t* owned, int64_t* n_shared);
void partition_free(fdapde_ctx* c);
int g_create(const int32_t* devices, int32_t n, fdapde_ctx** out);
void g_destroy(fdapde_ctx* root);
int g_info(const fdapde_ctx* root, int32_t* n_devices, int32_t* devices, int32_t* form, double* t_partition_ms, double* t_rank_setup_ms);
void g_mesh_changed(fdapde_ctx* root);
int g_dofs_build(fdapde_ctx* root, int order, int64_t* n_dofs);
int g_dofs_set_boundary(fdapde_ctx* root, const uint8_t* bnd);
int g_set_operator(fdapde_ctx* root, int32_t n_terms, const fdapde_term* terms);
int g_assemble_operator(fdapde_ctx* root, int32_t which, int32_t n_terms, const fdapde_term* terms, int32_t assembly);
int g_set_forcing(fdapde_ctx* root, const double* f_q, int32_t n_cols);
int g_set_dirichlet(fdapde_ctx* root, const double* g);
int g_init(fdapde_ctx* root, const fdapde_options* opt);
int g_solver_prepare(fdapde_ctx* root, int32_t with_dirichlet);
int g_solve(fdapde_ctx* root, const fdapde_options* opt, fdapde_info* info);
int g_solution(fdapde_ctx* root, double* solution);
int g_force(fdapde_ctx* root, double* force);
int g_lump(fdapde_ctx* root, int32_t which, double* diag);
int g_matrix_values(fdapde_ctx* root, int32_t which, double* values);
int g_spmv(fdapde_ctx* root, int32_t which, const double* x, double* y);
int g_solve_parabolic(fdapde_ctx* root, const fdapde_options* opt, int32_t n_times, double delta_t, const double* initial_condition, const double* dirichlet, double* solution, fdapde_info* info);
int g_lin_compute(fdapde_ctx* root, int32_t which, const double* values, int32_t symmetric);
int g_lin_solve(fdapde_ctx* root, const fdapde_options* opt, const double* b, int32_t n_rhs, double* x, fdapde_info* info);
int g_tune(fdapde_ctx* root, const char* key, int32_t value);
int g_synchronize(fdapde_ctx* root);
int g_layout_kind(fdapde_ctx* root, int32_t with_dirichlet, int32_t* kind, int32_t* symmetric_storage, int32_t* workgroups, int32_t* rows_per_thread);

// ---- dense inverse of small systems (eng_dense.hip)
bool dense_eligible(const fdapde_ctx* c);
double dense_build_estimate_ms(int64_t n);
int dense_build(fdapde_ctx* c, const double* A, int use_bnd, fdapde_ctx::Dense& D);
// ... of any CSR matrix of n rows (device arrays; bnd may be null where use_bnd = 0)
int dense_build_csr(fdapde_ctx* c, int64_t n, const int32_t* rowptr, const int32_t* colidx, const double* A, const uint8_t* bnd, int use_bnd, fdapde_ctx::Dense& D);
int dense_apply(fdapde_ctx* c, fdapde_ctx::Dense& D, int nc, const double* b, double* x);
int dense_solve_host(fdapde_ctx* c, fdapde_ctx::Dense& D, const double* b_host, int nc, double* x_host);
int dense_direct(fdapde_ctx* c, const double* A, int use_bnd, const double* f_dev, const double* g_dev, bool* solved);
void dense_step_rhs(fdapde_ctx* c, const double* mu, double inv_dt, const double* f, const double* g_ext_dev, double* rhs);
void dense_step_out(fdapde_ctx* c, const double* u, double* uprev, double* sol_ext_dev);
// eng_solve.hip: the blocked-ELL SpMV layout of boundary variant v (c->bk[v]; ok = false where the system does not take it) and its launch on whatever ell_val holds
int build_blocked(fdapde_ctx* c, int v);
void launch_spmv_blocked(fdapde_ctx* c, int v, const double* x, double* y, const double* w, double* partial, const int32_t* stop, hipEvent_t e0, hipEvent_t e1, int dot2_ww);
// eng_solve.hip: the coarse-level solves of the two-level solver -- the solver prepared once per coarse operator, then one run per right-hand side (c->force)
int coarse_prepare(fdapde_ctx* c, SolveState* ss);
int coarse_solve(fdapde_ctx* c, SolveState* ss, double rtol, int maxit, fdapde_info* info);
// eng_pmg.hip
bool pmg_eligible(const fdapde_ctx* c);
void pmg_release(fdapde_ctx* c);
int e_solve_pmg(fdapde_ctx* c, const fdapde_options* opt, fdapde_info* info);
int pmg_run(fdapde_ctx* c, const double* A, const double* f_dev, const double* g_dev, int use_bnd, const double* x0_dev, double extra_reaction, int64_t coarse_key,
            double rtol, int maxit);
// the flexible GMRES outer loop (eng_pmg.hip) for Q in {1, 2, 4, 8} columns in lockstep and its basis: interleaved vectors (kernels_cols.h), n words per
// column, V_0 .. V_mk, Z_0 .. Z_{mk-1} (n Q apart), part >= (mk + 2) Q np, dots >= (mk + 4) Q doubles
struct FgmresSpace {
    int64_t n;
    int mk;
    double *V, *Z, *part, *dots;
    int np;
};
// per column: in rr / bb / converged / broke, out also it and handed (Q > 1 only -- the recurrence said "converged", the true residual did not: the caller
// finishes that column at Q = 1 from its iterate; a single column restarts inside the loop)
struct FgmresCols {
    double rr[8], bb[8];
    int it[8];
    bool converged[8], broke[8], handed[8];
};
int fgmres_outer(fdapde_ctx* c, const FgmresSpace& s, int Q, double* x, double* r, const double* comb_dinv, double rtol, int maxit,
                 const std::function<int(const double*, double*, double*, bool&)>& precond, const std::function<int(double*)>& residual, FgmresCols& S);
// three dot products of single vectors (the BiCGStab outer method, the power iterations), and one per column of Q interleaved columns: the bits of the first
void fixed_dots(hipStream_t st, int64_t n, int np, const double* a0, const double* b0, const double* a1, const double* b1, const double* a2, const double* b2,
                double* part, double* out);
void fixed_dots_cols(hipStream_t st, int64_t n, int np, int Q, const double* a, const double* b, double* part, double* out);
// eng_amg.hip: FDAPDE_SOLVER_AMG
bool amg_eligible(const fdapde_ctx* c);
void amg_release(fdapde_ctx* c);
void amg_forget(fdapde_ctx* c);   // the fdapde_solve hierarchy no longer matches (the stepper built its own on a K of the call)
int amg_lin_solve(fdapde_ctx* c, const fdapde_options* opt, const double* b, int32_t n_rhs, double* x, fdapde_info* info);
int e_solve_amg(fdapde_ctx* c, const fdapde_options* opt, fdapde_info* info);
// one solve of K u = rhs against the hierarchy h (K: A with the Dirichlet rows as unit rows if use_bnd; rhs = f on the free rows, g on the Dirichlet rows),
// from x0_dev or from g / 0; result in c->u, outcome in c->info
int amg_run(fdapde_ctx* c, AmgHierarchy* h, const double* A, const double* f_dev, const double* g_dev, int use_bnd, const double* x0_dev, double rtol, int maxit);
// (re)build hierarchy *slot for A on the context's pattern (use_bnd: the Dirichlet DOFs belong to no aggregate)
int amg_build(fdapde_ctx* c, AmgHierarchy** slot, const double* A, int use_bnd, bool symmetric);
// fdapde_amg_hierarchy: levels, rows and entries per level (the first `cap` of them), whether the passes absorbed, what the set-up cost; FDAPDE_ENOTINIT for NULL
int amg_describe(const AmgHierarchy* h, int32_t cap, int32_t* n_levels, int64_t* rows, int64_t* nnz, int32_t* absorbed, double* setup_ms);
// fdapde_amg_cols_trace: the hierarchy's Q-column runs, the columns they took, the columns solved one by one; FDAPDE_ENOTINIT for NULL
int amg_cols_trace(const AmgHierarchy* h, int32_t* batches, int32_t* batched_cols, int32_t* single_cols);
int amg_lin_cols_trace(const fdapde_ctx* c, int32_t* batches, int32_t* batched_cols, int32_t* single_cols);   // the handle's (none once fdapde_lin_compute has outlived it)
const AmgHierarchy* amg_lin_live(const fdapde_ctx* c);   // the handle's hierarchy, NULL once fdapde_lin_compute has outlived it
// fdapde_amg_aggregates: the map row -> row of the next level of `level` (level 0 in the reference DOF numbering, -1: a row of no aggregate), for the scalar
// hierarchies and the block form's alike; FDAPDE_ENOTINIT for NULL, FDAPDE_EINVAL for a level without a next one, a NULL agg or cap < the level's rows
int amg_aggregates(fdapde_ctx* c, const AmgHierarchy* h, int32_t level, int64_t cap, int32_t* agg, int64_t* n_rows);
// fdapde_amg_order: the reference DOF of every row of level 0, in the level's own order; FDAPDE_ENOTINIT for NULL, FDAPDE_EINVAL for a NULL order or cap < its rows
int amg_order(fdapde_ctx* c, const AmgHierarchy* h, int64_t cap, int32_t* order, int64_t* n_rows);
// fdapde_amg_damping: the smoother's damping of the first `cap` levels, 0 on the last one; FDAPDE_ENOTINIT for NULL
int amg_damping(const AmgHierarchy* h, int32_t cap, int32_t* n_levels, double* omega);
int block_amg_cols_trace_ctx(const fdapde_ctx* c, int32_t* batches, int32_t* batched_cols, int32_t* single_cols);
int dense_step_loop(fdapde_ctx* c, fdapde_ctx::Dense& D, int32_t n_times, double inv_dt, const double* g_ext_dev, double* u0, double* sol_ext);
void preload_dense();
// eng_block.hip: 2 x 2 block systems on the FEM pattern (the smoothing system's handle) and Psi^T W Psi on that pattern
void block_release(fdapde_ctx* c);
void block_amg_forget(fdapde_ctx* c);   // the block handle's hierarchy is built again by its next solve (a set-up knob changed)
int block_amg_describe_ctx(const fdapde_ctx* c, int32_t cap, int32_t* n_levels, int64_t* rows, int64_t* nnz, int32_t* absorbed, double* setup_ms);
int block_amg_aggregates_ctx(fdapde_ctx* c, int32_t level, int64_t cap, int32_t* agg, int64_t* n_rows);
int block_amg_damping_ctx(const fdapde_ctx* c, int32_t cap, int32_t* n_levels, double* omega);
int block_amg_order_ctx(fdapde_ctx* c, int64_t cap, int32_t* order, int64_t* n_rows);
int e_block_compute(fdapde_ctx* c, const double* a11, const double* a12, const double* a21, const double* a22, int32_t symmetric);
int e_block_solve(fdapde_ctx* c, const fdapde_options* opt, const double* b, int32_t n_rhs, double* x, fdapde_info* info);
int e_block_spmv(fdapde_ctx* c, const double* x, double* y);
int e_block_bench_spmv(fdapde_ctx* c, int32_t reps, double* avg_ms, double* algorithmic_bytes);
int e_block_set_obs(fdapde_ctx* c, int64_t n_obs, const int64_t* rowptr, const int32_t* colidx, const double* values, const double* weights, double scale);
int e_block_obs_info(fdapde_ctx* c, int64_t* n_obs, int64_t* nnz, int32_t* team_rows, int32_t* team_cols);
int e_block_amg_obs_levels(fdapde_ctx* c, int32_t cap, int32_t* n_levels, int64_t* nnz, int32_t* longest_row, int32_t* team_rows, int32_t* team_cols);
int e_gram_pointwise(fdapde_ctx* c, int64_t n_locs, const int32_t* cell_ids, const double* values, const double* weights, double* out_values);
// eng_kron.hip: Kronecker-sum operators sum_k T_k (x) S_k, T_k dense q x q, S_k on the FEM pattern (the space-time systems' handle)
void kron_release(fdapde_ctx* c);
int e_kron_compute(fdapde_ctx* c, int32_t q, int32_t n_terms, const double* const* T, const double* const* S, int32_t symmetric);
int e_kron_solve(fdapde_ctx* c, const fdapde_options* opt, const double* b, int32_t n_rhs, double* x, fdapde_info* info);
int e_kron_spmv(fdapde_ctx* c, const double* x, double* y);
int e_kron_bench_spmv(fdapde_ctx* c, int32_t reps, double* avg_ms, double* algorithmic_bytes);
int e_kron_set_obs(fdapde_ctx* c, int32_t p, const double* Phi, int64_t n_obs, const int64_t* rowptr, const int32_t* colidx, const double* values,
                   const double* weights, double scale);
int e_kron_obs_info(fdapde_ctx* c, int32_t* p, int64_t* n_obs, int64_t* nnz, int32_t* form_rows, int32_t* form_cols);
void kron_amg_forget(fdapde_ctx* c);   // the Kronecker handle's hierarchy is built again by its next solve (a set-up knob changed)
int kron_amg_describe_ctx(const fdapde_ctx* c, int32_t cap, int32_t* n_levels, int64_t* rows, int64_t* nnz, int32_t* absorbed, double* setup_ms);
int kron_amg_aggregates_ctx(fdapde_ctx* c, int32_t level, int64_t cap, int32_t* agg, int64_t* n_rows);

// eng_kron_amg.hip: FDAPDE_SOLVER_KRON_AMG, the point-block multilevel preconditioner of the Kronecker-sum handle -- the hierarchy of the handle's factors
// (a KronAmg, amg_setup.h) on the context's pattern (src: the handle's device arrays, tnorm the Frobenius norms of its time factors, pick the spatial factor the aggregation reads or
// -1 for the weighted sum of magnitudes), and one column A x = b against it (b, x: interleaved, internal order, device)
struct KronAmg;
struct KronAmgSource {
    int q, ns, Q;
    bool t_in_lds;
    const double *vals, *tm, *dinv;
    const int32_t* band;
    double tnorm[8];
    int pick;
};
void kron_amg_free(KronAmg* h);
int kron_amg_build(fdapde_ctx* c, KronAmg** slot, const KronAmgSource& src);
int kron_amg_run(fdapde_ctx* c, KronAmg* h, const double* b_dev, double* x_dev, double rtol, int maxit, int* iters, double* relres, bool* converged, bool* broke);

// eng_block_amg.hip: FDAPDE_SOLVER_BLOCK_AMG, the point-block multilevel preconditioner of the block handle -- the hierarchy (a BlockAmg, amg_setup.h) of the unscaled block CSR
// `raw` on the context's pattern (strength_block: which of a11 a12 a21 a22 the aggregation reads), and one column A x = b against it (b, x: interleaved,
// internal order, device)
struct BlockAmg;
// the handle's live factored data term as the hierarchy takes it (knob block_amg_obs): Psi and Psi^T in the internal order on the device, the host copy the
// coarsening starts from, the weights, the term's share g of level 0's diagonal blocks; the arrays outlive the hierarchy (a change of the term drops it)
struct BlockAmgTerm {
    const fdapde_hip::ObsHost* host;
    double scale;
    int team_rows, team_cols;   // level 0's lanes per row of Psi / of Psi^T
    int team_knob;              // block_obs_team as fdapde_block_set_obs read it: the coarse levels' widths follow it too
    const int32_t *rp, *ci, *trp, *tci;
    const double *v, *tv, *w, *g;
};
void block_amg_free(BlockAmg* h);
int block_amg_build(fdapde_ctx* c, BlockAmg** slot, const double* raw, int strength_block, const BlockAmgTerm* term = nullptr);
// fdapde_block_obs_amg_levels: per level nnz(Psi_l), its longest row, the lanes per row of Psi_l / Psi_l^T; term_ms: the term's share of the set-up;
// FDAPDE_ENOTINIT where h is NULL or carries no term
int block_amg_obs_levels(const BlockAmg* h, int32_t cap, int32_t* n_levels, int64_t* nnz, int32_t* longest_row, int32_t* team_rows, int32_t* team_cols, double* term_ms);
bool block_amg_has_term(const BlockAmg* h);
int block_amg_run(fdapde_ctx* c, BlockAmg* h, const double* raw, const double* b_dev, double* x_dev, double rtol, int maxit, int* iters, double* relres,
                  bool* converged, bool* broke, bool warm = false);   // warm: x_dev holds the iterate to start from (a column a batch handed back)
// Q in {2, 4, 8} columns side by side (knob amg_cols; block_amg_width: the widest batch for `left` columns): ext (device) holds the stacked columns in the
// reference numbering and receives the solutions; col_b, col_x: a column of scratch each.  Adds to *iters, follows block_amg_solve's rules for the rest
int block_amg_width(const fdapde_ctx* c, const BlockAmg* h, int32_t left, int maxit);
int block_amg_batch(fdapde_ctx* c, BlockAmg* h, const double* raw, int Q, double* ext, double* col_b, double* col_x, double rtol, int maxit, int* iters, double* worst,
                    bool* not_conv, bool* broke_any);

// code objects of the units loaded up front (fdapde_ctx_create)
void preload_assembly();
void preload_solve();
void preload_dist();
void preload_persist();
// ... and those of the set-up units (13 + 6 + 6 MB of device code: 30 ms to load), on a helper thread started by the first fdapde_ctx_create
// of a process; preload_wait(units) waits for the first `units` of them (fdapde_dofs_build, the solver layout, fdapde_topology_build)
void preload_setup_async(int device);
void preload_wait(int units);

// ---- single-launch solver (persist_engine.hip) -----------------------------------------------------------------------------------
// layout of boundary variant v, built on first use (ps.tried / ps.ok tell the outcome)
int build_persist(fdapde_ctx* c, int v);
// scaled values into the layout's blocks (after the scaled full-pattern matrix c->sval is in place)
int fill_persist(fdapde_ctx* c, int v);
int fill_persist_scaled(fdapde_ctx* c, int v, const double* A);   // ... from the unscaled matrix + c->scale (no scaled full-pattern copy needed)
// the whole fused-update CG as one launch; *ran = false: the launch gave up (hand-off timeout) or can never be resident
int run_persist_cols(fdapde_ctx* c, int v, double tol2, int maxit, int n_cols, const double* r_cols, double* x_cols, double* sc_cols, int32_t* ctl_cols,
                     int32_t* h_ctl, double* h_sc, bool* ran, bool bicg = false);   // several right-hand sides side by side in one launch
int run_persist(fdapde_ctx* c, int v, double tol2, int maxit, bool* ran, bool bicg = false);
int run_persist_direct(fdapde_ctx* c, int v, double tol2, int maxit, const double* b_host, double* x_host, bool* ran);   // one column, one workgroup, zero-copy in and out   // bicg: the BiCGStab kernel (plain layouts, <= 8 rows per thread)

// ---- row-distributed multi-GPU form of the single-launch solver (persist_engine.hip); all COLLECTIVE over the context's ranks
int build_rowdist(fdapde_ctx* c, int v);
int rowdist_import_ghosts(fdapde_ctx* c, int v, double* vec);   // owners' values of a per-DOF vector into this rank's ghost columns
int fill_rowdist(fdapde_ctx* c, int v);
int run_rowdist(fdapde_ctx* c, int v, double tol2, int maxit, bool* ran, bool bicg = false);
void release_rowdist(fdapde_ctx* c);

}   // namespace fdapde_engine

#endif
