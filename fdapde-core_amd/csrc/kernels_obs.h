// kernels_obs.h -- the factored data term of the 2 x 2 block handle: A + scale [Psi^T W Psi, 0; 0, 0] with Psi (n_obs x n, CSR) kept as it is, so that an
// areal sampling design (fdaPDE basis/lagrangian_basis.h:203-283: a row of Psi spans every DOF of its region, and Psi^T Psi is far off the FEM pattern) can use
// the handle.  y += scale Psi^T (W (Psi x_1)) is two sparse rectangular products, linear in nnz(Psi):
//   k_obs_gather   t = W Psi x_1        a team of T lanes per observation (a row of Psi)
//   k_obs_scatter  y_i += D_i^-1 [s; 0], s = scale (Psi^T t)_i        a team per DOF over its row of Psi^T (a second CSR, observations ascending)
//   k_obs_diag     g_i = scale sum_k w_k Psi[k, i]^2                 the term's share of the diagonal block D_i (set-up)
// Layout: the columns of Psi are internal DOF ids, vectors are interleaved per DOF (kernels_block.h): the first unknown of DOF i sits at 2 i.  The access
// pattern is k_block_spmv's: a lane takes entries rs + l, rs + l + T, ..., a lane past the row's end issues no load (no array needs padding), the in-team sum
// is the fixed butterfly of team_sum<T>.  No atomics: the same bits every run.  T = 8 for short rows (pointwise Psi: 3 - 10 entries), T = 64 for long ones
// (areal Psi: hundreds to 10^5); the rule is host_obs.h's obs_team_width.  Every kernel reads the stop flag first, as every kernel of a GMRES cycle does.
// Algorithmic bytes of the term per operator application (every array once per pass), nz = nnz(Psi):
//   gather   12 nz + 4 (n_obs + 1) + 8 n_obs (w) + 8 n (x_1) + 8 n_obs (t written)
//   scatter  12 nz + 4 (n + 1) + 8 n_obs (t) + 16 n (the first column of D^-1) + 32 n (y read and written)
// The multilevel cycle of FDAPDE_SOLVER_BLOCK_AMG with the term carried (knob block_amg_obs, eng_block_amg.hip) keeps one Psi_l per level, Psi_{l+1} = Psi_l P_s
// (host_obs.h obs_coarsen), and two more forms of the products, one column each:
//   k_obs_gather_acc     t += W Psi x_1      12 nz + 4 (n_obs + 1) + 8 n_obs (w) + 8 n (x_1) + 16 n_obs (t read and written)
//   k_obs_scatter_store  s = scale Psi^T t   12 nz + 4 (n + 1) + 8 n_obs (t) + 8 n (s written; an empty row stores 0)
#ifndef FDAPDE_KERNELS_OBS_H
#define FDAPDE_KERNELS_OBS_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_reduce.h"

namespace fdapde_hip {

template <int T>
static __global__ __launch_bounds__(256) void k_obs_gather(int64_t n_obs, const int32_t* rp, const int32_t* ci, const double* v, const double* w, const double* x,
                                                           double* t, const int32_t* stop) {
    if (stop && __syncthreads_or(*stop != 0)) return;
    constexpr int TEAMS = 256 / T;
    const int l = threadIdx.x % T;
    const int64_t row = (int64_t)blockIdx.x * TEAMS + threadIdx.x / T;
    const bool row_ok = row < n_obs;
    const int64_t rc = row_ok ? row : n_obs - 1;   // (lanes of a row past the end go through the motions on the last row and do not store)
    const int rs = rp[rc], re = rp[rc + 1];
    double a = 0.0;
    for (int k = rs + l; k < re; k += T) a += v[k] * x[2 * (int64_t)ci[k]];
    a = team_sum<T>(a);
    if (l == 0 && row_ok) t[row] = w[row] * a;
}

// dinv: the inverted diagonal blocks [4 n] where the kernel serves the Krylov stage's operator D^-1 A -- (d00, d10) = the first column of D_i^-1 -- or NULL
// for the unscaled product ((1, 0)).  A DOF in no observation (an empty row of Psi^T) leaves y_i as it is.
template <int T>
static __global__ __launch_bounds__(256) void k_obs_scatter(int64_t n, const int32_t* trp, const int32_t* tci, const double* tv, const double* t, double scale,
                                                            const double* dinv, double* y, const int32_t* stop) {
    if (stop && __syncthreads_or(*stop != 0)) return;
    constexpr int TEAMS = 256 / T;
    const int l = threadIdx.x % T;
    const int64_t row = (int64_t)blockIdx.x * TEAMS + threadIdx.x / T;
    const bool row_ok = row < n;
    const int64_t rc = row_ok ? row : n - 1;
    const int rs = trp[rc], re = trp[rc + 1];
    double a = 0.0;
    for (int k = rs + l; k < re; k += T) a += tv[k] * t[tci[k]];
    a = team_sum<T>(a);
    if (l == 0 && row_ok && re > rs) {
        const double s = scale * a;
        if (dinv) {
            const double d00 = dinv[4 * row], d10 = dinv[4 * row + 2];
            y[2 * row] += d00 * s, y[2 * row + 1] += d10 * s;
        } else {
            y[2 * row] += s;
        }
    }
}

// t_k += w_k (Psi x_1)_k: the second half of W Psi (zt + P e) = W Psi_l zt + W Psi_{l+1} e in the cycle's post-smoothing, over the next level's shorter rows
template <int T>
static __global__ __launch_bounds__(256) void k_obs_gather_acc(int64_t n_obs, const int32_t* rp, const int32_t* ci, const double* v, const double* w, const double* x,
                                                               double* t) {
    constexpr int TEAMS = 256 / T;
    const int l = threadIdx.x % T;
    const int64_t row = (int64_t)blockIdx.x * TEAMS + threadIdx.x / T;
    const bool row_ok = row < n_obs;
    const int64_t rc = row_ok ? row : n_obs - 1;
    const int rs = rp[rc], re = rp[rc + 1];
    double a = 0.0;
    for (int k = rs + l; k < re; k += T) a += v[k] * x[2 * (int64_t)ci[k]];
    a = team_sum<T>(a);
    if (l == 0 && row_ok) t[row] += w[row] * a;
}

// s_i = scale (Psi^T t)_i stored (not added): the term's share of a coarse level's y = A x, which k_bamg_spmv_dots adds before its dot products
template <int T>
static __global__ __launch_bounds__(256) void k_obs_scatter_store(int64_t n, const int32_t* trp, const int32_t* tci, const double* tv, const double* t, double scale,
                                                                  double* s) {
    constexpr int TEAMS = 256 / T;
    const int l = threadIdx.x % T;
    const int64_t row = (int64_t)blockIdx.x * TEAMS + threadIdx.x / T;
    const bool row_ok = row < n;
    const int64_t rc = row_ok ? row : n - 1;
    const int rs = trp[rc], re = trp[rc + 1];
    double a = 0.0;
    for (int k = rs + l; k < re; k += T) a += tv[k] * t[tci[k]];
    a = team_sum<T>(a);
    if (l == 0 && row_ok) s[row] = re > rs ? scale * a : 0.0;
}

template <int T>
static __global__ __launch_bounds__(256) void k_obs_diag(int64_t n, const int32_t* trp, const int32_t* tci, const double* tv, const double* w, double scale,
                                                         double* g, const int32_t* stop) {
    if (stop && __syncthreads_or(*stop != 0)) return;
    constexpr int TEAMS = 256 / T;
    const int l = threadIdx.x % T;
    const int64_t row = (int64_t)blockIdx.x * TEAMS + threadIdx.x / T;
    const bool row_ok = row < n;
    const int64_t rc = row_ok ? row : n - 1;
    const int rs = trp[rc], re = trp[rc + 1];
    double a = 0.0;
    for (int k = rs + l; k < re; k += T) {
        const double p = tv[k];
        a += w[tci[k]] * (p * p);
    }
    a = team_sum<T>(a);
    if (l == 0 && row_ok) g[row] = scale * a;
}

}  // namespace fdapde_hip
#endif
