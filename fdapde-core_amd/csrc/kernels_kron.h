// kernels_kron.h -- Kronecker-sum operators on the FEM pattern: A = sum_k T_k (x) S_k, T_k dense q x q (1 <= q <= 64), S_k n x n on the context's pattern
// (the reference's Kronecker(A, B), fdaPDE/linear_algebra/kronecker_product.h:56-80, evaluated into an explicit sparse matrix there; kept as factors here:
// the space-time separable smoothing system and the monolithic parabolic system).  Layout: the context's rowptr / colidx, ONE column index per pattern
// entry, the n_S <= 8 distinct spatial factors interleaved per entry (vals[k n_S + sigma]: an entry's spatial values are one contiguous read), the time
// factors column-major (tm[(sigma q + s) q + r] = T_sigma[r, s]), vectors interleaved per DOF: unknown r of DOF i at z[i q + r] (a gathered DOF is q
// contiguous doubles).  D_i = sum_sigma T_sigma S_sigma[i, i] is the q x q diagonal block of DOF i; its inverse is stored column-major per DOF
// (dinv[(i q + s) q + r] = D_i^-1[r, s]): the point-block Jacobi of kernels_block.h carried to q unknowns per DOF.
// A team of Q lanes (the power of two >= q, 2 <= Q <= 64; q = 1 runs as Q = 2 with one idle lane) owns a spatial row; lane l owns T-row l.  Lanes with
// l >= q and teams past row n issue no global load or store: nothing is read out of bounds and no array needs padding (the rule of k_block_spmv).
// No atomics, every sum in a fixed order spelled out with contraction off: the same bits every run.
#ifndef FDAPDE_KERNELS_KRON_H
#define FDAPDE_KERNELS_KRON_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "kernels_block.h"

namespace fdapde_hip {

constexpr int kKronMaxQ = 64;      // unknowns per DOF
constexpr int kKronMaxTerms = 8;   // terms handed over, hence distinct spatial factors
// f(std::integral_constant<int, Q>) for a team width Q in {2, 4, 8, 16, 32, 64} (the power of two >= q; the data term's: >= max(p, q)): every launch of a
// kernel templated on the team width goes through here
template <typename F> void by_team(int Q, F&& f) {
    switch (Q) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    }
}
// The time factors ride in LDS for the whole workgroup where all of them are at most this many doubles (8 KiB), else the epilogue reads them from global
// memory, where every workgroup shares them in cache.  Measured on the space-time system with four factors (the operator D^-1 A, 502 681 DOFs): the copy
// wins at q = 10 and 16 (400 and 1 024 doubles: 0.502 against 0.530 ms, 0.563 against 0.600) and loses at q = 32 (4 096 doubles, 32 KiB copied by every
// workgroup of 8 rows: 2.06 against 1.66 ms); nothing between was measured, so the limit is the largest size at which the copy was seen to win.
constexpr int kKronLdsFactorDoubles = 1024;

// LDS doubles of k_kron_spmv: 256 n_S for the z_sigma of every team (+ 256 for the row's product where D^-1 is fused in) + n_S q^2 for the time factors
__host__ __device__ inline size_t kron_spmv_lds_doubles(int q, int ns, bool fuse, bool t_in_lds) {
    return (size_t)256 * (size_t)ns + (fuse ? 256 : 0) + (t_in_lds ? (size_t)ns * q * q : 0);
}

// y = A x (FUSE: y = D^-1 A x) on the interleaved layout.  The team walks its row entry by entry: the entry's n_S spatial values and its column index
// (the same address in every lane of the team: one read), then the q contiguous doubles of DOF j; lane l accumulates z_sigma[l] += S_sigma[i,j] x[j q + l].
// Epilogue: the z_sigma go through LDS, lane l forms sum_sigma sum_s T_sigma[l, s] z_sigma[s] for s in band[2 l] .. band[2 l + 1] (the columns outside hold
// exact zeros in every T_sigma: skipping them drops additions of +-0 only), sigma outer, s ascending, one fma each.  A row's q stores are contiguous.
// t_in_lds: the workgroup copies the time factors into LDS first (kKronLdsFactorDoubles; else they are read from tm).
// Algorithmic bytes per launch: 8 n_S nnz + 4 nnz + 4 (n + 1) + 16 q n (+ 8 q^2 n for D^-1 where fused).
template <int Q, bool FUSE>
static __global__ __launch_bounds__(256) void k_kron_spmv(int64_t n, int q, int ns, const int32_t* rowptr, const int32_t* colidx, const double* vals, const double* tm,
                                                          const int32_t* band, const double* dinv, const double* x, double* y, const int32_t* stop, int t_in_lds) {
#pragma clang fp contract(off)
    extern __shared__ double kron_lds[];
    if (stop && __syncthreads_or(*stop != 0)) return;
    constexpr int TEAMS = 256 / Q;
    const int l = threadIdx.x % Q, team = threadIdx.x / Q;
    const int64_t row = (int64_t)blockIdx.x * TEAMS + team;
    const bool lane_ok = l < q, act = lane_ok && row < n;
    double* zs = kron_lds;                                   // [team][sigma][Q]
    double* ys = kron_lds + 256 * ns;                        // [team][Q] (FUSE)
    double* tl = kron_lds + 256 * ns + (FUSE ? 256 : 0);     // [sigma][s][r] (t_in_lds)
    if (t_in_lds)
        for (int t = threadIdx.x; t < ns * q * q; t += 256) tl[t] = tm[t];
    double z[kKronMaxTerms];
#pragma unroll
    for (int s = 0; s < kKronMaxTerms; ++s) z[s] = 0.0;
    if (act) {
        const int rs = rowptr[row], re = rowptr[row + 1];
        int k = rs;
        for (; k + 4 <= re; k += 4) {   // four entries' loads in flight at once (a gather waits for its index); the additions stay in entry order
            int32_t cj[4];
            double xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cj[u] = colidx[k + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[u] = x[(int64_t)cj[u] * q + l];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double* v = vals + (int64_t)(k + u) * ns;
#pragma unroll
                for (int s = 0; s < kKronMaxTerms; ++s)
                    if (s < ns) z[s] = __builtin_fma(v[s], xv[u], z[s]);
            }
        }
        for (; k < re; ++k) {
            const double xv = x[(int64_t)colidx[k] * q + l];
            const double* v = vals + (int64_t)k * ns;
#pragma unroll
            for (int s = 0; s < kKronMaxTerms; ++s)
                if (s < ns) z[s] = __builtin_fma(v[s], xv, z[s]);
        }
    }
    double* zt = zs + (size_t)team * ns * Q;
#pragma unroll
    for (int s = 0; s < kKronMaxTerms; ++s)
        if (s < ns) zt[s * Q + l] = z[s];
    __syncthreads();
    double acc = 0.0;
    if (act) {
        const double* tt = t_in_lds ? tl : tm;
        const int lo = band[2 * l], hi = band[2 * l + 1];
        for (int sg = 0; sg < ns; ++sg) {
#pragma unroll 4
            for (int s = lo; s <= hi; ++s) acc = __builtin_fma(tt[((size_t)sg * q + s) * q + l], zt[sg * Q + s], acc);
        }
    }
    if constexpr (FUSE) {
        ys[team * Q + l] = acc;
        __syncthreads();
        if (act) {
            const double* d = dinv + (size_t)row * q * q;
            double o = 0.0;
#pragma unroll 8
            for (int s = 0; s < q; ++s) o = __builtin_fma(d[(size_t)s * q + l], ys[team * Q + s], o);   // (unrolled: the loads of D^-1 in flight together)
            y[row * q + l] = o;
        }
    } else {
        if (act) y[row * q + l] = acc;
    }
}

// y_i = D_i^-1 x_i for every DOF (y may be x): the batched q x q product of the Krylov stage where it is not fused into the operator kernel, and of its
// right-hand side.  The same sum as the fused epilogue: s ascending, one fma each.  Bytes: 8 q^2 n + 16 q n.
template <int Q>
static __global__ __launch_bounds__(256) void k_kron_dinv_apply(int64_t n, int q, const double* dinv, const double* x, double* y, const int32_t* stop) {
#pragma clang fp contract(off)
    __shared__ double xs[256];
    if (stop && __syncthreads_or(*stop != 0)) return;
    const int l = threadIdx.x % Q, team = threadIdx.x / Q;
    const int64_t row = (int64_t)blockIdx.x * (256 / Q) + team;
    const bool act = l < q && row < n;
    xs[threadIdx.x] = act ? x[row * q + l] : 0.0;
    __syncthreads();
    if (!act) return;
    const double* d = dinv + (size_t)row * q * q;
    double o = 0.0;
#pragma unroll 8
    for (int s = 0; s < q; ++s) o = __builtin_fma(d[(size_t)s * q + l], xs[team * Q + s], o);
    y[row * q + l] = o;
}

// D_i = sum_sigma T_sigma S_sigma[i, i] (sigma ascending) and its inverse, a team per DOF in a workgroup of ONE wavefront (64 / Q teams): in-place
// Gauss-Jordan with partial pivoting in LDS (lane l owns row l, resp. column l where a row is scaled or two rows are swapped; the row exchanges are undone
// as column exchanges in reverse order at the end).  flag raised where a pivot is not above 1e-14 times the block's largest entry, or is not finite, or the
// DOF has no diagonal entry: no point-block Jacobi form (the block's inverse is then left as the identity).  LDS: 64 Q doubles (32 KiB at Q = 64).
// g ([p n], p contiguous per DOF), phi (p x q, column-major): the factored data term's share Phi^T diag(g_i) Phi of D_i (kernels_kron_obs.h k_kron_obs_diag),
// added after the pattern's sum with tau ascending, or NULL.
template <int Q>
static __global__ __launch_bounds__(64) void k_kron_diag_inv(int64_t n, int q, int ns, const int32_t* rowptr, const int32_t* colidx, const double* vals, const double* tm,
                                                             const double* g, const double* phi, int p, double* dinv, int32_t* flag) {
#pragma clang fp contract(off)
    __shared__ double a_all[64 * Q];
    __shared__ int32_t piv_all[64];
    const int l = threadIdx.x % Q, team = threadIdx.x / Q;
    const int64_t i = (int64_t)blockIdx.x * (64 / Q) + team;
    const bool lane_ok = l < q, act = lane_ok && i < n;
    double* a = a_all + (size_t)team * Q * Q;   // a[r + c q], column-major like the time factors
    int32_t* piv = piv_all + team * Q;
    bool bad = false;
    if (act) {
        const int32_t k0 = rowptr[i], k1 = rowptr[i + 1];
        const int32_t d = blk_lower_bound(colidx, k0, k1, (int32_t)i);
        const bool has = d < k1 && colidx[d] == (int32_t)i;
        bad = !has;
        for (int c = 0; c < q; ++c) {
            double v = 0.0;
            if (has)
                for (int sg = 0; sg < ns; ++sg) v = __builtin_fma(tm[((size_t)sg * q + c) * q + l], vals[(int64_t)d * ns + sg], v);
            if (g)
                for (int tau = 0; tau < p; ++tau) v = __builtin_fma(phi[tau + (size_t)l * p] * g[i * p + tau], phi[tau + (size_t)c * p], v);
            a[l + c * q] = v;
        }
    } else if (lane_ok) {
        for (int c = 0; c < q; ++c) a[l + c * q] = l == c ? 1.0 : 0.0;
    }
    __syncthreads();
    double mx = 0.0;
    if (lane_ok)
        for (int t = 0; t < q * q; ++t) {
            const double v = fabs(a[t]);
            mx = (v > mx || !(v == v)) ? v : mx;   // (a NaN sticks)
        }
    const double floor_ = 1e-14 * mx;
    for (int k = 0; k < q; ++k) {
        int p = k;
        double best = -1.0;
        if (lane_ok) {
            for (int r = k; r < q; ++r) {   // (every lane of the team finds the same pivot row: first of the largest)
                const double v = fabs(a[r + k * q]);
                if (v > best) best = v, p = r;
            }
            if (!(best > floor_) || !isfinite(best) || !isfinite(mx)) bad = true;
            if (l == 0) piv[k] = p;
        }
        __syncthreads();
        if (lane_ok && p != k) {   // rows k and p change places: lane l moves column l
            const double u = a[k + l * q];
            a[k + l * q] = a[p + l * q], a[p + l * q] = u;
        }
        __syncthreads();
        const double inv = lane_ok ? 1.0 / a[k + k * q] : 0.0;
        __syncthreads();
        if (lane_ok) a[k + l * q] = l == k ? inv : a[k + l * q] * inv;   // row k scaled: lane l its column l
        __syncthreads();
        if (lane_ok && l != k) {   // row l eliminated
            const double f = a[l + k * q];
            for (int c = 0; c < q; ++c)
                if (c != k) a[l + c * q] = __builtin_fma(-f, a[k + c * q], a[l + c * q]);
            a[l + k * q] = -f * inv;
        }
        __syncthreads();
    }
    for (int k = q - 1; k >= 0; --k) {
        const int p = lane_ok ? piv[k] : k;
        if (lane_ok && p != k) {
            const double u = a[l + k * q];
            a[l + k * q] = a[l + p * q], a[l + p * q] = u;
        }
    }
    __syncthreads();
    if (!act) return;
    if (bad) *flag = 1;
    double* o = dinv + (size_t)i * q * q;
    for (int c = 0; c < q; ++c) o[(size_t)c * q + l] = bad ? (l == c ? 1.0 : 0.0) : a[l + c * q];
}

// the spatial factors as handed over (reference slot order, factor sigma at ext[sigma nnz ...]) -> interleaved per internal slot
static __global__ void k_kron_pack(int64_t nnz, int ns, const int32_t* slot_i2e, const double* ext, double* vals) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nnz * ns) return;
    const int64_t s = t / ns, sg = t - s * ns;
    vals[t] = ext[sg * nnz + slot_i2e[s]];
}

// a column in the reference's Kronecker order (unknown r of DOF e at b_ext[r n + e], reference DOF numbering) -> internal DOF order, unknown r of DOF i at
// z[i si + r sr] (interleaved: si = q, sr = 1; stacked for the dense inverse: si = 1, sr = n); column blockIdx.y
static __global__ void k_kron_stage(int64_t n, int q, const int32_t* i2e, const double* b_ext, double* z, int64_t si, int64_t sr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * q) return;
    const size_t col = blockIdx.y;
    const int64_t r = t / n, i = t - r * n;
    z[col * (size_t)n * q + i * si + r * sr] = b_ext[col * (size_t)n * q + r * n + i2e[i]];
}
// ... and back
static __global__ void k_kron_unstage(int64_t n, int q, const int32_t* i2e, const double* z, double* x_ext, int64_t si, int64_t sr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * q) return;
    const size_t col = blockIdx.y;
    const int64_t r = t / n, i = t - r * n;
    x_ext[col * (size_t)n * q + r * n + i2e[i]] = z[col * (size_t)n * q + i * si + r * sr] + 0.0;
}

// the factors as ONE CSR matrix of q n rows in the stacked order (row r n + i, column s n + j; internal DOF numbering): what the dense inverse is built
// from.  One thread per row; an entry is sum_sigma T_sigma[r, s] S_sigma[i, j], sigma ascending (an explicit zero where every T_sigma[r, s] is zero).
static __global__ void k_kron_expand(int64_t n, int q, int ns, const int32_t* rowptr, const int32_t* colidx, const double* vals, const double* tm, int32_t* rowptr2,
                                     int32_t* colidx2, double* val2) {
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n * q) return;
    const int64_t nnz = rowptr[n];
    if (t == n * q) {
        rowptr2[t] = (int32_t)(nnz * q * q);
        return;
    }
    const int64_t r = t / n, i = t - r * n;
    const int32_t k0 = rowptr[i], len = rowptr[i + 1] - k0;
    int64_t o = r * nnz * q + (int64_t)k0 * q;
    rowptr2[t] = (int32_t)o;
    for (int s = 0; s < q; ++s)
        for (int32_t k = k0; k < k0 + len; ++k, ++o) {
            double v = 0.0;
            for (int sg = 0; sg < ns; ++sg) v = __builtin_fma(tm[((size_t)sg * q + s) * q + r], vals[(int64_t)k * ns + sg], v);
            colidx2[o] = (int32_t)(s * n + colidx[k]), val2[o] = v;
        }
}

// ... and in the interleaved order the vectors use (row i q + r, column j q + s): what the multilevel cycle's coarsest level is inverted from.  The same
// entry sums; a row's columns ascend (entry outer, s inner).
static __global__ void k_kron_expand_il(int64_t n, int q, int ns, const int32_t* rowptr, const int32_t* colidx, const double* vals, const double* tm, int32_t* rowptr2,
                                        int32_t* colidx2, double* val2) {
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n * q) return;
    if (t == n * q) {
        rowptr2[t] = (int32_t)((int64_t)rowptr[n] * q * q);
        return;
    }
    const int64_t i = t / q, r = t - i * q;
    const int32_t k0 = rowptr[i], len = rowptr[i + 1] - k0;
    int64_t o = (int64_t)k0 * q * q + r * (int64_t)len * q;
    rowptr2[t] = (int32_t)o;
    for (int32_t k = k0; k < k0 + len; ++k)
        for (int s = 0; s < q; ++s, ++o) {
            double v = 0.0;
            for (int sg = 0; sg < ns; ++sg) v = __builtin_fma(tm[((size_t)sg * q + s) * q + r], vals[(int64_t)k * ns + sg], v);
            colidx2[o] = (int32_t)((int64_t)colidx[k] * q + s), val2[o] = v;
        }
}

// ---- the multilevel cycle of FDAPDE_SOLVER_KRON_AMG (eng_kron_amg.hip): the cycle kernels of kernels_block.h carried to q unknowns per DOF ------------
// A level is a Kronecker sum on its own pattern (rp / ci / n_S values per entry, the SAME time factors on every level), the inverted q x q diagonal blocks
// (k_kron_diag_inv on the level's arrays) and vectors interleaved per DOF; the smoother is om D^-1.  The access pattern is k_kron_spmv's: a team of Q lanes
// per row, lane l owns T-row l, the epilogue through LDS with the band skip, lanes l >= q and teams past the last row issue no global load or store.  One
// column (the cycle op of the same name at Q = 1 columns).  Contraction off, every sum in a fixed order.

// the scalar strength matrix on the pattern: s_k = -sum_sigma w_sigma |S_sigma[k]| (w_sigma = |T_sigma|_F, sigma ascending; every coupling counts as an
// M-matrix coupling by its magnitude), or -- pick >= 0 -- the spatial factor `pick` as given
static __global__ void k_kamg_strength(int64_t nnz, int ns, const double* vals, const double* w, int pick, double* out) {
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz) return;
    if (pick >= 0) {
        out[k] = vals[k * ns + pick];
        return;
    }
    double s = 0.0;
    for (int sg = 0; sg < ns; ++sg) s = __builtin_fma(w[sg], fabs(vals[k * ns + sg]), s);
    out[k] = -s;
}

// LDS doubles of the cycle kernels: 256 n_S for the z_sigma of every team, 256 for a row's residual, n_S q^2 for the time factors where they are copied
__host__ __device__ inline size_t kamg_lds_doubles(int q, int ns, bool t_in_lds) { return (size_t)256 * (size_t)ns + 256 + (t_in_lds ? (size_t)ns * q * q : 0); }

// the spatial half of a row's product: zt[sigma Q + l] = sum_j S_sigma[row, j] v_j[l], entries ascending, v_j[l] = ld(j) (every lane writes: idle ones zeros)
template <int Q, typename LD>
__device__ __forceinline__ void kamg_row(bool act, int64_t row, int l, int ns, const int32_t* rp, const int32_t* ci, const double* vals, LD&& ld, double* zt) {
#pragma clang fp contract(off)
    double z[kKronMaxTerms];
#pragma unroll
    for (int s = 0; s < kKronMaxTerms; ++s) z[s] = 0.0;
    if (act) {
        const int rs = rp[row], re = rp[row + 1];
        int k = rs;
        for (; k + 4 <= re; k += 4) {   // (k_kron_spmv's: four gathers in flight, the additions in entry order)
            int32_t cj[4];
            double xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cj[u] = ci[k + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[u] = ld((int64_t)cj[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double* v = vals + (int64_t)(k + u) * ns;
#pragma unroll
                for (int s = 0; s < kKronMaxTerms; ++s)
                    if (s < ns) z[s] = __builtin_fma(v[s], xv[u], z[s]);
            }
        }
        for (; k < re; ++k) {
            const double xv = ld((int64_t)ci[k]);
            const double* v = vals + (int64_t)k * ns;
#pragma unroll
            for (int s = 0; s < kKronMaxTerms; ++s)
                if (s < ns) z[s] = __builtin_fma(v[s], xv, z[s]);
        }
    }
#pragma unroll
    for (int s = 0; s < kKronMaxTerms; ++s)
        if (s < ns) zt[s * Q + l] = z[s];
}
// ... and the time half (after a barrier): sum_sigma sum_s T_sigma[l, s] z_sigma[s], sigma outer, s ascending within the band, one fma each
template <int Q> __device__ __forceinline__ double kamg_time(int l, int q, int ns, const double* tt, const int32_t* band, const double* zt) {
#pragma clang fp contract(off)
    const int lo = band[2 * l], hi = band[2 * l + 1];
    double acc = 0.0;
    for (int sg = 0; sg < ns; ++sg) {
#pragma unroll 4
        for (int s = lo; s <= hi; ++s) acc = __builtin_fma(tt[((size_t)sg * q + s) * q + l], zt[sg * Q + s], acc);
    }
    return acc;
}

// pre-smoothing from zero: zt_i = om D_i^-1 r_i (k_kron_dinv_apply's sum, scaled)
template <int Q>
static __global__ __launch_bounds__(256) void k_kamg_smooth(int64_t n, int q, const double* dinv, double om, const double* r, double* zt) {
#pragma clang fp contract(off)
    __shared__ double xs[256];
    const int l = threadIdx.x % Q, team = threadIdx.x / Q;
    const int64_t row = (int64_t)blockIdx.x * (256 / Q) + team;
    const bool act = l < q && row < n;
    xs[threadIdx.x] = act ? r[row * q + l] : 0.0;
    __syncthreads();
    if (!act) return;
    const double* d = dinv + (size_t)row * q * q;
    double o = 0.0;
#pragma unroll 8
    for (int s = 0; s < q; ++s) o = __builtin_fma(d[(size_t)s * q + l], xs[team * Q + s], o);
    zt[row * q + l] = om * o;
}

// the restricted residual of the smoothed zt, a team per aggregate: rc_a = sum over its members i, ascending, of (r_i - (A zt)_i); unknown l of aggregate a at
// rc[(a q + l) rs] (one column: interleaved and column-major coincide).  The member loop runs to the workgroup's longest aggregate (a barrier per member row).
template <int Q>
static __global__ __launch_bounds__(256) void k_kamg_pre_restrict(int64_t nc, int q, int ns, const int32_t* mptr, const int32_t* midx, const int32_t* rp, const int32_t* ci,
                                                                  const double* vals, const double* tm, const int32_t* band, const double* r, const double* zt,
                                                                  double* rc, int64_t rs, int t_in_lds) {
#pragma clang fp contract(off)
    extern __shared__ double kron_lds[];
    constexpr int TEAMS = 256 / Q;
    const int l = threadIdx.x % Q, team = threadIdx.x / Q;
    const int64_t ag = (int64_t)blockIdx.x * TEAMS + team;
    const bool lane_ok = l < q, ag_ok = lane_ok && ag < nc;
    double* zl = kron_lds + (size_t)team * ns * Q;
    double* tl = kron_lds + 256 * ns + 256;
    if (t_in_lds)
        for (int t = threadIdx.x; t < ns * q * q; t += 256) tl[t] = tm[t];
    const double* tt = t_in_lds ? tl : tm;
    const int32_t m1 = ag_ok ? mptr[ag + 1] : 0;
    int32_t m = ag_ok ? mptr[ag] : 0;
    double c = 0.0;
    for (; __syncthreads_or(m < m1); ++m) {
        const bool act = m < m1;   // (ag_ok: else m1 = 0)
        const int64_t i = act ? midx[m] : 0;
        kamg_row<Q>(act, i, l, ns, rp, ci, vals, [&](int64_t j) { return zt[j * q + l]; }, zl);
        __syncthreads();
        if (act) c += r[i * q + l] - kamg_time<Q>(l, q, ns, tt, band, zl);
    }
    if (ag_ok) rc[(ag * q + l) * rs] = c;
}

// out_i = z_i + om D_i^-1 (r_i - (A z)_i) with z = zt + P e: prolongation (every row has an aggregate), residual and post-smoothing in one pass
template <int Q>
static __global__ __launch_bounds__(256) void k_kamg_post(int64_t n, int q, int ns, const int32_t* rp, const int32_t* ci, const double* vals, const double* tm,
                                                          const int32_t* band, const double* dinv, double om, const int32_t* agg, const double* e, const double* r,
                                                          const double* zt, double* out, int t_in_lds) {
#pragma clang fp contract(off)
    extern __shared__ double kron_lds[];
    constexpr int TEAMS = 256 / Q;
    const int l = threadIdx.x % Q, team = threadIdx.x / Q;
    const int64_t row = (int64_t)blockIdx.x * TEAMS + team;
    const bool act = l < q && row < n;
    double* zl = kron_lds + (size_t)team * ns * Q;
    double* ys = kron_lds + 256 * ns;
    double* tl = ys + 256;
    if (t_in_lds)
        for (int t = threadIdx.x; t < ns * q * q; t += 256) tl[t] = tm[t];
    kamg_row<Q>(act, row, l, ns, rp, ci, vals, [&](int64_t j) { return zt[j * q + l] + e[(int64_t)agg[j] * q + l]; }, zl);
    __syncthreads();
    double zi = 0.0, d = 0.0;
    if (act) {
        zi = zt[row * q + l] + e[(int64_t)agg[row] * q + l];
        d = r[row * q + l] - kamg_time<Q>(l, q, ns, t_in_lds ? tl : tm, band, zl);
    }
    ys[team * Q + l] = d;
    __syncthreads();
    if (!act) return;
    const double* di = dinv + (size_t)row * q * q;
    double o = 0.0;
#pragma unroll 8
    for (int s = 0; s < q; ++s) o = __builtin_fma(di[(size_t)s * q + l], ys[team * Q + s], o);
    out[row * q + l] = __builtin_fma(om, o, zi);
}

// y = A x and the three dot products p_d . q_d of a GCR step (any of the vectors may be y itself; p2 may be NULL: a zero) as per-workgroup partials
// part[d gridDim.x + block]: a fixed grid, the workgroup strides over the rows, a lane sums its own unknown's products, then the wavefronts' sums in order
template <int Q>
static __global__ __launch_bounds__(256) void k_kamg_spmv_dots(int64_t n, int q, int ns, const int32_t* rp, const int32_t* ci, const double* vals, const double* tm,
                                                               const int32_t* band, const double* x, double* y, const double* p0, const double* q0, const double* p1,
                                                               const double* q1, const double* p2, const double* q2, double* part, int t_in_lds) {
#pragma clang fp contract(off)
    extern __shared__ double kron_lds[];
    __shared__ double red[3][4];
    constexpr int TEAMS = 256 / Q;
    const int l = threadIdx.x % Q, team = threadIdx.x / Q;
    double* zl = kron_lds + (size_t)team * ns * Q;
    double* tl = kron_lds + 256 * ns + 256;
    if (t_in_lds)
        for (int t = threadIdx.x; t < ns * q * q; t += 256) tl[t] = tm[t];
    const double* tt = t_in_lds ? tl : tm;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * TEAMS; base < n; base += (int64_t)gridDim.x * TEAMS) {   // (the same trips for every lane of the workgroup)
        const int64_t row = base + team;
        const bool act = l < q && row < n;
        kamg_row<Q>(act, row, l, ns, rp, ci, vals, [&](int64_t j) { return x[j * q + l]; }, zl);
        __syncthreads();
        if (act) {
            const int64_t w = row * q + l;
            const double yi = kamg_time<Q>(l, q, ns, tt, band, zl);
            y[w] = yi;
            d0 += (p0 == y ? yi : p0[w]) * (q0 == y ? yi : q0[w]);
            d1 += (p1 == y ? yi : p1[w]) * (q1 == y ? yi : q1[w]);
            if (p2) d2 += (p2 == y ? yi : p2[w]) * (q2 == y ? yi : q2[w]);
        }
        __syncthreads();
    }
    const int wv = threadIdx.x >> 6;
    const double t0 = wave_sum(d0), t1 = wave_sum(d1), t2 = wave_sum(d2);
    if ((threadIdx.x & 63) == 0) red[0][wv] = t0, red[1][wv] = t1, red[2][wv] = t2;
    __syncthreads();
    if (threadIdx.x < 3) part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

}  // namespace fdapde_hip
#endif
