// kernels_kron_obs.h -- the factored data term of the Kronecker-sum handle: A + scale (Phi (x) Psi)^T W (Phi (x) Psi) with Phi (p x q, dense, column-major,
// 1 <= p <= 64), Psi (n_obs x n, CSR, rows of any length) and W = diag(w) over (instant, location) pairs kept as they are: a space-time model with areal
// sampling (Psi^T Psi far off the FEM pattern), with missing observations (W no Kronecker product) or with observation instants that are not the time
// nodes (Phi) -- kernels_obs.h carried to q unknowns per DOF, with the access pattern of k_kron_spmv.  Per application two rectangular sparse products with
// q-vectors per DOF and two small dense products per row:
//   k_kron_obs_gather   t = W (Phi (x) Psi) x                      a team per observation (a row of Psi)
//   k_kron_obs_scatter  y_i += [D_i^-1] scale ((Phi (x) Psi)^T t)_i   a team per DOF over its row of Psi^T (a second CSR, observations ascending)
//   k_kron_obs_diag     g_i[tau] = scale sum_k w[tau, k] Psi[k, i]^2  the term's share Phi^T diag(g_i) Phi of the diagonal block D_i (set-up)
// Layout: the columns of Psi are internal DOF ids, vectors are interleaved per DOF (kernels_kron.h: unknown l of DOF j at x[j q + l]), the weights and the
// intermediate are interleaved per observation (w[k p + tau], t[k p + tau]: a row's p values are contiguous), Phi[tau, s] at phi[tau + s p].
// Team width QP: the power of two >= max(p, q), 2 <= QP <= 64.  Lanes past p or q and teams past the last row issue no global load or store; nothing is
// padded.  Two forms per kernel, chosen per matrix (host_kron_obs.h kron_obs_form):
//   narrow  one team per row, 256 / QP rows per workgroup; the team walks its row entry by entry
//   wide    one workgroup per row: its G = 256 / QP sub-teams take entries g, g + G, g + 2 G, ..., the partial vectors go to LDS and sub-team 0 adds the
//           G partials with g ascending -- a fixed order: the same bits every run; the two forms differ from each other in their last bits
// Phi is read from global memory, where every workgroup shares it in cache (at most 4 096 doubles); a copy in LDS was not measured.  No atomics, every sum in
// a fixed order with contraction off.  Every kernel reads the stop flag first, as every kernel of a GMRES cycle does.
// Algorithmic bytes per application (every array once per pass), nz = nnz(Psi), m = n_obs:
//   gather   12 nz + 4 (m + 1) + 8 q n + 16 p m
//   scatter  12 nz + 4 (n + 1) + 8 p m + 16 q n (+ 8 q^2 n for D^-1 in the Krylov stage)
#ifndef FDAPDE_KERNELS_KRON_OBS_H
#define FDAPDE_KERNELS_KRON_OBS_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fdapde_hip {

// a row's sum of term(e, .) over its entries rs <= e < re, per lane: the team's own walk (narrow), or the sub-teams' strided walks added by sub-team 0 with
// g ascending (wide: the value is sub-team 0's, every thread of the workgroup has to call).  term(e, a) gives a + the entry's product.  part: 256 doubles.
template <int QP, bool WIDE, typename F> __device__ __forceinline__ double kron_obs_row(bool lane_ok, int rs, int re, F&& term, double* part) {
#pragma clang fp contract(off)
    double a = 0.0;
    if constexpr (!WIDE) {
        if (lane_ok) {
#pragma unroll 4
            for (int e = rs; e < re; ++e) a = term(e, a);
        }
        return a;
    } else {
        constexpr int G = 256 / QP;
        const int l = threadIdx.x % QP, g = threadIdx.x / QP;
        if (lane_ok) {
#pragma unroll 4
            for (int e = rs + g; e < re; e += G) a = term(e, a);
        }
        part[g * QP + l] = a;
        __syncthreads();
        double s = 0.0;
        if (g == 0)
            for (int h = 0; h < G; ++h) s += part[h * QP + l];
        return s;
    }
}

template <int QP, bool WIDE>
static __global__ __launch_bounds__(256) void k_kron_obs_gather(int64_t m, int q, int p, const int32_t* rp, const int32_t* ci, const double* v, const double* phi,
                                                                const double* w, const double* x, double* t, const int32_t* stop) {
#pragma clang fp contract(off)
    __shared__ double part[256];
    __shared__ double us[256];
    if (stop && __syncthreads_or(*stop != 0)) return;
    const int l = threadIdx.x % QP, sub = threadIdx.x / QP;
    const int64_t row = WIDE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (256 / QP) + sub;
    const int tm = WIDE ? 0 : sub;
    const bool head = !WIDE || sub == 0, row_ok = row < m;
    int rs = 0, re = 0;
    if (row_ok) rs = rp[row], re = rp[row + 1];
    const double u = kron_obs_row<QP, WIDE>(row_ok && l < q, rs, re, [&](int e, double a) { return __builtin_fma(v[e], x[(int64_t)ci[e] * q + l], a); }, part);
    if (head) us[tm * QP + l] = u;   // (lanes past q hold zeros)
    __syncthreads();
    if (!(head && row_ok && l < p)) return;
    double a = 0.0;
#pragma unroll 4
    for (int s = 0; s < q; ++s) a = __builtin_fma(phi[l + (size_t)s * p], us[tm * QP + s], a);
    t[row * p + l] = w[row * p + l] * a;
}

// dinv: the inverted diagonal blocks [q q n] where the kernel serves the Krylov stage's operator D^-1 A (the column walk of k_kron_dinv_apply), or NULL for
// the unscaled product.  A DOF in no observation (an empty row of Psi^T) leaves y_i as it is.
template <int QP, bool WIDE>
static __global__ __launch_bounds__(256) void k_kron_obs_scatter(int64_t n, int q, int p, const int32_t* trp, const int32_t* tci, const double* tv, const double* phi,
                                                                 const double* t, double scale, const double* dinv, double* y, const int32_t* stop) {
#pragma clang fp contract(off)
    __shared__ double part[256];
    __shared__ double ss[256];
    __shared__ double zs[256];
    if (stop && __syncthreads_or(*stop != 0)) return;
    const int l = threadIdx.x % QP, sub = threadIdx.x / QP;
    const int64_t row = WIDE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (256 / QP) + sub;
    const int tm = WIDE ? 0 : sub;
    const bool head = !WIDE || sub == 0, row_ok = row < n;
    int rs = 0, re = 0;
    if (row_ok) rs = trp[row], re = trp[row + 1];
    const double s = kron_obs_row<QP, WIDE>(row_ok && l < p, rs, re, [&](int e, double a) { return __builtin_fma(tv[e], t[(int64_t)tci[e] * p + l], a); }, part);
    if (head) ss[tm * QP + l] = s;
    __syncthreads();
    const bool out = head && row_ok && l < q && re > rs;
    double z = 0.0;
    if (out) {
#pragma unroll 4
        for (int tau = 0; tau < p; ++tau) z = __builtin_fma(phi[tau + (size_t)l * p], ss[tm * QP + tau], z);
        z = scale * z;
    }
    if (dinv) {   // (the same for every thread)
        if (head) zs[tm * QP + l] = z;
        __syncthreads();
        if (!out) return;
        const double* d = dinv + (size_t)row * q * q;
        double o = 0.0;
#pragma unroll 8
        for (int c = 0; c < q; ++c) o = __builtin_fma(d[(size_t)c * q + l], zs[tm * QP + c], o);
        y[row * q + l] += o;
    } else if (out) {
        y[row * q + l] += z;
    }
}

// g[i p + tau] = scale sum_k w[k p + tau] Psi[k, i]^2, observations ascending (k_kron_diag_inv adds Phi^T diag(g_i) Phi to D_i)
template <int QP, bool WIDE>
static __global__ __launch_bounds__(256) void k_kron_obs_diag(int64_t n, int p, const int32_t* trp, const int32_t* tci, const double* tv, const double* w, double scale,
                                                              double* g, const int32_t* stop) {
#pragma clang fp contract(off)
    __shared__ double part[256];
    if (stop && __syncthreads_or(*stop != 0)) return;
    const int l = threadIdx.x % QP, sub = threadIdx.x / QP;
    const int64_t row = WIDE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (256 / QP) + sub;
    const bool head = !WIDE || sub == 0, row_ok = row < n;
    int rs = 0, re = 0;
    if (row_ok) rs = trp[row], re = trp[row + 1];
    const double s = kron_obs_row<QP, WIDE>(row_ok && l < p, rs, re, [&](int e, double a) { return __builtin_fma(w[(int64_t)tci[e] * p + l], tv[e] * tv[e], a); }, part);
    if (head && row_ok && l < p) g[row * p + l] = scale * s;
}

}   // namespace fdapde_hip
#endif
