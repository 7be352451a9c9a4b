// kernels_cols.h -- what the multilevel solvers' kernels share (eng_amg.hip, kernels_block.h, the batched flexible GMRES of eng_pmg.hip): a vector is Q in
// {1, 2, 4, 8} interleaved columns, column q of word i at [i * Q + q] (the layout of kernels_multirhs.h), so the Q values a gathered operand needs are
// contiguous -- for Q >= 2 16-byte aligned and fetched as 16-byte loads.  The columns never mix: a column is computed in the same order at every width, and the
// single-column solve is the Q = 1 instantiation of the same kernels.
#ifndef FDAPDE_KERNELS_COLS_H
#define FDAPDE_KERNELS_COLS_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace fdapde_hip {

constexpr int kAmgColsMax = 8;   // the widest batch

typedef double cols_v2f64_t __attribute__((ext_vector_type(2)));

// the Q columns of one word (Q >= 2: p is 16-byte aligned -- the base is, and Q is even; Q = 1: a plain 8-byte load / store)
template <int Q> __device__ __forceinline__ void ld_cols(const double* p, double (&v)[Q]) {
    static_assert(Q == 1 || Q == 2 || Q == 4 || Q == 8, "1, 2, 4 or 8 columns");
    if constexpr (Q == 1) v[0] = *p;
    else {
#pragma unroll
        for (int q = 0; q < Q; q += 2) {
            const cols_v2f64_t t = *reinterpret_cast<const cols_v2f64_t*>(p + q);
            v[q] = t.x, v[q + 1] = t.y;
        }
    }
}
template <int Q> __device__ __forceinline__ void st_cols(double* p, const double (&v)[Q]) {
    if constexpr (Q == 1) *p = v[0];
    else {
#pragma unroll
        for (int q = 0; q < Q; q += 2) *reinterpret_cast<cols_v2f64_t*>(p + q) = cols_v2f64_t{v[q], v[q + 1]};
    }
}

// a factor per column and the columns a kernel may write (bit q): the columns outside the mask keep their bits
struct ColScal {
    double f[kAmgColsMax];
    unsigned mask;
};

// interleaved <-> column-major n x Q (the coarsest level's vectors: dense_apply takes columns), and one column out of / into an interleaved vector
static __global__ void k_amg_il2cm(int64_t n, int Q, const double* il, double* cm) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * Q) return;
    const int64_t i = e / Q, q = e - i * Q;
    cm[q * n + i] = il[e];
}
static __global__ void k_amg_cm2il(int64_t n, int Q, const double* cm, double* il) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * Q) return;
    const int64_t i = e / Q, q = e - i * Q;
    il[e] = cm[q * n + i];
}
static __global__ void k_amg_col_get(int64_t n, int Q, int q, const double* il, double* col) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) col[i] = il[i * Q + q];
}
static __global__ void k_amg_col_put(int64_t n, int Q, int q, const double* col, double* il) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) il[i * Q + q] = col[i];
}

template <typename F> void by_cols(int Q, F&& f) {
    if (Q == 1) f(std::integral_constant<int, 1>{});
    else if (Q == 2) f(std::integral_constant<int, 2>{});
    else if (Q == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}

// ... and by team width too: f(T, Q) as integral constants.  MINT: the narrowest team the hierarchy uses -- 4 for the scalar levels (eng_amg.hip: 4, 8, 16),
// 8 for the block levels (eng_block_amg.hip: 8, 16)
template <int MINT, typename F> void by_team_cols(int T, int Q, F&& f) {
    auto g = [&](auto t) { by_cols(Q, [&](auto q) { f(t, q); }); };
    if constexpr (MINT <= 4) {
        if (T <= 4) return g(std::integral_constant<int, 4>{});
    }
    if (T <= 8) g(std::integral_constant<int, 8>{});
    else g(std::integral_constant<int, 16>{});
}

}   // namespace fdapde_hip
#endif
