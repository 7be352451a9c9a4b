// kernels_block.h -- 2 x 2 block systems on the FEM pattern (fdaPDE/linear_algebra/sparse_block_matrix.h:29-128: the smoothing system
//     [ -Psi^T W Psi   lambda R1^T ] [f]   [ -Psi^T W z ]
//     [  lambda R1     lambda R0   ] [g] = [  lambda u   ]
// every block of which lies on the pattern of stiff() / mass()).  Layout: block CSR in the solver's internal DOF order -- the context's
// rowptr / colidx, ONE column index per pattern entry, four contiguous doubles [a11 a12 a21 a22] per entry (32-byte aligned) -- and vectors
// interleaved per DOF: z[2 i] = f_i, z[2 i + 1] = g_i.  The Krylov stage works on D^-1 A, D = the 2 x 2 diagonal block of every DOF (left
// block-Jacobi, folded into the values once per fdapde_block_compute); the Gram matrix Psi^T W Psi is accumulated with fp64 atomics.
#ifndef FDAPDE_KERNELS_BLOCK_H
#define FDAPDE_KERNELS_BLOCK_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_cols.h"
#include "kernels_reduce.h"

namespace fdapde_hip {

typedef double blk_v2f64_t __attribute__((ext_vector_type(2)));

constexpr int kBlockTeam = 8;   // lanes per block row of k_block_spmv: one pass covers 8 entries (2-D P1 rows: 7, 3-D P1: ~15, P2: 20 - 30)

__device__ __forceinline__ int32_t blk_lower_bound(const int32_t* a, int32_t lo, int32_t hi, int32_t x) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// y = A x on the interleaved layout.  T lanes share a block row; a lane takes whole entries k = rs + l, rs + l + T, ...: the 32 bytes of values
// as two 16-byte loads, one column index, one 16-byte gather of the x pair.  Lanes past the row's end issue no load at all (nothing is read
// out of bounds: the arrays need no padding).  The in-team sum is a fixed butterfly: the same bits every run.  One 16-byte store per row.
// Algorithmic bytes per launch: 36 nnz + 4 (n + 1) + 32 n.
template <int T>
static __global__ __launch_bounds__(256) void k_block_spmv(int64_t n, const int32_t* rowptr, const int32_t* colidx, const double* vals, const double* x, double* y,
                                                           const int32_t* stop) {
    if (stop && __syncthreads_or(*stop != 0)) return;
    constexpr int TEAMS = 256 / T;
    const int l = threadIdx.x % T;
    const int64_t row = (int64_t)blockIdx.x * TEAMS + threadIdx.x / T;
    const bool row_ok = row < n;
    const int64_t rc = row_ok ? row : n - 1;   // (lanes of a row past the end go through the motions on the last row and do not store)
    const int rs = rowptr[rc], re = rowptr[rc + 1];
    double a0 = 0.0, a1 = 0.0;
    for (int k = rs + l; k < re; k += T) {
        const blk_v2f64_t* v = reinterpret_cast<const blk_v2f64_t*>(vals + 4 * (int64_t)k);
        const blk_v2f64_t top = v[0], bot = v[1];
        const int col = colidx[k];
        const blk_v2f64_t xp = *reinterpret_cast<const blk_v2f64_t*>(x + 2 * (int64_t)col);
        a0 += top.x * xp.x + top.y * xp.y;
        a1 += bot.x * xp.x + bot.y * xp.y;
    }
    a0 = team_sum<T>(a0), a1 = team_sum<T>(a1);
    if (l == 0 && row_ok) *reinterpret_cast<blk_v2f64_t*>(y + 2 * row) = blk_v2f64_t{a0, a1};
}

// the four blocks as handed over (reference slot order, block q at ext[q * nnz ...], a NULL block as zeros) -> [a11 a12 a21 a22] per internal slot
static __global__ void k_block_pack(int64_t nnz, const int32_t* slot_i2e, const double* ext, double* raw) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nnz) return;
    const int64_t e = slot_i2e[s];
    blk_v2f64_t* o = reinterpret_cast<blk_v2f64_t*>(raw + 4 * s);
    o[0] = blk_v2f64_t{ext[e], ext[nnz + e]};
    o[1] = blk_v2f64_t{ext[2 * nnz + e], ext[3 * nnz + e]};
}

// D_i^-1 of every DOF's diagonal block; flag raised where |det| <= 1e-14 max|entry|^2 (or the block is missing / not finite): no block-Jacobi form.
// add11: a per-DOF addend to the (1,1) entry of D_i (the factored data term's share, kernels_obs.h k_obs_diag), or NULL
static __global__ void k_block_diag_inv(int64_t n, const int32_t* rowptr, const int32_t* colidx, const double* raw, const double* add11, double* dinv, int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t k0 = rowptr[i], k1 = rowptr[i + 1];
    const int32_t d = blk_lower_bound(colidx, k0, k1, (int32_t)i);
    double a = 0, b = 0, cc = 0, e = 0;
    if (d < k1 && colidx[d] == (int32_t)i) a = raw[4 * (int64_t)d], b = raw[4 * (int64_t)d + 1], cc = raw[4 * (int64_t)d + 2], e = raw[4 * (int64_t)d + 3];
    if (add11) a += add11[i];
    const double det = a * e - b * cc;
    const double mx = fmax(fmax(fabs(a), fabs(b)), fmax(fabs(cc), fabs(e)));
    double* o = dinv + 4 * i;
    if (!(fabs(det) > 1e-14 * mx * mx) || !isfinite(det)) {
        *flag = 1;
        o[0] = 1.0, o[1] = 0.0, o[2] = 0.0, o[3] = 1.0;
        return;
    }
    const double inv = 1.0 / det;
    o[0] = e * inv, o[1] = -b * inv, o[2] = -cc * inv, o[3] = a * inv;
}

// scaled = D_i^-1 times block row i (T lanes per row, as the product walks it)
static __global__ void k_block_scale(int64_t n, const int32_t* rowptr, const double* raw, const double* dinv, double* scaled) {
    constexpr int T = kBlockTeam;
    const int l = threadIdx.x % T;
    const int64_t row = (int64_t)blockIdx.x * (256 / T) + threadIdx.x / T;
    if (row >= n) return;
    const double d0 = dinv[4 * row], d1 = dinv[4 * row + 1], d2 = dinv[4 * row + 2], d3 = dinv[4 * row + 3];
    for (int k = rowptr[row] + l; k < rowptr[row + 1]; k += T) {
        const double a = raw[4 * (int64_t)k], b = raw[4 * (int64_t)k + 1], cc = raw[4 * (int64_t)k + 2], e = raw[4 * (int64_t)k + 3];
        double* o = scaled + 4 * (int64_t)k;
        o[0] = d0 * a + d1 * cc, o[1] = d0 * b + d1 * e, o[2] = d2 * a + d3 * cc, o[3] = d2 * b + d3 * e;
    }
}

// a stacked column in the reference numbering (rows 0 .. n-1 the first block row, n .. 2n-1 the second) -> interleaved internal order, times
// D^-1 where dinv is given (the Krylov stage's right-hand side); column blockIdx.y of nc
static __global__ void k_block_stage(int64_t n, const int32_t* i2e, const double* b_ext, const double* dinv, double* z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t col = blockIdx.y;
    const int64_t e = i2e[i];
    const double f = b_ext[col * 2 * (size_t)n + e], g = b_ext[col * 2 * (size_t)n + n + e];
    double* o = z + col * 2 * (size_t)n + 2 * i;
    if (dinv) o[0] = dinv[4 * i] * f + dinv[4 * i + 1] * g, o[1] = dinv[4 * i + 2] * f + dinv[4 * i + 3] * g;
    else o[0] = f, o[1] = g;
}
// ... and back
static __global__ void k_block_unstage(int64_t n, const int32_t* i2e, const double* z, double* x_ext) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t col = blockIdx.y;
    const int64_t e = i2e[i];
    const double* s = z + col * 2 * (size_t)n + 2 * i;
    x_ext[col * 2 * (size_t)n + e] = s[0] + 0.0, x_ext[col * 2 * (size_t)n + n + e] = s[1] + 0.0;
}

// start of a Krylov column: x = 0, r = bt, |bt|^2 partials ...
static __global__ __launch_bounds__(256) void k_block_krylov_init(int64_t n2, const double* bt, double* x, double* r, double* part) {
    __shared__ double red[4];
    double a = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = bt[i];
        x[i] = 0.0, r[i] = v, a += isfinite(v) ? v * v : 1e300;
    }
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// ... sc[0] = |b|^2, sc[3] = sc[21] = |r|^2 (the slots the GMRES kernels read), ctl cleared; a zero right-hand side is solved by x = 0
static __global__ void k_block_krylov_init_fin(const double* part, int np, double* sc, int32_t* ctl) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0;
    for (int i = 0; i < np; ++i) s += part[i];
    sc[0] = s, sc[3] = s, sc[21] = s;
    for (int k = 0; k < 8; ++k) ctl[k] = 0;
    if (!(s > 0.0)) ctl[0] = 1;
}

// the four blocks as ONE CSR matrix of 2 n rows in the interleaved order (row 2 i + p, column 2 j + q): what the dense inverse is built from
static __global__ void k_block_expand(int64_t n, const int32_t* rowptr, const int32_t* colidx, const double* raw, int32_t* rowptr2, int32_t* colidx2, double* val2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        rowptr2[2 * n] = 4 * rowptr[n];
        return;
    }
    const int32_t k0 = rowptr[i], len = rowptr[i + 1] - k0;
    const int32_t r0 = 4 * k0, r1 = 4 * k0 + 2 * len;
    rowptr2[2 * i] = r0, rowptr2[2 * i + 1] = r1;
    for (int32_t t = 0; t < len; ++t) {
        const int64_t k = k0 + t;
        const int32_t j = colidx[k];
        colidx2[r0 + 2 * t] = 2 * j, colidx2[r0 + 2 * t + 1] = 2 * j + 1;
        colidx2[r1 + 2 * t] = 2 * j, colidx2[r1 + 2 * t + 1] = 2 * j + 1;
        val2[r0 + 2 * t] = raw[4 * k], val2[r0 + 2 * t + 1] = raw[4 * k + 1];
        val2[r1 + 2 * t] = raw[4 * k + 2], val2[r1 + 2 * t + 1] = raw[4 * k + 3];
    }
}

// ---- the multilevel cycle of FDAPDE_SOLVER_BLOCK_AMG (eng_block_amg.hip): block forms of eng_amg.hip's cycle kernels ------------------------------
// A level is a block CSR matrix (rp / ci / four doubles per entry), the inverted 2 x 2 diagonal blocks dinv (four doubles per row) and vectors
// interleaved per row; the smoother is om D^-1.  The access pattern is k_block_spmv's: a team of T lanes per row (or aggregate), a lane takes whole
// entries (two 16-byte loads, one index, 16-byte gathers), no load past a row's end, the fixed team_sum butterfly.
__device__ __forceinline__ blk_v2f64_t blk_ld2(const double* p) { return *reinterpret_cast<const blk_v2f64_t*>(p); }
// r = b - t (the outer iteration's true residual, t = A x)
static __global__ void k_bamg_residual(int64_t n2, const double* b, const double* t, double* r) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n2) r[i] = b[i] - t[i];
}
// ---- The cycle kernels take Q in {1, 2, 4, 8} interleaved columns (kernels_cols.h): unknown u of DOF i, column q at [(2 i + u) Q + q]; the single-column solve
// runs their Q = 1 instantiations.  A column's arithmetic does not depend on Q (the same team, the same entries to the same lanes, blk_mul_cols, team_sum, the same
// grid of partials), Q accumulator pairs per lane; the blocks and indices are read once for all columns, a gathered DOF is 2 Q contiguous doubles.  (The outer
// iteration's r = b - t is k_bamg_residual over the 2 n Q words.)
// The arithmetic is spelled out with contraction off: a.x b.x + a.y b.y as fma(a.x, b.x, a.y b.y), r - om s as fma(-om, s, r), z + om d as fma(om, d, z), every
// accumulation a plain addition; left to itself the compiler fuses the unrolled column forms differently at some widths, and a column's last bits would depend
// on its batch.
__device__ __forceinline__ blk_v2f64_t blk_mul_cols(const blk_v2f64_t top, const blk_v2f64_t bot, const blk_v2f64_t v) {
#pragma clang fp contract(off)
    return blk_v2f64_t{__builtin_fma(top.x, v.x, top.y * v.y), __builtin_fma(bot.x, v.x, bot.y * v.y)};
}
__device__ __forceinline__ double blk_dot_cols(const blk_v2f64_t u, const blk_v2f64_t w) {
#pragma clang fp contract(off)
    return __builtin_fma(u.x, w.x, u.y * w.y);
}
template <int Q> __device__ __forceinline__ void blk_ld_cols(const double* p, blk_v2f64_t (&v)[Q]) {   // p = base + 2 i Q
    double a[Q], b[Q];
    ld_cols<Q>(p, a), ld_cols<Q>(p + Q, b);
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = blk_v2f64_t{a[q], b[q]};
}
template <int Q> __device__ __forceinline__ void blk_st_cols(double* p, const blk_v2f64_t (&v)[Q]) {
    double a[Q], b[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) a[q] = v[q].x, b[q] = v[q].y;
    st_cols<Q>(p, a), st_cols<Q>(p + Q, b);
}
// k_block_spmv for the Q >= 2 columns of a batch's outer iteration (no stop flag)
template <int T, int Q>
static __global__ __launch_bounds__(256) void k_block_spmv_cols(int64_t n, const int32_t* rowptr, const int32_t* colidx, const double* vals, const double* x, double* y) {
#pragma clang fp contract(off)
    constexpr int TEAMS = 256 / T;
    const int l = threadIdx.x % T;
    const int64_t row = (int64_t)blockIdx.x * TEAMS + threadIdx.x / T;
    const bool row_ok = row < n;
    const int64_t rc = row_ok ? row : n - 1;
    const int rs = rowptr[rc], re = rowptr[rc + 1];
    double a0[Q], a1[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) a0[q] = 0.0, a1[q] = 0.0;
    for (int k = rs + l; k < re; k += T) {
        const blk_v2f64_t* v = reinterpret_cast<const blk_v2f64_t*>(vals + 4 * (int64_t)k);
        const blk_v2f64_t top = v[0], bot = v[1];
        const int col = colidx[k];
        blk_v2f64_t xp[Q];
        blk_ld_cols<Q>(x + 2 * (int64_t)col * Q, xp);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const blk_v2f64_t t = blk_mul_cols(top, bot, xp[q]);
            a0[q] += t.x, a1[q] += t.y;
        }
    }
    blk_v2f64_t o[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) o[q] = blk_v2f64_t{team_sum<T>(a0[q]), team_sum<T>(a1[q])};
    if (l == 0 && row_ok) blk_st_cols<Q>(y + 2 * row * Q, o);
}
// pre-smoothing from zero and the restricted residual in one pass, a team per aggregate: zt_i = om D_i^-1 r_i for its members i, and
// rc_a = sum over members of (r_i - om sum_j A_ij D_j^-1 r_j); unknown u of aggregate a, column q at rc[(2 a + u) rs + q cs] (interleaved, or column-major for
// the dense inverse of the coarsest level)
template <int T, int Q>
static __global__ __launch_bounds__(256) void k_bamg_pre_restrict(int64_t nc, const int32_t* mptr, const int32_t* midx, const int32_t* rp, const int32_t* ci,
                                                                  const double* bv, const double* dinv, double om, const double* r, double* zt, double* rc,
                                                                  int64_t rs, int64_t cs) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x % T;
    const int64_t ag = (int64_t)blockIdx.x * (256 / T) + threadIdx.x / T;
    if (ag >= nc) return;
    double c0[Q], c1[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) c0[q] = 0.0, c1[q] = 0.0;
    for (int32_t m = mptr[ag]; m < mptr[ag + 1]; ++m) {
        const int32_t i = midx[m];
        double s0[Q], s1[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) s0[q] = 0.0, s1[q] = 0.0;
        for (int32_t k = rp[i] + lane; k < rp[i + 1]; k += T) {
            const blk_v2f64_t top = blk_ld2(bv + 4 * (int64_t)k), bot = blk_ld2(bv + 4 * (int64_t)k + 2);
            const int64_t j = ci[k];
            const blk_v2f64_t dt = blk_ld2(dinv + 4 * j), db = blk_ld2(dinv + 4 * j + 2);
            blk_v2f64_t rj[Q];
            blk_ld_cols<Q>(r + 2 * j * Q, rj);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const blk_v2f64_t y = blk_mul_cols(dt, db, rj[q]);
                const blk_v2f64_t t = blk_mul_cols(top, bot, y);
                s0[q] += t.x, s1[q] += t.y;
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) s0[q] = team_sum<T>(s0[q]), s1[q] = team_sum<T>(s1[q]);
        blk_v2f64_t ri[Q];
        blk_ld_cols<Q>(r + 2 * (int64_t)i * Q, ri);
        if (lane == 0) {
            const blk_v2f64_t dt = blk_ld2(dinv + 4 * (int64_t)i), db = blk_ld2(dinv + 4 * (int64_t)i + 2);
            blk_v2f64_t z[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const blk_v2f64_t y = blk_mul_cols(dt, db, ri[q]);
                z[q] = blk_v2f64_t{om * y.x, om * y.y};
            }
            blk_st_cols<Q>(zt + 2 * (int64_t)i * Q, z);
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) c0[q] += __builtin_fma(-om, s0[q], ri[q].x), c1[q] += __builtin_fma(-om, s1[q], ri[q].y);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) rc[2 * ag * rs + q * cs] = c0[q], rc[(2 * ag + 1) * rs + q * cs] = c1[q];
    }
}
// out_i = z_i + om D_i^-1 (r_i - sum_j A_ij z_j) with z = zt + P e: prolongation (every row has an aggregate), residual and post-smoothing in one pass
template <int T, int Q>
static __global__ __launch_bounds__(256) void k_bamg_post(int64_t n, const int32_t* rp, const int32_t* ci, const double* bv, const double* dinv, double om,
                                                          const int32_t* agg, const double* e, const double* r, const double* zt, double* out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x % T;
    const int64_t i = (int64_t)blockIdx.x * (256 / T) + threadIdx.x / T;
    if (i >= n) return;
    double s0[Q], s1[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) s0[q] = 0.0, s1[q] = 0.0;
    for (int32_t k = rp[i] + lane; k < rp[i + 1]; k += T) {
        const blk_v2f64_t top = blk_ld2(bv + 4 * (int64_t)k), bot = blk_ld2(bv + 4 * (int64_t)k + 2);
        const int64_t j = ci[k];
        blk_v2f64_t zj[Q], eg[Q];
        blk_ld_cols<Q>(zt + 2 * j * Q, zj), blk_ld_cols<Q>(e + 2 * (int64_t)agg[j] * Q, eg);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const blk_v2f64_t z = zj[q] + eg[q];
            const blk_v2f64_t t = blk_mul_cols(top, bot, z);
            s0[q] += t.x, s1[q] += t.y;
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) s0[q] = team_sum<T>(s0[q]), s1[q] = team_sum<T>(s1[q]);
    if (lane == 0) {
        const blk_v2f64_t dt = blk_ld2(dinv + 4 * i), db = blk_ld2(dinv + 4 * i + 2);
        blk_v2f64_t zi[Q], eg[Q], ri[Q], o[Q];
        blk_ld_cols<Q>(zt + 2 * i * Q, zi), blk_ld_cols<Q>(e + 2 * (int64_t)agg[i] * Q, eg), blk_ld_cols<Q>(r + 2 * i * Q, ri);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const blk_v2f64_t z = zi[q] + eg[q];
            const blk_v2f64_t d = blk_mul_cols(dt, db, blk_v2f64_t{ri[q].x - s0[q], ri[q].y - s1[q]});
            o[q] = blk_v2f64_t{__builtin_fma(om, d.x, z.x), __builtin_fma(om, d.y, z.y)};
        }
        blk_st_cols<Q>(out + 2 * i * Q, o);
    }
}
// y = A x and the three dot products p_d . q_d of a GCR step per column (any of the vectors may be y itself) as per-workgroup partials
// part[(d Q + q) gridDim.x + block]: a fixed grid, every team strides over the rows, the same bits every run.
// ADD: add[i Q + q] (the factored data term's share of the row, kernels_obs.h k_obs_scatter_store) joins the first component of row i before the products;
// algorithmic bytes per launch 36 nnz + 4 (n + 1) + 16 n (x) + 16 n (y) + 16 n per vector of the dots that is not y, and 8 n more for add
template <int T, int Q, bool ADD = false>
static __global__ __launch_bounds__(256) void k_bamg_spmv_dots(int64_t n, const int32_t* rp, const int32_t* ci, const double* bv, const double* x, double* y,
                                                               const double* p0, const double* q0, const double* p1, const double* q1, const double* p2,
                                                               const double* q2, double* part, const double* add = nullptr) {
#pragma clang fp contract(off)
    __shared__ double red[3 * Q][4];
    const int lane = threadIdx.x % T;
    double d0[Q], d1[Q], d2[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) d0[q] = d1[q] = d2[q] = 0.0;
    const int64_t teams = (int64_t)gridDim.x * (256 / T);
    for (int64_t i = (int64_t)blockIdx.x * (256 / T) + threadIdx.x / T; i < n; i += teams) {
        double s0[Q], s1[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) s0[q] = 0.0, s1[q] = 0.0;
        for (int32_t k = rp[i] + lane; k < rp[i + 1]; k += T) {
            const blk_v2f64_t top = blk_ld2(bv + 4 * (int64_t)k), bot = blk_ld2(bv + 4 * (int64_t)k + 2);
            blk_v2f64_t xj[Q];
            blk_ld_cols<Q>(x + 2 * (int64_t)ci[k] * Q, xj);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const blk_v2f64_t t = blk_mul_cols(top, bot, xj[q]);
                s0[q] += t.x, s1[q] += t.y;
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) s0[q] = team_sum<T>(s0[q]), s1[q] = team_sum<T>(s1[q]);
        if (lane == 0) {
            blk_v2f64_t yi[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) yi[q] = blk_v2f64_t{s0[q], s1[q]};
            if constexpr (ADD) {
#pragma unroll
                for (int q = 0; q < Q; ++q) yi[q].x += add[i * Q + q];
            }
            blk_st_cols<Q>(y + 2 * i * Q, yi);
            auto dots = [&](const double* a, const double* b, double (&d)[Q]) {
                blk_v2f64_t u[Q], w[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) u[q] = w[q] = yi[q];
                if (a != y) blk_ld_cols<Q>(a + 2 * i * Q, u);
                if (b != y) blk_ld_cols<Q>(b + 2 * i * Q, w);
#pragma unroll
                for (int q = 0; q < Q; ++q) d[q] += blk_dot_cols(u[q], w[q]);
            };
            dots(p0, q0, d0), dots(p1, q1, d1);
            if (p2) dots(p2, q2, d2);
        }
    }
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const double t0 = wave_sum(d0[q]), t1 = wave_sum(d1[q]), t2 = wave_sum(d2[q]);
        if ((threadIdx.x & 63) == 0) red[q][w] = t0, red[Q + q][w] = t1, red[2 * Q + q][w] = t2;
    }
    __syncthreads();
    if (threadIdx.x < 3 * Q) part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}
// Q stacked columns in the reference numbering (column q at b_ext + 2 n q) <-> interleaved internal order
static __global__ void k_block_stage_cols(int64_t n, int Q, const int32_t* i2e, const double* b_ext, double* z) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * Q) return;
    const int64_t i = t / Q, q = t - i * Q, e = i2e[i];
    z[2 * i * Q + q] = b_ext[q * 2 * n + e], z[(2 * i + 1) * Q + q] = b_ext[q * 2 * n + n + e];
}
static __global__ void k_block_unstage_cols(int64_t n, int Q, const int32_t* i2e, const double* z, double* x_ext) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * Q) return;
    const int64_t i = t / Q, q = t - i * Q, e = i2e[i];
    x_ext[q * 2 * n + e] = z[2 * i * Q + q] + 0.0, x_ext[q * 2 * n + n + e] = z[(2 * i + 1) * Q + q] + 0.0;
}
// ---- ... and its set-up: the scalar strength matrix (the block Galerkin sums are k_bamg_gsum's, beside k_amg_gsum in eng_amg.hip) ------------------------
static __global__ void k_bamg_pick(int64_t nnz, const double* bv, int q, double* out) {   // block q of every entry
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nnz) out[k] = bv[4 * k + q];
}

// ---- Psi^T W Psi on the pattern --------------------------------------------------------------------------------------------------------
static __global__ void k_block_invert_perm(int64_t n, const int32_t* i2e, int32_t* e2i) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) e2i[i2e[i]] = (int32_t)i;
}
// one lane per (location, a, b): out[slot(dof_a, dof_b)] += w psi_a psi_b, the slot found by a search in row dof_a (as the element-wise
// assembly forms do); locations outside the mesh (cell id -1) contribute nothing.  fp64 atomics: the order of the additions is not fixed.
static __global__ void k_gram_pointwise(int64_t n_locs, int nb, const int32_t* cell_ids, const int32_t* cell_e2i, const int32_t* cdofs, const double* values,
                                        const double* weights, const int32_t* rowptr, const int32_t* colidx, double* out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nb2 = nb * nb;
    if (t >= n_locs * nb2) return;
    const int64_t loc = t / nb2;
    const int ab = (int)(t - loc * nb2), a = ab / nb, b = ab - a * nb;
    const int32_t ce = cell_ids[loc];
    if (ce < 0) return;
    const int64_t ci = cell_e2i[ce];
    const int32_t i = cdofs[ci * nb + a], j = cdofs[ci * nb + b];
    const int32_t k1 = rowptr[i + 1];
    const int32_t k = blk_lower_bound(colidx, rowptr[i], k1, j);
    if (k >= k1 || colidx[k] != j) return;
    const double va = values[loc * nb + a], vb = values[loc * nb + b];
    const double term = weights ? (weights[loc] * va) * vb : va * vb;
    atomicAdd(out + k, term);
}

}  // namespace fdapde_hip
#endif
