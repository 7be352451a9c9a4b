// eng_amg.hip -- FDAPDE_SOLVER_AMG: flexible GMRES around a K-cycle over an AGGREGATION hierarchy built from the matrix alone.
//
// Why: the reference solves every system with SparseLU (fem_linear_elliptic_solver.h:38-47, the factor-once handle of utils/symbols.h:133-160), which
// does not care about mesh size or conditioning; Jacobi-preconditioned Krylov needs O(1 / h) iterations.  The two-level solver (eng_pmg.hip) takes
// that away for order-2 spaces only, and its P1 level is itself solved by Jacobi-Krylov.  A hierarchy built from the matrix serves P1 and P2, 2-D and
// 3-D, fdapde_solve, the parabolic stepper and the handle (whose matrix has no mesh behind it) alike.
//
// What:
//   set-up    level 0 is the system the reference solves (the row-zeroed matrix of fem_solver_base.h:142-155: the Dirichlet DOFs belong to no aggregate,
//             their correction is 0 on every level) or the handle's matrix, in the internal (locality) DOF order.  A level's aggregates come from TWO
//             pairwise passes of handshake matching on the strength graph (-a_ij >= theta max_k -a_ik on the symmetric part; a row without negative
//             couplings goes by |a_ij|): every free node proposes to its strongest unmatched strong neighbour (ties: a hash of the index pair), mutual proposals
//             pair, kAmgRounds rounds (from kAmgStrongRounds on weak couplings count too), leftovers stay single -- the second pass on the Galerkin matrix of the first: aggregates of at most 4 nodes
//             -- unless the pass ABSORBS (knob amg_absorb): a row the rounds left single joins the pair of its most strongly coupled paired neighbour
//             (k_amg_absorb), so an aggregate is a pair and whatever singles chose it.  The singles are an independent set that pairing alone carries from
//             level to level -- their neighbours are heavy aggregates that prefer each other -- until they are most of a level and coarsening stalls (3-D).  The
//             coarse matrix is P^T A P with piecewise-constant P, built as a stable key sort of the (agg(i), agg(j)) pairs and a segmented sum in
//             ascending fine-slot order: no float atomics, the same bits every run.  Levels until one has at most `amg_coarse_rows` rows; that one is
//             inverted once (dense_build_csr, kernels_dense.h).
//   cycle     on every level: damped Jacobi (1.5 / lambda_max(D^-1 A)), the coarse correction, damped Jacobi.  Below the finest level the coarse
//             correction is two steps of flexible CG (GCR for a non-symmetric level) preconditioned by the next level's cycle: the K-cycle of
//             Notay & Vassilevski -- with unsmoothed aggregation a V-cycle does not give counts independent of the mesh size.  Scalars stay on the
//             device (fixed-order reductions, k_amg_coef); nothing returns to the host inside the cycle.
//   outer     the flexible GMRES of the two-level solver (fgmres_outer, eng_pmg.hip) through amg_outer_cols (amg_setup.h), the run all three multilevel solvers
//             share; amg_run_cols brings this solver's product, residual and Dirichlet lift.  The level loop of the build pass is amg_build_levels' (amg_setup.h).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "context.h"
#include "amg_setup.h"
#include "engine.h"
#include "kernels_cols.h"
#include "kernels_dense.h"
#include "kernels_reduce.h"

namespace fdapde_engine {

namespace {
using namespace fdapde_hip;

// ---- set-up kernels (one thread per row: a set-up pass, not a hot path; the row rules are amg_rows.h's) ----
__global__ void k_amg_init_mate(int64_t n, const uint8_t* excl, int32_t* mate) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mate[i] = (excl && excl[i]) ? kMateExcluded : kMateFree;
}
__global__ void k_amg_strength(int64_t n, const int32_t* rp, const int32_t* ci, const double* a, const uint8_t* excl, double* sw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) amg_strength_row(i, rp, ci, a, excl, sw);
}
__global__ void k_amg_propose(int64_t n, const int32_t* rp, const int32_t* ci, const double* sw, const int32_t* mate, int relaxed, int32_t* prop) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) prop[i] = amg_propose_row(i, rp, ci, sw, mate, relaxed);
}
// mutual proposals pair (each side writes its own word: the outcome does not depend on who runs first)
__global__ void k_amg_accept(int64_t n, const int32_t* prop, int32_t* mate) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || mate[i] != kMateFree) return;
    const int32_t j = prop[i];
    if (j >= 0 && prop[j] == (int32_t)i) mate[i] = j;
}
__global__ void k_amg_absorb(int64_t n, const int32_t* rp, const int32_t* ci, const double* sw, const int32_t* mate, int32_t* host) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) host[i] = amg_absorb_row(i, rp, ci, sw, mate);
}
__global__ void k_amg_leaders(int64_t n, const int32_t* mate, const int32_t* host, int32_t* lead) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lead[i] = amg_leader(i, mate, host) ? 1 : 0;
}
__global__ void k_amg_assign(int64_t n, const int32_t* mate, const int32_t* host, const int32_t* id, int32_t* agg) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) agg[i] = amg_aggregate_of(i, mate, host, id);
}
__global__ void k_amg_compose(int64_t n, const int32_t* agg1, const int32_t* agg2, int32_t* agg) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) agg[i] = agg1[i] < 0 ? -1 : agg2[agg1[i]];
}
// Galerkin product: every entry's (agg(i) nc + agg(j)) key, `sentinel` where a side has no aggregate
__global__ void k_amg_gkeys(int64_t n, const int32_t* rp, const int32_t* ci, const int32_t* agg, uint64_t nc, uint64_t sentinel, uint64_t* keys, int32_t* idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t ai = agg[i];
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
        const int32_t aj = agg[ci[k]];
        keys[k] = (ai >= 0 && aj >= 0) ? (uint64_t)ai * nc + (uint64_t)aj : sentinel;
        idx[k] = k;
    }
}
__global__ void k_amg_heads(int64_t m, const uint64_t* keys, uint64_t sentinel, int32_t* head) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < m) head[e] = (keys[e] != sentinel && (e == 0 || keys[e] != keys[e - 1])) ? 1 : 0;
}
// one thread per coarse entry: the sum of its fine entries in ascending slot order (the stable sort kept them so)
__global__ void k_amg_gsum(int64_t m, const uint64_t* keys, const int32_t* idx, const double* a, const int32_t* head, const int32_t* pos, uint64_t nc,
                           int32_t* rp_c, int32_t* ci_c, double* a_c) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m || !head[e]) return;
    const uint64_t key = keys[e];
    double s = 0.0;
    for (int64_t q = e; q < m && keys[q] == key; ++q) s += a[idx[q]];
    const int32_t p = pos[e];
    const uint64_t row = key / nc;
    a_c[p] = s, ci_c[p] = (int32_t)(key - row * nc);
    if (e == 0 || keys[e - 1] / nc != row) rp_c[row] = p;
}
// ... and the payload of the block form, four doubles per entry, summed over the same fine entries in the same order
__global__ void k_bamg_gsum(int64_t m, const uint64_t* keys, const int32_t* idx, const int32_t* head, const int32_t* pos, const double* bv, double* bv_c) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m || !head[e]) return;
    const uint64_t key = keys[e];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int64_t q = e; q < m && keys[q] == key; ++q) {
        const double* v = bv + 4 * (int64_t)idx[q];
        s0 += v[0], s1 += v[1], s2 += v[2], s3 += v[3];
    }
    double* o = bv_c + 4 * (int64_t)pos[e];
    o[0] = s0, o[1] = s1, o[2] = s2, o[3] = s3;
}
// ... and a payload of any other width (the Kronecker form's n_S spatial values per entry): one thread per coarse entry and component, the same order
__global__ void k_amg_gsum_pay(int64_t m, int width, const uint64_t* keys, const int32_t* idx, const int32_t* head, const int32_t* pos, const double* pay, double* pay_c) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e = t / width;
    if (e >= m || !head[e]) return;
    const int s = (int)(t - e * width);
    const uint64_t key = keys[e];
    double sum = 0.0;
    for (int64_t q = e; q < m && keys[q] == key; ++q) sum += pay[(int64_t)width * idx[q] + s];
    pay_c[(int64_t)width * pos[e] + s] = sum;
}
// members of every aggregate, ascending: keys agg(i) (nc for none), sorted stably with the row index
__global__ void k_amg_mkeys(int64_t n, const int32_t* agg, uint32_t nc, uint32_t* keys, int32_t* idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = agg[i] >= 0 ? (uint32_t)agg[i] : nc, idx[i] = (int32_t)i;
}
__global__ void k_amg_mptr(int64_t n, const uint32_t* keys, uint32_t nc, int32_t* mptr) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    if (e == 0 || keys[e] != keys[e - 1]) mptr[keys[e]] = (int32_t)e;   // (keys[e] <= nc: mptr has nc + 1 words)
    if (e == n - 1 && keys[e] < nc) mptr[nc] = (int32_t)n;
}
// D^-1 (0 on the excluded rows); flag: a free row without a usable diagonal entry
__global__ void k_amg_dinv(int64_t n, const int32_t* rp, const int32_t* ci, const double* a, const uint8_t* excl, double* dinv, int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (excl && excl[i]) {
        dinv[i] = 0.0;
        return;
    }
    double d = 0.0;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k)
        if (ci[k] == (int32_t)i) d = a[k];
    const double v = 1.0 / d;
    if (!(d != 0.0) || !isfinite(v)) atomicOr(flag, 1), dinv[i] = 0.0;
    else dinv[i] = v;
}
// y = D^-1 A x (the power iteration's operator)
__global__ void k_amg_dax(int64_t n, const int32_t* rp, const int32_t* ci, const double* a, const double* dinv, const double* x, double* y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) s += a[k] * x[ci[k]];
    y[i] = dinv[i] * s;
}
__global__ void k_amg_hashvec(int64_t n, const double* dinv, double* x) {   // a fixed pseudo-random start (0 where D^-1 is)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull, z = (z ^ (z >> 27)) * 0x94D049BB133111EBull, z ^= z >> 31;
    x[i] = dinv[i] == 0.0 ? 0.0 : (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}
__global__ void k_amg_scale(int64_t n, const double* a, double f, double* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = f * a[i];
}

// ---- cycle kernels: a team of T lanes per row (coarse levels are latency-bound: few launches, each fused as far as the data flow allows), for Q interleaved
// columns (kernels_cols.h): word i of column q at [i * Q + q].  A column's arithmetic does not depend on Q -- the same team width, the same entries to the same
// lanes, the same team_sum / wave_sum / block_sum, the same grid of partials -- with Q accumulators per lane; the matrix and its indices are read once for all
// columns, a gathered operand is Q contiguous doubles.  No column reads another.  The single-column solve runs the Q = 1 instantiations.
// These kernels (and the Gram-Schmidt kernels of eng_pmg.hip) write each expression once and leave its contraction to the compiler, which fuses the unrolled per-column
// copies of every width, Q = 1 included, alike (s += a x, r - om s, z + om d (r - s), w -= h v): that is a property of this compiler, not of the language -- the
// block forms in kernels_block.h needed theirs spelled out.  tests/test_gpu_amg_cols.py holds every column of Q = 2, 4, 8 to the Q = 1 run's bits on 2-D and
// 3-D, P1 and P2 hierarchies; if a toolchain changes a width's fusion that test fails, and the remedy is kernels_block.h's.
// tests/test_gpu_amg_iterates.py holds the result of every width to an extended-precision restatement of the cycle on the device's own aggregates and damping
// (fdapde_amg_aggregates, fdapde_amg_damping): the k-th iterate within a few hundred u of its scale, measured 2 - 80.

// pre-smoothing from zero and the restricted residual in one pass, a team per aggregate: zt_i = om d_i r_i for its members, and
// rc_a = sum over members i of (r_i - sum_j a_ij om d_j r_j); word w of column q of rc at rc[w * rs + q * cs] (interleaved, or column-major for the dense
// inverse of the coarsest level)
template <int T, int Q>
__global__ __launch_bounds__(256) void k_amg_pre_restrict(int64_t nc, const int32_t* mptr, const int32_t* midx, const int32_t* rp, const int32_t* ci, const double* a,
                                                          const double* dinv, double om, const double* r, double* zt, double* rc, int64_t rs, int64_t cs) {
    const int lane = threadIdx.x & (T - 1);
    const int64_t ag = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / T;
    if (ag >= nc) return;
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    for (int32_t m = mptr[ag]; m < mptr[ag + 1]; ++m) {
        const int32_t i = midx[m];
        double s[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) s[q] = 0.0;
        for (int32_t k = rp[i] + lane; k < rp[i + 1]; k += T) {
            const int32_t j = ci[k];
            const double ak = a[k], dj = dinv[j];
            double rj[Q];
            ld_cols<Q>(r + (int64_t)j * Q, rj);
#pragma unroll
            for (int q = 0; q < Q; ++q) s[q] += ak * (dj * rj[q]);
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) s[q] = team_sum<T>(s[q]);
        double ri[Q];
        ld_cols<Q>(r + (int64_t)i * Q, ri);
        if (lane == 0) {
            double z[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) z[q] = om * dinv[i] * ri[q];
            st_cols<Q>(zt + (int64_t)i * Q, z);
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] += ri[q] - om * s[q];
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) rc[ag * rs + q * cs] = acc[q];
    }
}
// out_i = z_i + om d_i (r_i - sum_j a_ij z_j) with z = zt + P e (the coarse correction prolongated on the fly)
template <int T, int Q>
__global__ __launch_bounds__(256) void k_amg_post(int64_t n, const int32_t* rp, const int32_t* ci, const double* a, const double* dinv, double om, const int32_t* agg,
                                                  const double* e, const double* r, const double* zt, double* out) {
    const int lane = threadIdx.x & (T - 1);
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / T;
    if (i >= n) return;
    double s[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] = 0.0;
    for (int32_t k = rp[i] + lane; k < rp[i + 1]; k += T) {
        const int32_t j = ci[k], g = agg[j];
        const double ak = a[k];
        double zj[Q], eg[Q];
        ld_cols<Q>(zt + (int64_t)j * Q, zj);
        if (g >= 0) ld_cols<Q>(e + (int64_t)g * Q, eg);
        else {
#pragma unroll
            for (int q = 0; q < Q; ++q) eg[q] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) s[q] += ak * (zj[q] + eg[q]);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] = team_sum<T>(s[q]);
    if (lane == 0) {
        const int32_t g = agg[i];
        double zi[Q], eg[Q], ri[Q], o[Q];
        ld_cols<Q>(zt + i * Q, zi), ld_cols<Q>(r + i * Q, ri);
        if (g >= 0) ld_cols<Q>(e + (int64_t)g * Q, eg);
        else {
#pragma unroll
            for (int q = 0; q < Q; ++q) eg[q] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const double z = zi[q] + eg[q];
            o[q] = z + om * dinv[i] * (ri[q] - s[q]);
        }
        st_cols<Q>(out + i * Q, o);
    }
}
// y = A x and up to three dot products p_d . q_d per column (any of them may be y itself) as per-workgroup partials part[(d Q + q) gridDim.x + block]: a fixed
// grid, the same bits every run
template <int T, int Q>
__global__ __launch_bounds__(256) void k_amg_spmv_dots(int64_t n, const int32_t* rp, const int32_t* ci, const double* a, const double* x, double* y, const double* p0,
                                                       const double* q0, const double* p1, const double* q1, const double* p2, const double* q2, double* part) {
    __shared__ double red[3 * Q][4];
    const int lane = threadIdx.x & (T - 1);
    double d0[Q], d1[Q], d2[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) d0[q] = d1[q] = d2[q] = 0.0;
    const int64_t teams = (int64_t)gridDim.x * blockDim.x / T;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / T; i < n; i += teams) {
        double s[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) s[q] = 0.0;
        for (int32_t k = rp[i] + lane; k < rp[i + 1]; k += T) {
            const double ak = a[k];
            double xj[Q];
            ld_cols<Q>(x + (int64_t)ci[k] * Q, xj);
#pragma unroll
            for (int q = 0; q < Q; ++q) s[q] += ak * xj[q];
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) s[q] = team_sum<T>(s[q]);
        if (lane == 0) {
            st_cols<Q>(y + i * Q, s);
            auto dot = [&](const double* u, const double* v, double (&d)[Q]) {
                double uv[Q], vv[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) uv[q] = vv[q] = s[q];
                if (u != y) ld_cols<Q>(u + i * Q, uv);
                if (v != y) ld_cols<Q>(v + i * Q, vv);
#pragma unroll
                for (int q = 0; q < Q; ++q) d[q] += uv[q] * vv[q];
            };
            dot(p0, q0, d0), dot(p1, q1, d1);
            if (p2) dot(p2, q2, d2);
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
// the K-cycle's scalars from the partials of k_amg_spmv_dots, a workgroup per column: column blockIdx.x of Q reads part[(d Q + q) np ..] and keeps its scalars
// in sc[8 q ..].  Stage 1 (c = B b, v = A c): FCG rho1 = c.v, alpha1 = c.b; GCR rho1 = v.v, alpha1 = v.b; sc[0] = rho1, sc[1] = alpha1 / rho1.  Stage 2
// (rt = b - sc[1] v, d = B rt, w = A d): FCG gamma = d.v, rho2 = d.w - gamma^2 / rho1, alpha2 = d.rt; GCR gamma = v.w, rho2 = w.w - gamma^2 / rho1,
// alpha2 = w.rt; the correction e = sc[2] c + sc[3] d.  A step that cannot be taken (rho <= 0, not finite) contributes nothing: the guards are the column's own
__global__ __launch_bounds__(256) void k_amg_coef(const double* part, int np, int Q, int stage, double* sc_all) {
    __shared__ double red[5];
    const int col = blockIdx.x;
    double* sc = sc_all + 8 * col;
    double t[3];
    for (int q = 0; q < 3; ++q) {
        double s = 0.0;
        for (int i = threadIdx.x; i < np; i += 256) s += part[((size_t)q * Q + col) * np + i];
        t[q] = block_sum(s, red);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (stage == 1) {
        const double rho1 = t[0], a1 = rho1 > 0.0 && isfinite(rho1) ? t[1] / rho1 : 0.0;
        sc[0] = rho1, sc[1] = isfinite(a1) ? a1 : 0.0;
    } else {
        const double rho1 = sc[0], gamma = t[0];
        const double rho2 = rho1 > 0.0 ? t[1] - gamma * gamma / rho1 : 0.0;
        double cd = rho2 > 0.0 && isfinite(rho2) ? t[2] / rho2 : 0.0;
        double cc = sc[1] - (rho1 > 0.0 ? cd * gamma / rho1 : 0.0);
        if (!isfinite(cd) || !isfinite(cc)) cd = 0.0, cc = sc[1];
        sc[2] = cc, sc[3] = cd;
    }
}
template <int Q> __global__ void k_amg_axpy_sc(int64_t n, const double* b, const double* v, const double* sc, double* rt) {   // rt_q = b_q - sc[8 q + 1] v_q
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double bi[Q], vi[Q], o[Q];
    ld_cols<Q>(b + i * Q, bi), ld_cols<Q>(v + i * Q, vi);
#pragma unroll
    for (int q = 0; q < Q; ++q) o[q] = bi[q] - sc[8 * q + 1] * vi[q];
    st_cols<Q>(rt + i * Q, o);
}
template <int Q> __global__ void k_amg_comb2(int64_t n, const double* cv, const double* dv, const double* sc, double* e) {   // e_q = sc[8 q + 2] c_q + sc[8 q + 3] d_q
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double ci[Q], di[Q], o[Q];
    ld_cols<Q>(cv + i * Q, ci), ld_cols<Q>(dv + i * Q, di);
#pragma unroll
    for (int q = 0; q < Q; ++q) o[q] = sc[8 * q + 2] * ci[q] + sc[8 * q + 3] * di[q];
    st_cols<Q>(e + i * Q, o);
}
// the finest level's system: y = K x (the Dirichlet rows as unit rows if use_bnd); with f: r = rhs - K x (rhs = f, g on the Dirichlet rows)
template <int T, int Q>
__global__ __launch_bounds__(256) void k_amg_apply_K(int64_t n, const int32_t* rp, const int32_t* ci, const double* a, const uint8_t* bnd, int use_bnd, const double* x,
                                                     const double* f, const double* g, double* y) {
    const int lane = threadIdx.x & (T - 1);
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / T;
    if (i >= n) return;
    const bool unit = use_bnd && bnd[i];
    double s[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] = 0.0;
    if (!unit)
        for (int32_t k = rp[i] + lane; k < rp[i + 1]; k += T) {
            const double ak = a[k];
            double xj[Q];
            ld_cols<Q>(x + (int64_t)ci[k] * Q, xj);
#pragma unroll
            for (int q = 0; q < Q; ++q) s[q] += ak * xj[q];
        }
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] = team_sum<T>(s[q]);
    if (lane == 0) {
        double o[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const double kx = unit ? x[i * Q + q] : s[q];
            o[q] = f ? (unit ? g[i * Q + q] : f[i * Q + q]) - kx : kx;
        }
        st_cols<Q>(y + i * Q, o);
    }
}
// x = g on the Dirichlet rows; elsewhere x0 (a warm start) or 0 (any layout: elementwise over the n Q words, row = e / Q)
__global__ void k_amg_start(int64_t n, int Q, const uint8_t* bnd, int use_bnd, const double* g, const double* x0, double* x) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n * Q) x[e] = (use_bnd && bnd[e / Q]) ? g[e] : (x0 ? x0[e] : 0.0);
}
// the handle's columns between the reference numbering (column-major n x Q) and the internal order (interleaved)
__global__ void k_amg_gather(int64_t n, int Q, const int32_t* idx, const double* src, double* dst) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * Q) return;
    const int64_t i = e / Q, q = e - i * Q;
    dst[e] = src[q * n + idx[i]];
}
__global__ void k_amg_scatter(int64_t n, int Q, const int32_t* idx, const double* src, double* dst) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * Q) return;
    const int64_t i = e / Q, q = e - i * Q;
    dst[q * n + idx[i]] = src[e];
}
template <typename T> bool same_dev(const T* p, size_t n, const std::vector<T>& h) {
    if (h.size() != n) return false;
    std::vector<T> g(n);
    if (n && hipMemcpy(g.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost) != hipSuccess) return false;
    return n == 0 || std::memcmp(g.data(), h.data(), sizeof(T) * n) == 0;
}

// one pairwise pass on the device (absorb: followed by the absorption of the rows it left single): agg (n words), *nc
int dev_pairwise(fdapde_ctx* c, int64_t n, int64_t nnz, const int32_t* rp, const int32_t* ci, const double* a, const uint8_t* excl, int absorb, DBuf<int32_t>& agg,
                 int32_t* nc) {
    hipStream_t st = c->stream;
    const dim3 bv(256);
    DBuf<double> sw;
    DBuf<int32_t> mate, prop, lead, id, host;
    DBuf<char> tmp;
    HIPCHK(c, sw.alloc((size_t)nnz));
    HIPCHK(c, mate.alloc((size_t)n));
    HIPCHK(c, prop.alloc((size_t)n));
    HIPCHK(c, lead.alloc((size_t)n + 1));
    HIPCHK(c, id.alloc((size_t)n + 1));
    HIPCHK(c, agg.alloc((size_t)n));
    hipLaunchKernelGGL(k_amg_strength, dim3(gn(n)), bv, 0, st, n, rp, ci, a, excl, sw.p);
    hipLaunchKernelGGL(k_amg_init_mate, dim3(gn(n)), bv, 0, st, n, excl, mate.p);
    for (int round = 0; round < kAmgRounds; ++round) {
        hipLaunchKernelGGL(k_amg_propose, dim3(gn(n)), bv, 0, st, n, rp, ci, sw.p, mate.p, round >= kAmgStrongRounds ? 1 : 0, prop.p);
        hipLaunchKernelGGL(k_amg_accept, dim3(gn(n)), bv, 0, st, n, prop.p, mate.p);
    }
    if (absorb) {
        HIPCHK(c, host.alloc((size_t)n));
        hipLaunchKernelGGL(k_amg_absorb, dim3(gn(n)), bv, 0, st, n, rp, ci, sw.p, mate.p, host.p);
    }
    HIPCHK(c, hipMemsetAsync(lead.p + n, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_amg_leaders, dim3(gn(n)), bv, 0, st, n, mate.p, (const int32_t*)host.p, lead.p);
    size_t need = 0;
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(nullptr, need, lead.p, id.p, (int)(n + 1), st));
    HIPCHK(c, tmp.alloc(need));
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(tmp.p, need, lead.p, id.p, (int)(n + 1), st));
    hipLaunchKernelGGL(k_amg_assign, dim3(gn(n)), bv, 0, st, n, mate.p, (const int32_t*)host.p, id.p, agg.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(nc, id.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDAPDE_OK;
}
inline int key_bits(uint64_t v) {
    int b = 1;
    while (b < 64 && (v >> b) != 0) ++b;
    return b;
}

// the Galerkin product P^T A P of piecewise-constant P (agg) on the device: a stable key sort, a segmented sum in ascending fine-slot order.  pay (or
// NULL): `width` doubles per entry (the block form's four, the Kronecker form's n_S), summed per coarse entry over the same sorted slots into pay_c
int dev_galerkin(fdapde_ctx* c, int64_t n, int64_t nnz, const int32_t* rp, const int32_t* ci, const double* a, const int32_t* agg, int32_t nc, AmgLevel& out,
                 const double* pay, int width, DBuf<double>* pay_c) {
    if (pay && width < 1) return fail(c, FDAPDE_EINVAL, "dev_galerkin: a payload of no width");
    hipStream_t st = c->stream;
    const dim3 bv(256);
    const uint64_t ncu = (uint64_t)nc, sentinel = ncu * ncu;
    DBuf<uint64_t> keys, keys_s;
    DBuf<int32_t> idx, idx_s, head, pos;
    DBuf<char> tmp;
    HIPCHK(c, keys.alloc((size_t)nnz));
    HIPCHK(c, keys_s.alloc((size_t)nnz));
    HIPCHK(c, idx.alloc((size_t)nnz));
    HIPCHK(c, idx_s.alloc((size_t)nnz));
    HIPCHK(c, head.alloc((size_t)nnz + 1));
    HIPCHK(c, pos.alloc((size_t)nnz + 1));
    hipLaunchKernelGGL(k_amg_gkeys, dim3(gn(n)), bv, 0, st, n, rp, ci, agg, ncu, sentinel, keys.p, idx.p);
    const int end_bit = key_bits(sentinel);
    size_t need_sort = 0, need_scan = 0;
    HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(nullptr, need_sort, keys.p, keys_s.p, idx.p, idx_s.p, (int)nnz, 0, end_bit, st));
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(nullptr, need_scan, head.p, pos.p, (int)(nnz + 1), st));
    HIPCHK(c, tmp.alloc(std::max(need_sort, need_scan)));
    HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(tmp.p, need_sort, keys.p, keys_s.p, idx.p, idx_s.p, (int)nnz, 0, end_bit, st));
    HIPCHK(c, hipMemsetAsync(head.p + nnz, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_amg_heads, dim3(gn(nnz)), bv, 0, st, nnz, keys_s.p, sentinel, head.p);
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(tmp.p, need_scan, head.p, pos.p, (int)(nnz + 1), st));
    int32_t nnz_c = 0;
    HIPCHK(c, hipMemcpyAsync(&nnz_c, pos.p + nnz, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    out.n = nc, out.nnz = nnz_c;
    HIPCHK(c, out.rp_own.alloc((size_t)nc + 1));
    HIPCHK(c, out.ci_own.alloc((size_t)std::max(nnz_c, 1)));
    HIPCHK(c, out.a_own.alloc((size_t)std::max(nnz_c, 1) + 2));
    if (pay) HIPCHK(c, pay_c->alloc((size_t)width * (size_t)std::max(nnz_c, 1)));
    HIPCHK(c, hipMemcpyAsync(out.rp_own.p + nc, &nnz_c, sizeof(int32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_amg_gsum, dim3(gn(nnz)), bv, 0, st, nnz, keys_s.p, idx_s.p, a, head.p, pos.p, ncu, out.rp_own.p, out.ci_own.p, out.a_own.p);
    if (pay && width == 4) hipLaunchKernelGGL(k_bamg_gsum, dim3(gn(nnz)), bv, 0, st, nnz, keys_s.p, idx_s.p, head.p, pos.p, pay, pay_c->p);
    else if (pay) hipLaunchKernelGGL(k_amg_gsum_pay, dim3(gn(nnz * width)), bv, 0, st, nnz, width, keys_s.p, idx_s.p, head.p, pos.p, pay, pay_c->p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));   // (nnz_c is this frame's; the scratch goes out of scope)
    out.rp = out.rp_own.p, out.ci = out.ci_own.p, out.a = out.a_own.p;
    return FDAPDE_OK;
}
// members of each aggregate (CSR, ascending row index)
int dev_members(fdapde_ctx* c, int64_t n, const int32_t* agg, int32_t nc, DBuf<int32_t>& mptr, DBuf<int32_t>& midx) {
    hipStream_t st = c->stream;
    const dim3 bv(256);
    DBuf<uint32_t> keys, keys_s;
    DBuf<int32_t> idx;
    DBuf<char> tmp;
    HIPCHK(c, keys.alloc((size_t)n));
    HIPCHK(c, keys_s.alloc((size_t)n));
    HIPCHK(c, idx.alloc((size_t)n));
    HIPCHK(c, midx.alloc((size_t)n));
    HIPCHK(c, mptr.alloc((size_t)nc + 1));
    hipLaunchKernelGGL(k_amg_mkeys, dim3(gn(n)), bv, 0, st, n, agg, (uint32_t)nc, keys.p, idx.p);
    size_t need = 0;
    const int end_bit = key_bits((uint64_t)nc);
    HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys.p, keys_s.p, idx.p, midx.p, (int)n, 0, end_bit, st));
    HIPCHK(c, tmp.alloc(need));
    HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(tmp.p, need, keys.p, keys_s.p, idx.p, midx.p, (int)n, 0, end_bit, st));
    hipLaunchKernelGGL(k_amg_mptr, dim3(gn(n)), bv, 0, st, n, keys_s.p, (uint32_t)nc, mptr.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    return FDAPDE_OK;
}
// the level step of F by the host loops (host_amg.cpp), compared bit for bit with what amg_coarsen built
int amg_check_level(fdapde_ctx* c, const AmgLevel& F, int absorb, const double* pay, int width, const char* tag, size_t level, const AmgCoarse& K, const AmgLevel& N,
                    const DBuf<double>* payN) {
    HostCsr hf;
    std::vector<uint8_t> excl;
    std::vector<double> hpay;
    hf.n = F.n;
    if (int rc = fetch(c, F.rp, (size_t)F.n + 1, hf.rp)) return rc;
    if (int rc = fetch(c, F.ci, (size_t)F.nnz, hf.ci)) return rc;
    if (int rc = fetch(c, F.a, (size_t)F.nnz, hf.a)) return rc;
    if (F.excl)
        if (int rc = fetch(c, F.excl, (size_t)F.n, excl)) return rc;
    if (pay)
        if (int rc = fetch(c, pay, (size_t)width * (size_t)F.nnz, hpay)) return rc;
    HostCoarse h;
    host_coarsen(hf, F.excl ? excl.data() : nullptr, absorb, pay ? hpay.data() : nullptr, width, h);
    const std::string vals = pay ? " strength values" : " values";
    std::string which;
    if (h.n1 != K.n1 || !same_dev(K.agg1.p, (size_t)F.n, h.agg1)) which += " pass-1 aggregates";
    if (h.n2 != K.n2 || (h.n1 == K.n1 && !same_dev(K.agg2.p, (size_t)K.n1, h.agg2))) which += " pass-2 aggregates";
    if (which.empty()) {
        if (!same_dev(K.T.rp, (size_t)K.n1 + 1, h.T.rp) || !same_dev(K.T.ci, (size_t)K.T.nnz, h.T.ci)) which += " pair-graph pattern";
        else if (!same_dev(K.T.a, (size_t)K.T.nnz, h.T.a)) which += " pair-graph" + vals;
        else if (pay && !same_dev(K.payT.p, (size_t)width * (size_t)K.T.nnz, h.payT)) which += " pair-graph block values";
        if (!same_dev(N.rp, (size_t)K.n2 + 1, h.N.rp) || !same_dev(N.ci, (size_t)N.nnz, h.N.ci)) which += " coarse pattern";
        else if (!same_dev(N.a, (size_t)N.nnz, h.N.a)) which += " coarse" + vals;
        else if (pay && !same_dev(payN->p, (size_t)width * (size_t)N.nnz, h.payN)) which += " coarse block values";
        if (!same_dev(F.agg.p, (size_t)F.n, h.agg)) which += " composite aggregates";
        if (!same_dev(F.mptr.p, (size_t)K.n2 + 1, h.mptr) || !same_dev(F.midx.p, h.midx.size(), h.midx)) which += " members";
    }
    if (which.empty()) return FDAPDE_OK;
    c->err = std::string("amg_setup_check: ") + tag + "level " + std::to_string(level) + ": the device-built hierarchy differs from the host-built one:" + which;
    return FDAPDE_EHIP;
}
}   // namespace

int amg_coarsen(fdapde_ctx* c, AmgLevel& F, int absorb, const double* pay, int width, AmgCoarse& K, AmgLevel& N, DBuf<double>* payN) {
    if (int rc = dev_pairwise(c, F.n, F.nnz, F.rp, F.ci, F.a, F.excl, absorb, K.agg1, &K.n1)) return rc;
    if (K.n1 == 0) return FDAPDE_OK;
    AmgLevel& T = K.T;
    if (int rc = dev_galerkin(c, F.n, F.nnz, F.rp, F.ci, F.a, K.agg1.p, K.n1, T, pay, width, &K.payT)) return rc;
    if (int rc = dev_pairwise(c, T.n, T.nnz, T.rp, T.ci, T.a, nullptr, absorb, K.agg2, &K.n2)) return rc;
    if (int rc = dev_galerkin(c, T.n, T.nnz, T.rp, T.ci, T.a, K.agg2.p, K.n2, N, pay ? K.payT.p : nullptr, width, payN)) return rc;
    HIPCHK(c, F.agg.alloc((size_t)F.n));
    hipLaunchKernelGGL(k_amg_compose, dim3(gn(F.n)), dim3(256), 0, c->stream, F.n, K.agg1.p, K.agg2.p, F.agg.p);
    HIPCHK(c, hipGetLastError());
    return dev_members(c, F.n, F.agg.p, K.n2, F.mptr, F.midx);
}

int amg_next_level(fdapde_ctx* c, AmgLevel& F, int absorb, const double* pay, int width, int per, int64_t coarse_rows, int64_t dense_limit, const char* tag,
                   size_t level, AmgLevel& N, DBuf<double>* payN, AmgVerdict* verdict) {
    AmgCoarse K;
    if (int rc = amg_coarsen(c, F, absorb, pay, width, K, N, payN)) return rc;
    *verdict = kAmgNoFreeRows;
    if (K.n1 == 0) return FDAPDE_OK;
    if (c->amg_setup_check)
        if (int rc = amg_check_level(c, F, absorb, pay, width, tag, level, K, N, payN)) return rc;
    *verdict = kAmgNext;
    if ((double)K.n2 > kAmgStall * (double)F.n && per * (int64_t)K.n2 > coarse_rows) {   // coarsening stalled: a level the dense inverse takes ends the hierarchy
        *verdict = per * F.n > dense_limit ? kAmgStalled : kAmgEnd;
        F.agg.release(), F.mptr.release(), F.midx.release();
    }
    return FDAPDE_OK;
}

namespace {
// a level's work vectors laid out for Q interleaved columns (L.np is set); they only grow.  On the coarsest level b / ecm are column-major (what dense_apply
// takes), e the correction interleaved again -- one column is both.  zt is zeroed whenever the width changes: rows of no aggregate are never written, and the
// cycle reads their 0 in the current width's layout (no other vector has a row the cycle does not write before it reads it)
int level_width(fdapde_ctx* c, AmgLevel& L, int per, bool last, int Q) {
    if (L.cols == Q) return FDAPDE_OK;
    const size_t nw = (size_t)per * (size_t)std::max<int64_t>(L.n, 1) * (size_t)Q;
    for (DBuf<double>* p : {&L.b, &L.zt, &L.cv, &L.v, &L.dv, &L.w, &L.rt, &L.e}) HIPCHK(c, p->alloc(nw));
    if (last && Q > 1) HIPCHK(c, L.ecm.alloc(nw));
    HIPCHK(c, hipMemsetAsync(L.zt.p, 0, sizeof(double) * nw, c->stream));
    HIPCHK(c, L.part.alloc(3 * (size_t)Q * (size_t)std::max(L.np, 1024)));
    HIPCHK(c, L.sc.alloc(8 * (size_t)kAmgColsMax));
    HIPCHK(c, hipMemsetAsync(L.sc.p, 0, 8 * (size_t)kAmgColsMax * sizeof(double), c->stream));
    L.cols = Q;
    return FDAPDE_OK;
}

// D^-1, the Jacobi damping 1.5 / lambda_max(D^-1 A) (15 power iterations), team width and work vectors of a level
int level_prepare(fdapde_ctx* c, AmgLevel& L, bool has_next) {
    hipStream_t st = c->stream;
    const dim3 bv(256);
    const int64_t n = L.n;
    HIPCHK(c, L.dinv.alloc((size_t)n));
    DBuf<int32_t> flag;
    HIPCHK(c, flag.alloc(1));
    HIPCHK(c, hipMemsetAsync(flag.p, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_amg_dinv, dim3(gn(n)), bv, 0, st, n, L.rp, L.ci, L.a, L.excl, L.dinv.p, flag.p);
    int32_t bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (bad) return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_AMG: a level has a zero diagonal entry (its damped Jacobi smoother needs one)");
    const double per_row = n > 0 ? (double)L.nnz / (double)n : 1.0;
    L.team = per_row <= 10.0 ? 4 : per_row <= 24.0 ? 8 : 16;
    L.np = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (n * L.team + 1023) / 1024));
    if (int rc = level_width(c, L, 1, !has_next, 1)) return rc;
    L.om = 0.0;
    if (!has_next) return FDAPDE_OK;   // (the coarsest level is inverted, not smoothed)
    // lambda_max(D^-1 A) by the power iteration (as the two-level solver's); the dots in a fixed order
    double* x = L.v.p;
    double* y = L.w.p;
    double h[3] = {0, 0, 0};
    hipLaunchKernelGGL(k_amg_hashvec, dim3(gn(n)), bv, 0, st, n, L.dinv.p, x);
    const int np = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (n + 4095) / 4096));
    double lam = 0.0;
    for (int pi = 0; pi < 15; ++pi) {
        hipLaunchKernelGGL(k_amg_dax, dim3(gn(n)), bv, 0, st, n, L.rp, L.ci, L.a, L.dinv.p, x, y);
        fixed_dots(st, n, np, x, x, y, y, nullptr, nullptr, L.part.p, L.sc.p);
        HIPCHK(c, hipMemcpyAsync(h, L.sc.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (!(h[0] > 0.0) || !std::isfinite(h[1])) break;
        lam = std::sqrt(h[1] / h[0]);
        if (!(h[1] > 0.0)) break;
        hipLaunchKernelGGL(k_amg_scale, dim3(gn(n)), bv, 0, st, n, y, 1.0 / std::sqrt(h[1]), x);
    }
    HIPCHK(c, hipMemsetAsync(L.sc.p, 0, 8 * sizeof(double), st));
    L.om = lam > 0.0 && std::isfinite(lam) ? 1.5 / lam : 0.0;
    return FDAPDE_OK;
}
}   // namespace

bool amg_eligible(const fdapde_ctx* c) {
    return c->has_device && c->dev_ready && c->comm == nullptr && c->ar_fn == nullptr && !c->halo_ready && !c->rd.ready && !c->group;
}

void amg_release(fdapde_ctx* c) {
    if (c->has_device) (void)hipSetDevice(c->device);
    delete c->amg;
    delete c->amg_lin;
    c->amg = c->amg_lin = nullptr;
}

namespace {
// the scalar cycle's launches: damped Jacobi (L.om D^-1) as the smoother
void scalar_pre_restrict(hipStream_t st, int Q, AmgLevel& L, AmgLevel& N, const double* r, double* rc, int64_t rs, int64_t cs) {
    by_team_cols<4>(L.team, Q, [&](auto t, auto q) {
        constexpr int T = decltype(t)::value, QC = decltype(q)::value;
        hipLaunchKernelGGL((k_amg_pre_restrict<T, QC>), dim3(gn(N.n * T)), dim3(256), 0, st, N.n, L.mptr.p, L.midx.p, L.rp, L.ci, L.a, L.dinv.p, L.om, r, L.zt.p, rc, rs, cs);
    });
}
void scalar_post(hipStream_t st, int Q, AmgLevel& L, AmgLevel& N, const double* r, double* out) {
    by_team_cols<4>(L.team, Q, [&](auto t, auto q) {
        constexpr int T = decltype(t)::value, QC = decltype(q)::value;
        hipLaunchKernelGGL((k_amg_post<T, QC>), dim3(gn(L.n * T)), dim3(256), 0, st, L.n, L.rp, L.ci, L.a, L.dinv.p, L.om, L.agg.p, N.e.p, r, L.zt.p, out);
    });
}
void scalar_spmv_dots(hipStream_t st, int Q, AmgLevel& L, const double* x, double* y, const double* p0, const double* q0, const double* p1, const double* q1,
                      const double* p2, const double* q2) {
    by_team_cols<4>(L.team, Q, [&](auto t, auto q) {
        constexpr int T = decltype(t)::value, QC = decltype(q)::value;
        hipLaunchKernelGGL((k_amg_spmv_dots<T, QC>), dim3((unsigned)L.np), dim3(256), 0, st, L.n, L.rp, L.ci, L.a, x, y, p0, q0, p1, q1, p2, q2, L.part.p);
    });
}
constexpr AmgCycleOps kScalarOps{scalar_pre_restrict, scalar_post, scalar_spmv_dots};

// the hierarchy of A with (absorb) or without absorption on every level; *stalled: the answer is the "coarsening stalled above the dense limit" refusal
int amg_build_pass(fdapde_ctx* c, AmgHierarchy** slot, const double* A, int use_bnd, bool symmetric, int absorb, bool* stalled) {
    *stalled = false;
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_ptr<AmgHierarchy> H(new AmgHierarchy());
    H->ops = &kScalarOps, H->sym = symmetric, H->use_bnd = use_bnd, H->A = A, H->absorbed = absorb;
    {
        std::unique_ptr<AmgLevel> L0(new AmgLevel());
        L0->n = c->hs.n_dofs, L0->nnz = c->hs.nnz, L0->rp = c->rowptr.p, L0->ci = c->colidx.p, L0->a = A, L0->excl = use_bnd ? c->bnd.p : nullptr;
        H->lv.push_back(std::move(L0));
    }
    constexpr AmgBuildWords words{
        "",
        "FDAPDE_SOLVER_AMG: coarsening stalled above the dense limit (a level kept more than 0.8 of its rows): the matrix has too few strong couplings for pairwise aggregation",
        "FDAPDE_SOLVER_AMG: a level above the dense limit has no free rows to aggregate", nullptr, nullptr, nullptr,
        "FDAPDE_SOLVER_AMG: the coarsest level is singular to working precision (a pure Neumann problem has no unique solution)"};
    if (int rc = amg_build_levels(c, *H, absorb, 0, kDenseMaxRows, words, [] { return std::unique_ptr<AmgLevel>(new AmgLevel()); }, stalled)) return rc;
    double nnz_all = 0.0;
    for (size_t l = 0; l < H->lv.size(); ++l) {
        if (int rc = level_prepare(c, *H->lv[l], l + 1 < H->lv.size())) return rc;
        nnz_all += (double)H->lv[l]->nnz;
    }
    H->op_complexity = nnz_all / std::max(1.0, (double)H->lv[0]->nnz);
    AmgLevel& C = *H->lv.back();
    const int dense_bnd = H->lv.size() == 1 ? use_bnd : 0;
    if (int rc = dense_build_csr(c, C.n, C.rp, C.ci, C.a, dense_bnd ? c->bnd.p : nullptr, dense_bnd, H->D)) return rc;
    if (!H->D.ready) return fail(c, FDAPDE_ENOCONV, words.coarsest_singular);
    H->setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *slot = H.release();
    return FDAPDE_OK;
}
}   // namespace

// the hierarchy of A (the context's pattern, internal order); use_bnd: level 0's Dirichlet DOFs (c->bnd) belong to no aggregate.  Knob amg_absorb: amg_build_retry
int amg_build(fdapde_ctx* c, AmgHierarchy** slot, const double* A, int use_bnd, bool symmetric) {
    return amg_build_retry(c, slot, [&](int absorb, bool* stalled) { return amg_build_pass(c, slot, A, use_bnd, symmetric, absorb, stalled); });
}

// fdapde_amg_cols_trace: since the hierarchy was built, the Q-column runs, the columns they took and the columns solved one by one
int amg_cols_trace(const AmgHierarchy* H, int32_t* batches, int32_t* batched_cols, int32_t* single_cols) {
    if (!H) return FDAPDE_ENOTINIT;
    if (batches) *batches = (int32_t)H->batches;
    if (batched_cols) *batched_cols = (int32_t)H->batched_cols;
    if (single_cols) *single_cols = (int32_t)H->single_cols;
    return FDAPDE_OK;
}

// (a hierarchy fdapde_lin_compute has outlived is not live: the next solve builds the new matrix's, and its trace starts at zero)
const AmgHierarchy* amg_lin_live(const fdapde_ctx* c) { return c->amg_lin && c->amg_lin->key == c->amg_lin_epoch ? c->amg_lin : nullptr; }
int amg_lin_cols_trace(const fdapde_ctx* c, int32_t* batches, int32_t* batched_cols, int32_t* single_cols) {
    return amg_cols_trace(amg_lin_live(c), batches, batched_cols, single_cols);
}

// fdapde_amg_hierarchy: rows and entries per level, counted in scalar unknowns (H->per of them to a node)
int amg_describe(const AmgHierarchy* H, int32_t cap, int32_t* n_levels, int64_t* rows, int64_t* nnz, int32_t* absorbed, double* setup_ms) {
    if (!H) return FDAPDE_ENOTINIT;
    if (n_levels) *n_levels = (int32_t)H->lv.size();
    for (size_t l = 0; l < H->lv.size() && (int64_t)l < (int64_t)cap; ++l) {
        if (rows) rows[l] = H->per * H->lv[l]->n;
        if (nnz) nnz[l] = H->per * H->per * H->lv[l]->nnz;
    }
    if (absorbed) *absorbed = H->absorbed;
    if (setup_ms) *setup_ms = H->setup_ms;
    return FDAPDE_OK;
}

// fdapde_amg_aggregates: agg[i] = the row of level + 1 that row i of `level` belongs to, -1 for a row of no aggregate (level 0's Dirichlet rows under use_bnd);
// level 0: i in the reference DOF numbering, through dof_i2e; deeper levels in the level's own numbering.  The block form's rows are block rows.  The resident
// maps copied out, no kernel
int amg_aggregates(fdapde_ctx* c, const AmgHierarchy* H, int32_t level, int64_t cap, int32_t* agg, int64_t* n_rows) {
    if (!H) return FDAPDE_ENOTINIT;
    if (level < 0 || (size_t)level + 1 >= H->lv.size()) return FDAPDE_EINVAL;
    const AmgLevel& L = *H->lv[(size_t)level];
    if (n_rows) *n_rows = L.n;
    if (!agg || cap < L.n) return FDAPDE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> own, i2e;
    if (int rc = fetch(c, L.agg.p, (size_t)L.n, own)) return rc;
    if (level > 0) {
        std::copy(own.begin(), own.end(), agg);
        return FDAPDE_OK;
    }
    if (int rc = fetch(c, c->dof_i2e.p, (size_t)L.n, i2e)) return rc;
    for (int64_t i = 0; i < L.n; ++i) agg[i2e[(size_t)i]] = own[(size_t)i];
    return FDAPDE_OK;
}

// fdapde_amg_order: order[i] = the reference DOF that row i of level 0 is (dof_i2e): the order level 0's own arithmetic runs in -- k_amg_hashvec's vector is a
// function of the row index
int amg_order(fdapde_ctx* c, const AmgHierarchy* H, int64_t cap, int32_t* order, int64_t* n_rows) {
    if (!H) return FDAPDE_ENOTINIT;
    const int64_t n = H->lv[0]->n;
    if (n_rows) *n_rows = n;
    if (!order || cap < n) return FDAPDE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(order, c->dof_i2e.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return FDAPDE_OK;
}

// fdapde_amg_damping: the smoother's damping per level as the cycle kernels take it, 0 on the last level (inverted, not smoothed)
int amg_damping(const AmgHierarchy* H, int32_t cap, int32_t* n_levels, double* omega) {
    if (!H) return FDAPDE_ENOTINIT;
    if (n_levels) *n_levels = (int32_t)H->lv.size();
    for (size_t l = 0; omega && l < H->lv.size() && (int64_t)l < (int64_t)cap; ++l) omega[l] = l + 1 < H->lv.size() ? H->lv[l]->om : 0.0;
    return FDAPDE_OK;
}

namespace {
// e_m = (level m's system)^-1 b_m approximately, for Q interleaved columns: the dense inverse on the coarsest level, two flexible CG / GCR steps around the cycle
// elsewhere.  The dots k_amg_coef reads, (p0.q0, p1.q1[, p2.q2]): flexible CG c.v, c.b then d.v, d.w, d.rt; GCR v.v, v.b then v.w, w.w, w.rt
int amg_correction(fdapde_ctx* c, AmgHierarchy& H, size_t m, int Q) {
    hipStream_t st = c->stream;
    AmgLevel& L = *H.lv[m];
    const int64_t n = H.per * L.n;
    if (m + 1 == H.lv.size()) {   // (b arrived column-major: amg_cycle)
        if (Q == 1) return dense_apply(c, H.D, 1, L.b.p, L.e.p);
        if (int rc = dense_apply(c, H.D, Q, L.b.p, L.ecm.p)) return rc;
        hipLaunchKernelGGL(k_amg_cm2il, dim3(gn(n * Q)), dim3(256), 0, st, n, Q, (const double*)L.ecm.p, L.e.p);
        return FDAPDE_OK;
    }
    double *b = L.b.p, *cv = L.cv.p, *v = L.v.p, *rt = L.rt.p, *dv = L.dv.p, *w = L.w.p;
    // step 1: c = B b, v = A c
    if (int rc = amg_cycle(c, H, m, Q, b, cv)) return rc;
    if (H.sym) H.ops->spmv_dots(st, Q, L, cv, v, cv, v, cv, b, nullptr, nullptr);
    else H.ops->spmv_dots(st, Q, L, cv, v, v, v, v, b, nullptr, nullptr);
    hipLaunchKernelGGL(k_amg_coef, dim3((unsigned)Q), dim3(256), 0, st, L.part.p, L.np, Q, 1, L.sc.p);
    by_cols(Q, [&](auto q) {
        constexpr int QC = decltype(q)::value;
        hipLaunchKernelGGL(k_amg_axpy_sc<QC>, dim3(gn(n)), dim3(256), 0, st, n, b, v, L.sc.p, rt);
    });
    // step 2: d = B rt, w = A d
    if (int rc = amg_cycle(c, H, m, Q, rt, dv)) return rc;
    if (H.sym) H.ops->spmv_dots(st, Q, L, dv, w, dv, v, dv, w, dv, rt);
    else H.ops->spmv_dots(st, Q, L, dv, w, v, w, w, w, w, rt);
    hipLaunchKernelGGL(k_amg_coef, dim3((unsigned)Q), dim3(256), 0, st, L.part.p, L.np, Q, 2, L.sc.p);
    by_cols(Q, [&](auto q) {
        constexpr int QC = decltype(q)::value;
        hipLaunchKernelGGL(k_amg_comb2<QC>, dim3(gn(n)), dim3(256), 0, st, n, cv, dv, L.sc.p, L.e.p);
    });
    return FDAPDE_OK;
}
}   // namespace

int amg_cycle(fdapde_ctx* c, AmgHierarchy& H, size_t l, int Q, const double* r, double* out) {
    AmgLevel &L = *H.lv[l], &N = *H.lv[l + 1];
    const bool dense_next = l + 2 == H.lv.size();   // the coarsest level's right-hand side goes out column-major: what dense_apply takes
    H.ops->pre_restrict(c->stream, Q, L, N, r, N.b.p, dense_next ? 1 : Q, dense_next ? H.per * N.n : 1);
    if (int rc = amg_correction(c, H, l + 1, Q)) return rc;
    H.ops->post(c->stream, Q, L, N, r, out);
    return FDAPDE_OK;
}

int amg_cols_width(int want, int64_t n_words, int mk) {
    int Q = want >= 8 ? 8 : want >= 4 ? 4 : want >= 2 ? 2 : 1;
    while (Q > 1 && (double)Q * (double)(2 * mk + 1) * (double)n_words * 8.0 > 16e9) Q /= 2;
    return Q;
}

int amg_cols_prepare(fdapde_ctx* c, AmgHierarchy& H, int Q) {
    for (size_t l = 0; l < H.lv.size(); ++l)
        if (int rc = level_width(c, *H.lv[l], H.per, l + 1 == H.lv.size(), Q)) return rc;
    return FDAPDE_OK;
}

int amg_dense_cols(fdapde_ctx* c, AmgHierarchy& H, int Q, const double* v, double* z) {
    if (Q == 1) return dense_apply(c, H.D, 1, v, z);
    AmgLevel& L = *H.lv.back();
    const int64_t nw = H.per * L.n;
    hipLaunchKernelGGL(k_amg_il2cm, dim3(gn(nw * Q)), dim3(256), 0, c->stream, nw, Q, v, L.b.p);
    if (int rc = dense_apply(c, H.D, Q, L.b.p, L.ecm.p)) return rc;
    hipLaunchKernelGGL(k_amg_cm2il, dim3(gn(nw * Q)), dim3(256), 0, c->stream, nw, Q, (const double*)L.ecm.p, z);
    return FDAPDE_OK;
}

namespace {
// One run against the hierarchy H for Q interleaved columns: K u = rhs per column (K: A with the Dirichlet rows as unit rows if use_bnd; rhs = f on the free rows,
// g on the Dirichlet rows), from x0 or from g / 0; f, g, x0, x interleaved on the device (x is written; g, x0 may be null; r: scratch).  amg_outer_cols
// (amg_setup.h) with this solver's launches: k_amg_apply_K as the product and, rhs - K x fused into it, the residual; k_amg_start as the lift of the Dirichlet
// data, whose residual the stop rule is relative to (as the two-level solver's).  amg_run is the call at Q = 1, a batch of the handle one at Q = 2, 4, 8
int amg_run_cols(fdapde_ctx* c, AmgHierarchy& H, const double* A, int Q, const uint8_t* bnd, int use_bnd, const double* f, const double* g, const double* x0, double* x,
                 double* r, double rtol, int maxit, int mk, FgmresCols& S, double* relres) {
    hipStream_t st = c->stream;
    AmgLevel& L0 = *H.lv[0];
    const int64_t n = L0.n;
    auto apply_K = [&](const double* in, const double* rhs, double* out) {   // out = K in, or (rhs given) rhs - K in
        by_team_cols<4>(L0.team, Q, [&](auto tt, auto q) {
            constexpr int T = decltype(tt)::value, QC = decltype(q)::value;
            hipLaunchKernelGGL((k_amg_apply_K<T, QC>), dim3(gn(n * T)), dim3(256), 0, st, n, L0.rp, L0.ci, A, bnd, use_bnd, in, rhs, g, out);
        });
    };
    auto residual = [&](const double* in, double* out) { apply_K(in, f, out); };
    auto start = [&](bool again) -> int {
        hipLaunchKernelGGL(k_amg_start, dim3(gn(n * Q)), dim3(256), 0, st, n, Q, bnd, use_bnd, g, again ? x0 : (const double*)nullptr, x);
        if (!again) residual(x, r);
        return FDAPDE_OK;
    };
    return amg_outer_cols(c, H, Q, mk, kAmgRunLifted, [&](const double* in, double* out) { apply_K(in, nullptr, out); }, residual, start, x0 != nullptr, x, r, rtol, maxit, S,
                          relres);
}
}   // namespace

// the single column: amg_run_cols at Q = 1 on the hierarchy's own vectors, the context's Dirichlet mask, its result and its record
int amg_run(fdapde_ctx* c, AmgHierarchy* hp, const double* A, const double* f_dev, const double* g_dev, int use_bnd, const double* x0_dev, double rtol, int maxit) {
    AmgHierarchy& H = *hp;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t n = H.lv[0]->n;
    const auto t_begin = std::chrono::steady_clock::now();
    HIPCHK(c, H.vec.alloc(2 * (size_t)n));
    double *x = H.vec.p, *r = x + n;
    FgmresCols S{};
    double true_rel = 0.0;
    if (int rc = amg_run_cols(c, H, A, 1, c->bnd.p, use_bnd, f_dev, g_dev, x0_dev, x, r, rtol, maxit, amg_restart_len(n, maxit), S, &true_rel)) return rc;
    const int it = S.it[0];
    const bool converged = S.converged[0], broke = S.broke[0];
    HIPCHK(c, c->u.alloc((size_t)n));
    HIPCHK(c, hipMemcpyAsync(c->u.p, x, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const double t_asm = c->info.t_assemble_ms;
    c->info = fdapde_info{};
    c->info.t_assemble_ms = t_asm;
    c->info.method_used = FDAPDE_SOLVER_AMG, c->info.iters = it, c->info.converged = converged ? 1 : 0, c->info.relres = true_rel, c->info.persistent = 0;
    c->info.t_solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (std::getenv("FDAPDE_DEBUG_SETUP")) {
        std::fprintf(stderr, "amg: %zu levels, rows %s, operator complexity %.3f, set-up %.2f ms, solve %.2f ms, %d iterations, true relres %.2e, absorbed %d, discarded build %.2f ms\n",
                     H.lv.size(), amg_rows_text(H).c_str(), H.op_complexity, H.setup_ms, c->info.t_solve_ms, it, true_rel, H.absorbed, H.discarded_ms);
    }
    if (!converged) {
        c->err = broke ? "FDAPDE_SOLVER_AMG: the flexible GMRES broke down" : "FDAPDE_SOLVER_AMG: maxit reached";
        return FDAPDE_ENOCONV;
    }
    return FDAPDE_OK;
}

// fdapde_solve with FDAPDE_SOLVER_AMG: the reference's row-zeroed system (fem_linear_elliptic_solver.h:38-47), its hierarchy kept while the matrix epoch and
// the Dirichlet variant stay
int e_solve_amg(fdapde_ctx* c, const fdapde_options* opt, fdapde_info* info) {
    if (!amg_eligible(c)) return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_AMG takes one-GPU contexts");
    const double rtol = (opt && opt->rtol > 0) ? opt->rtol : 1e-10;
    const int maxit = (opt && opt->maxit > 0) ? opt->maxit : 200;
    const double* A = c->vals[FDAPDE_MAT_STIFF].p;
    const int use_bnd = c->have_g ? 1 : 0;
    const int64_t key = 2 * c->init_count + use_bnd;
    if (!c->amg || c->amg->key != key || c->amg->A != A) {
        if (int rc = amg_build(c, &c->amg, A, use_bnd, c->op_symmetric)) {
            c->info = fdapde_info{};
            c->info.method_used = FDAPDE_SOLVER_AMG;
            if (info) *info = c->info;
            return rc;
        }
        c->amg->key = key;
    }
    const int rc = amg_run(c, c->amg, A, c->force.p, c->g.p, use_bnd, nullptr, rtol, maxit);
    if (rc != FDAPDE_OK && rc != FDAPDE_ENOCONV) return rc;
    c->solved = true, c->dirichlet_applied = c->have_g;
    if (info) *info = c->info;
    return rc;
}

void amg_forget(fdapde_ctx* c) {
    delete c->amg;
    c->amg = nullptr;
}

// fdapde_lin_solve with FDAPDE_SOLVER_AMG: the hierarchy of the handle's matrix (no Dirichlet reduction), built by the first solve after fdapde_lin_compute and
// shared by every later column; the columns in batches of 8, 4 and 2 side by side (amg_run_cols; knob amg_cols), a last one alone
int amg_lin_solve(fdapde_ctx* c, const fdapde_options* opt, const double* b, int32_t n_rhs, double* x, fdapde_info* info) {
    if (!amg_eligible(c)) return fail(c, FDAPDE_EUNSUPPORTED, "FDAPDE_SOLVER_AMG takes one-GPU contexts");
    const double rtol = (opt && opt->rtol > 0) ? opt->rtol : 1e-10;
    const int maxit = (opt && opt->maxit > 0) ? opt->maxit : 200;
    const int64_t n = c->hs.n_dofs;
    hipStream_t st = c->stream;
    const auto t0 = std::chrono::steady_clock::now();
    if (!c->amg_lin || c->amg_lin->key != c->amg_lin_epoch) {
        if (int rc = amg_build(c, &c->amg_lin, c->lin_mat.p, 0, c->lin_symmetric)) {
            c->info = fdapde_info{};
            c->info.method_used = FDAPDE_SOLVER_AMG;
            if (info) *info = c->info;
            return rc;
        }
        c->amg_lin->key = c->amg_lin_epoch;
    }
    c->solved = false;   // c->u is about to hold the handle's solutions, not PDE::solution()
    DBuf<double>& rhs = c->lin_rhs;
    HIPCHK(c, rhs.alloc((size_t)n));
    int total = 0, rc_all = FDAPDE_OK;
    double worst = 0.0;
    AmgHierarchy& H = *c->amg_lin;
    const int mk = amg_restart_len(n, maxit);   // (amg_run's restart length: a batch keeps it)
    for (int32_t j = 0; j < n_rhs;) {
        // batches of 8, then 4, then 2 columns (knob amg_cols: the widest; narrower where the basis budget asks for it); a last single column as before
        const int32_t left = n_rhs - j;
        const int Q = amg_cols_width(std::min<int32_t>(left, c->amg_cols), n, mk);
        if (Q > 1) {
            const size_t nq = (size_t)n * (size_t)Q;
            HIPCHK(c, H.qio.alloc(nq));
            HIPCHK(c, H.qvec.alloc(3 * nq));
            double *f = H.qvec.p, *xq = f + nq, *r = xq + nq;
            HIPCHK(c, hipMemcpyAsync(H.qio.p, b + (size_t)j * n, sizeof(double) * nq, hipMemcpyHostToDevice, st));   // (one copy per batch)
            hipLaunchKernelGGL(k_amg_gather, dim3(gn(n * Q)), dim3(256), 0, st, n, Q, c->dof_i2e.p, (const double*)H.qio.p, f);
            FgmresCols S{};
            double rel[kAmgColsMax];
            if (int rc = amg_run_cols(c, H, c->lin_mat.p, Q, nullptr, 0, f, nullptr, nullptr, xq, r, rtol, maxit, mk, S, rel)) return rc;
            ++H.batches, H.batched_cols += Q;
            for (int q = 0; q < Q; ++q) {
                bool conv = S.converged[q];
                int its = S.it[q];
                if (S.handed[q]) {   // the recurrence and the true residual disagreed: the rest of this column alone, from its iterate
                    hipLaunchKernelGGL(k_amg_col_get, dim3(gn(n)), dim3(256), 0, st, n, Q, q, (const double*)f, rhs.p);
                    hipLaunchKernelGGL(k_amg_col_get, dim3(gn(n)), dim3(256), 0, st, n, Q, q, (const double*)xq, c->tmp_e.p);
                    const int rc = amg_run(c, c->amg_lin, c->lin_mat.p, rhs.p, nullptr, 0, c->tmp_e.p, rtol, maxit - its);
                    if (rc != FDAPDE_OK && rc != FDAPDE_ENOCONV) return rc;
                    hipLaunchKernelGGL(k_amg_col_put, dim3(gn(n)), dim3(256), 0, st, n, Q, q, (const double*)c->u.p, xq);
                    conv = rc == FDAPDE_OK, its += c->info.iters, rel[q] = c->info.relres;
                    ++H.single_cols;
                }
                if (!conv) rc_all = FDAPDE_ENOCONV;
                total += its, worst = std::max(worst, rel[q]);
            }
            hipLaunchKernelGGL(k_amg_scatter, dim3(gn(n * Q)), dim3(256), 0, st, n, Q, c->dof_i2e.p, (const double*)xq, H.qio.p);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(x + (size_t)j * n, H.qio.p, sizeof(double) * nq, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            j += Q;
            continue;
        }
        ++H.single_cols;
        HIPCHK(c, hipMemcpyAsync(c->tmp_e.p, b + (size_t)j * n, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_amg_gather, dim3(gn(n)), dim3(256), 0, st, n, 1, c->dof_i2e.p, (const double*)c->tmp_e.p, rhs.p);
        const int rc = amg_run(c, c->amg_lin, c->lin_mat.p, rhs.p, nullptr, 0, nullptr, rtol, maxit);
        if (rc != FDAPDE_OK && rc != FDAPDE_ENOCONV) return rc;
        if (rc == FDAPDE_ENOCONV) rc_all = rc;
        total += c->info.iters, worst = std::max(worst, c->info.relres);
        hipLaunchKernelGGL(k_amg_scatter, dim3(gn(n)), dim3(256), 0, st, n, 1, c->dof_i2e.p, (const double*)c->u.p, c->tmp_e.p);
        HIPCHK(c, hipMemcpyAsync(x + (size_t)j * n, c->tmp_e.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));   // (tmp_e is reused by the next column)
        ++j;
    }
    const double t_asm = c->info.t_assemble_ms;
    c->info = fdapde_info{};
    c->info.t_assemble_ms = t_asm;
    c->info.iters = total, c->info.relres = worst, c->info.converged = rc_all == FDAPDE_OK ? 1 : 0, c->info.method_used = FDAPDE_SOLVER_AMG, c->info.persistent = 0;
    c->info.t_solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc_all != FDAPDE_OK) c->err = "FDAPDE_SOLVER_AMG: maxit reached in at least one column";
    if (info) *info = c->info;
    return rc_all;
}

}   // namespace fdapde_engine
