// kernels_spmv.h -- CSR SpMV fused with the Krylov dot products (k_spmv_team2); see kernels.h
#ifndef FDAPDE_KERNELS_SPMV_H
#define FDAPDE_KERNELS_SPMV_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "internal.h"
#include "kernels_reduce.h"

namespace fdapde_hip {

// ---------------------------------------------------------------------------------------------------------------
// CSR SpMV fused with the partial dot products of the Krylov solvers: y = A x and the partials of dot(w, y) with w = x (CG's
// p.Ap) or w = a second vector (BiCGStab's r0.v, t.s) and of dot(y, y) or dot(w, w).
// Grid = 8 * BPX workgroups; workgroup b serves the rows of band (b % 8): workgroups that share an XCD (and its 4 MiB L2) work
// on one contiguous eighth of the rows, so the x entries they gather stay in that L2.
// Algorithmic HBM bytes per launch: 12 nnz + 4 (n+1) + 16 n   (BASELINE.md).
// ---------------------------------------------------------------------------------------------------------------
struct SpmvArgs {
    const int32_t* rowptr;
    const int32_t* colidx;
    const double* vals;
    const double* x;
    double* y;
    int32_t nnz;
    const double* w;       // second vector of the fused dot products; nullptr: no dots
    double* partial;       // [2 * gridDim.x]: workgroup b writes (w.y, y.y) at 2b, 2b+1; nullptr: no dots
    const int32_t* stop;   // device flag: nonzero -> converged, kernel returns immediately (may be nullptr)
    int32_t unit_diag;     // compact solver matrix: the (dropped) diagonal is 1, y_i = x_i + sum of the stored entries
    int32_t dot2_ww;       // second fused dot: 0 -> y.y (BiCGStab's t.t), 1 -> w.w over owned rows (single-reduction CG's r.r)
    const uint8_t* owned;  // multi-GPU: rows this rank counts in w.w (nullptr = all)
    const uint16_t* col16; // 16-bit column codes (window << 14 | offset) of the pattern, or nullptr   (host_build_col16)
    const int32_t* tbase;  // four window bases per group of 32 rows; tbase[4 g] < 0: wide group, read colidx instead
    const int32_t* vrow;   // segmented pattern (host_build_solver_pattern_seg): (row, chunk | n_chunks << 8) per virtual row
    int32_t n_cols;        // number of columns = length of x (the row count the kernels get may be the virtual one)
};
__device__ __forceinline__ double spmv_dot2(const SpmvArgs& s, int64_t row, double wv, double out) {
    if (!s.dot2_ww) return out * out;
    return (s.owned && !s.owned[row]) ? 0.0 : wv * wv;
}

// Team form: T lanes per row, T = the power of two whose 2 T entries cover the mean row length, U rows per team in flight.
// Consecutive teams take consecutive rows, so every val / colidx load instruction of a wavefront covers one contiguous range of
// the CSR arrays (64/T rows); there is no LDS staging of the matrix and no barrier, each lane keeps U independent load -> gather
// chains in flight.  The in-team tree sum is a fixed order: results are bitwise reproducible run to run.
// Every lane takes two consecutive entries: every val load instruction is 16 B per lane (1 KiB per wavefront, the widest global
// access), every colidx load 8 B per lane.  T lanes cover 2 T entries of a row per pass.  A row's lane pairs start at the even
// index rs & ~1, so that every pair is one 16-byte-aligned val load and one 8-byte-aligned colidx load (the entry below rs, if
// any, belongs to the previous row and is masked).  The CSR value / index arrays carry two padding entries so that the pair load
// of a row's last odd entry stays in bounds.
typedef double v2f64_t __attribute__((ext_vector_type(2)));
typedef int v2i32_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) volatile double lds_vf64_t;
struct __attribute__((packed, aligned(8))) F64x2 { double x, y; };
struct __attribute__((packed, aligned(4))) I32x2 { int x, y; };

// The instantiation flags, each selected by a size, a pattern or the platform (launch_spmv):
//   C16   the columns come as 16-bit codes, two per 4-byte load, decoded with the four window bases of the 32-row group when the
//         gathers are issued: 2 instead of 4 index bytes per entry
//   DIST  multi-GPU: the implicit unit diagonal is owner-masked, the ownership byte is loaded unconditionally with the gathers
//   WX    the dot operand IS x (CG's p.Ap): one row load serves the dot and the diagonal
//   VROWS the CSR rows are the chunks ("virtual rows") of a segmented pattern; the chunks of a row sit in one tile and are added up
//         after the LDS transpose, every chunk lane storing the row's total to the row's y (same value, same address)
//   NTV   nontemporal value stream for teams of <= 8 lanes on large matrices (see load_pair; wider teams always have it)
template <int T, int U, bool C16, bool DIST, bool WX, bool VROWS = false, bool NTV = false>
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_spmv_team2(SpmvArgs s, int64_t n,
                                                                                            int64_t rows_per_band) {
    constexpr int TEAMS = 64 / T;
    constexpr int WROWS = TEAMS * U;
    static_assert(WROWS < 64, "one rowptr load per tile");
    __shared__ double red[8];
    __shared__ double ystage[4][WROWS];
    static_assert(!C16 || 32 % WROWS == 0, "16-bit column codes need tiles inside a 32-row group");
    static_assert(!VROWS || C16, "segmented patterns always come with column codes");
    static_assert(!NTV || (C16 && T <= 8), "the value-stream switch exists for coded matrices and teams of <= 8 lanes");
    if (s.stop && __syncthreads_or(*s.stop != 0)) return;
    const int band = blockIdx.x & 7, lb = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, team = lane / T, l = lane % T;
    // Tiles are dealt round-robin to the wavefronts of a band, so that at any moment the wavefronts of an XCD read one
    // advancing window of the CSR arrays.  (Giving every wavefront its own contiguous share of rows balances the tail
    // better but measured 9 % slower at C3 size, 81.7 vs 74.8 us: thousands of independent address streams.)
    const int64_t band_begin = band * rows_per_band;
    const int64_t band_end = min(n, band_begin + rows_per_band);
    const int64_t stride = (int64_t)bpx * 4 * WROWS;
    double d_wy = 0, d_yy = 0;
    const int last = s.nnz - 1;
    // row pointers: ONE coalesced load of the tile's WROWS + 1 pointers, shuffled to the teams (8 ds_bpermute per tile).
    // Loading them per (tile, u) with team-uniform 8-byte loads instead was measured slower (79.5 vs 66.0 us): every
    // extra vector-memory instruction costs address-processing time whatever its footprint.
    auto load_rp = [&](int64_t base) -> int {
        const int64_t r = base + lane;
        return s.rowptr[r < band_end ? r : band_end];
    };
    auto load_pair = [&](int rs, int re, F64x2& v, I32x2& c) {
        const int k = (rs & ~1) + 2 * l;
        const int kc = k < last ? k : (last & ~1);
        F64x2 vv;
        I32x2 cc;
        // Cache policy of the matrix stream: DEFAULT.  A wavefront's val / code load covers 8 rows, i.e. pieces of 128-byte lines
        // that the next load of the same wavefront (the next 8 rows) completes; with the nontemporal hint the lines are not kept
        // and get fetched again (C3, same box: both nontemporal 58.2 us, codes default 52.0, values default 45.2, both 45.3 us
        // back-to-back; inside CG 40.6 / 37.3 / 33.9 / 32.7 ms per solve).
        // Teams of 16+ lanes (rows of 32+ entries, P2) read whole lines per row and keep the hint (C5-size matrix, same box: both
        // nontemporal 361.6 us, both default 371.5 us).
        constexpr bool NT_V = NTV || T >= 16, NT_C = T >= 16;
        if constexpr (C16) {
            // Large matrices -- the x / y slices of a row band no longer fit the XCD's L2 next to a default-policy value stream --
            // are launched with the hint on the values only (NTV: 2.5 M rows 88.5 -> 76.9 us; C3 45.3 -> 52.0 us).  A
            // run-time switch between the two loads does not survive the optimiser (the loads are merged and the hint dropped).
            v2f64_t a;
            if constexpr (NT_V)
                a = __builtin_nontemporal_load(reinterpret_cast<const v2f64_t*>(s.vals + kc));
            else
                a = *reinterpret_cast<const v2f64_t*>(s.vals + kc);
            vv.x = a.x, vv.y = a.y;
            if constexpr (NT_C)
                cc.x = (int)__builtin_nontemporal_load(reinterpret_cast<const unsigned int*>(s.col16 + kc)), cc.y = 0;
            else
                cc.x = (int)*reinterpret_cast<const unsigned int*>(s.col16 + kc), cc.y = 0;
        } else {
            const v2f64_t a = *reinterpret_cast<const v2f64_t*>(s.vals + kc);
            const v2i32_t b = *reinterpret_cast<const v2i32_t*>(s.colidx + kc);
            vv.x = a.x, vv.y = a.y, cc.x = b.x, cc.y = b.y;
        }
        const bool ok0 = k < re && k >= rs, ok1 = k + 1 < re;
        v.x = ok0 ? vv.x : 0.0, v.y = ok1 ? vv.y : 0.0;
        if constexpr (C16)
            c = cc;   // raw code pair; masked entries have a zero value and their decoded column is clamped into range
        else
            c.x = ok0 ? cc.x : 0, c.y = ok1 ? cc.y : 0;
    };
    // window bases of the 32-row group of a tile (wave-uniform address)
    typedef int v4i32_t __attribute__((ext_vector_type(4)));
    // the four window bases travel as ONE dword per lane (lane & 3) and are broadcast with v_readlane when the tile is decoded,
    // instead of a 16-byte load that returns the same 16 bytes to all 64 lanes (61.7 -> 61.4 us)
    auto load_tb = [&](int64_t b) -> v4i32_t {
        if constexpr (C16) {
            const int64_t bc = b < band_end ? b : band_begin;
            const int g = __builtin_amdgcn_readfirstlane((int)(bc >> 5));
            return v4i32_t{s.tbase[4 * (int64_t)g + (lane & 3)], 0, 0, 0};
        } else
            return v4i32_t{0, 0, 0, 0};
    };
    auto expand_tb = [&](const v4i32_t& t) -> v4i32_t {
        if constexpr (C16)
            return v4i32_t{__builtin_amdgcn_readlane(t.x, 0), __builtin_amdgcn_readlane(t.x, 1), __builtin_amdgcn_readlane(t.x, 2),
                           __builtin_amdgcn_readlane(t.x, 3)};
        else
            return t;
    };
    const int ncol1 = s.n_cols - 1;
    auto decode = [&](unsigned int code, const v4i32_t& tb) -> int {
        const int b01 = (code & 0x4000u) ? tb.y : tb.x, b23 = (code & 0x4000u) ? tb.w : tb.z;
        const int col = ((code & 0x8000u) ? b23 : b01) + (int)(code & 0x3fffu);
        return col < ncol1 ? col : ncol1;
    };
    auto load_vi = [&](int64_t b) -> v2i32_t {   // (row, chunk info) of this lane's virtual row in the tile at b (clamped)
        if constexpr (VROWS) {
            const int64_t v = b + (lane % WROWS);
            return *reinterpret_cast<const v2i32_t*>(s.vrow + 2 * (v < band_end ? v : band_end - 1));
        } else
            return v2i32_t{0, 0};
    };
    int64_t base = band_begin + (int64_t)(lb * 4 + wave) * WROWS;
    if (base < band_end) {
        int rp0 = load_rp(base);
        int rp1 = load_rp(base + stride);
        int rs[U], re[U];
        F64x2 v[U];
        I32x2 c[U];
        v4i32_t tb = load_tb(base);
        v2i32_t vi = load_vi(base);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            rs[u] = __shfl(rp0, u * TEAMS + team, 64), re[u] = __shfl(rp0, u * TEAMS + team + 1, 64);
            load_pair(rs[u], re[u], v[u], c[u]);
        }
        // explicit LDS address space: a volatile GENERIC pointer compiles to flat_load / flat_store, which count on vmcnt and
        // made every tile drain all of its prefetched loads (s_waitcnt vmcnt(0))
        lds_vf64_t* ys = (lds_vf64_t*)&ystage[wave][0];
        const double* wp = s.w ? s.w : s.x;   // always dereferenceable; the dots are discarded when s.w is null
        const double dots = s.w ? 1.0 : 0.0;
        // One tile.  FULL tiles (all WROWS rows inside the band) run branch-free: the w operand of the fused dot is loaded
        // WITH the gathers (a load issued after the reduction would expose a full memory latency per tile), and the y
        // store is unconditional -- lanes l >= U repeat lane l % U (same value, same address), because a store under an
        // exec-masked branch makes the next iteration's wait for the val/colidx loads a vmcnt(0) that also drains the store.
        // Both together: 66.9 -> 57.7 us in the ablation.  The band's last, partial tile takes the masked path once.
        auto tile = [&](auto full_tag) {
            constexpr bool FULL = decltype(full_tag)::value;
            double xa[U], xb[U];
            const v4i32_t tb_lane = tb;
            tb = expand_tb(tb_lane);
            if constexpr (C16) {
                if (tb.x < 0) {   // wide group (wave-uniform, rare): its columns do not fit four windows
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int k = (rs[u] & ~1) + 2 * l;
                        const v2i32_t b = *reinterpret_cast<const v2i32_t*>(s.colidx + (k < last ? k : (last & ~1)));
                        c[u].x = b.x, c[u].y = b.y;
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const unsigned int code = (unsigned int)c[u].x;
                        c[u].x = decode(code & 0xffffu, tb), c[u].y = decode(code >> 16, tb);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) xa[u] = s.x[c[u].x], xb[u] = s.x[c[u].y];
            // lane j < WROWS reports row base + j (rows are transposed into lane order through ystage below)
            const int64_t vr = base + (lane % WROWS);   // CSR (virtual) row of this lane
            const bool row_ok = FULL || vr < band_end;
            // y / x / w row of this lane: the virtual row itself, or the row it is a chunk of
            const int64_t rowc = VROWS ? (int64_t)vi.x : (row_ok ? vr : band_end - 1);
            const int64_t row = rowc;
            // implicit unit diagonal of the compact solver matrix (multi-GPU: added by the owner of the DOF only)
            double wv, xd;
            if constexpr (WX) {   // the dot operand IS x (CG: p.Ap): one row load serves the dot and the diagonal
                const double xv = s.x[rowc];
                wv = xv;
                if constexpr (DIST)
                    xd = (s.unit_diag && s.owned[rowc]) ? xv : 0.0;
                else
                    xd = s.unit_diag ? xv : 0.0;
            } else {
                wv = wp[rowc];
                if constexpr (DIST) {   // multi-GPU instantiation: ownership byte and x loaded unconditionally with the gathers
                    const uint8_t mine = s.owned[rowc];
                    const double xv = s.x[rowc];
                    xd = (s.unit_diag && mine) ? xv : 0.0;
                } else
                    xd = (s.unit_diag && !(s.owned && !s.owned[rowc])) ? s.x[rowc] : 0.0;
            }
            int rsn[U], ren[U];
            F64x2 vn[U];
            I32x2 cn[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                rsn[u] = __shfl(rp1, u * TEAMS + team, 64), ren[u] = __shfl(rp1, u * TEAMS + team + 1, 64);
                load_pair(rsn[u], ren[u], vn[u], cn[u]);
            }
            const v4i32_t tbn = load_tb(base + stride);
            const v2i32_t vin = load_vi(base + stride);
            rp1 = load_rp(base + 2 * stride);
            double acc[U];
            bool long_row = false;
#pragma unroll
            for (int u = 0; u < U; ++u)
                acc[u] = v[u].x * xa[u] + v[u].y * xb[u], long_row |= re[u] - (rs[u] & ~1) > 2 * T;
            if (__any(long_row)) {   // rows longer than a team pass: further passes of 2 T entries, all U rows at once
                int maxlen = 0;
#pragma unroll
                for (int u = 0; u < U; ++u) maxlen = max(maxlen, re[u] - (rs[u] & ~1));
                for (int off = 2 * T; __any(off < maxlen); off += 2 * T) {
                    // only lanes that still have entries issue loads (a clamped, unmasked load would fetch the next rows' data)
                    F64x2 tv[U];
                    I32x2 tc[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int k = (rs[u] & ~1) + off + 2 * l;
                        tv[u].x = tv[u].y = 0.0, tc[u].x = tc[u].y = 0;
                        if (k < re[u]) {
                            const v2f64_t a = *reinterpret_cast<const v2f64_t*>(s.vals + k);
                            tv[u].x = a.x, tv[u].y = k + 1 < re[u] ? a.y : 0.0;
                            bool coded = false;
                            if constexpr (C16) coded = tb.x >= 0;
                            if (coded) {
                                const unsigned int code = *reinterpret_cast<const unsigned int*>(s.col16 + k);
                                tc[u].x = decode(code & 0xffffu, tb), tc[u].y = decode(code >> 16, tb);
                            } else {
                                const v2i32_t b = *reinterpret_cast<const v2i32_t*>(s.colidx + k);
                                tc[u].x = b.x, tc[u].y = k + 1 < re[u] ? b.y : 0;
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int k = (rs[u] & ~1) + off + 2 * l;
                        if (k < re[u]) acc[u] += tv[u].x * s.x[tc[u].x] + tv[u].y * s.x[tc[u].y];
                    }
                }
            }
            // every lane of a team gets the team's U row sums; lane l < U keeps row (u = l, team) = tile row l*TEAMS + team.
            // Stored from there, consecutive lanes would write rows TEAMS apart: 32 separate 8-byte partial writes per
            // instruction (measured: as expensive as all the x gathers).  The sums are transposed into lane order through
            // a 256-byte per-wavefront LDS buffer (one ds_write_b64 + one ds_read_b64, wave-synchronous, no barrier), so
            // that lanes 0..WROWS-1 store WROWS consecutive rows = whole cache lines; lanes above repeat them.
            double pick = 0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double t = team_sum<T>(acc[u]);
                if (l == u) pick = t;
            }
            if (l < U) ys[l * TEAMS + team] = pick;
            __builtin_amdgcn_wave_barrier();
            double out;
            if constexpr (VROWS) {   // total of the row this lane's chunk belongs to (its chunks are adjacent in the tile)
                const int ck = vi.y & 255, cn = vi.y >> 8, j0 = (lane % WROWS) - ck;
                double t = 0;
                for (int d = 0; d < cn; ++d) t += ys[j0 + d];
                out = t + xd;
            } else
                out = ys[lane % WROWS] + xd;
            if constexpr (FULL) {
                // store flavours measured and dropped (all within noise of the plain store): nontemporal, write-through
                // (sc1), 16 bytes per lane, stores confined to 32 KiB
                s.y[row] = out;
            } else {
                if (row_ok) s.y[row] = out;
            }
            __builtin_amdgcn_wave_barrier();
            const double once = (lane < WROWS && row_ok && (!VROWS || (vi.y & 255) == 0)) ? dots : 0.0;   // each row counted by one lane
            d_wy += once * (wv * out), d_yy += once * spmv_dot2(s, rowc, wv, out);
#pragma unroll
            for (int u = 0; u < U; ++u) rs[u] = rsn[u], re[u] = ren[u], c[u] = cn[u], v[u] = vn[u];
            tb = tbn, vi = vin;
        };
        for (; base + WROWS <= band_end; base += stride) tile(std::true_type {});
        if (base < band_end) tile(std::false_type {});
    }
    if (s.partial) {
        const double a = block_sum(d_wy, red);
        const double b = block_sum(d_yy, red);
        if (threadIdx.x == 0) s.partial[2 * blockIdx.x] = a, s.partial[2 * blockIdx.x + 1] = b;
    }
}


}  // namespace fdapde_hip
#endif