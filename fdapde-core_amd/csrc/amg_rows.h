// amg_rows.h -- the row rules of the aggregation set-up and the host loops built on them (host_amg.cpp).  No HIP in here: the kernels of
// eng_amg.hip call the rules one thread per row, the host loops call them row after row -- what the knob amg_setup_check compares bit for bit, and what
// tests/test_host_amg.py holds to the numpy restatement without a GPU.
#ifndef FDAPDE_AMG_ROWS_H
#define FDAPDE_AMG_ROWS_H

#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define FDAPDE_AMG_RULE __host__ __device__ inline
#else
#define FDAPDE_AMG_RULE inline
#endif

namespace fdapde_engine {

constexpr double kAmgTheta = 0.25;   // strength threshold of a coupling, relative to the row's strongest
constexpr int kAmgRounds = 10;       // handshake rounds per pairwise pass ...
constexpr int kAmgStrongRounds = 3;  // ... the first of them on strong couplings only
constexpr int kMateFree = -1, kMateExcluded = -2;

// the coupling of (i, j) in the symmetric part, as a positive number for an M-matrix entry: -(a_ij + a_ji) -- a_ji looked up even where the matrix is
// symmetric (an assembled a_ji need not carry a_ij's last bit): the same word from both ends, which the matching's order of the edges relies on
FDAPDE_AMG_RULE double amg_sym_coupling(const int32_t* rp, const int32_t* ci, const double* a, int32_t k, int32_t i, int32_t j) {
    double at = 0.0;
    for (int32_t q = rp[j]; q < rp[j + 1]; ++q)
        if (ci[q] == i) {
            at = a[q];
            break;
        }
    return -(a[k] + at);
}
// sw[k] = the strength of entry k: > 0 a strong coupling, < 0 (minus its strength) a weak one, 0 none (the diagonal, excluded rows and columns)
FDAPDE_AMG_RULE void amg_strength_row(int64_t i, const int32_t* rp, const int32_t* ci, const double* a, const uint8_t* excl, double* sw) {
    const int32_t b = rp[i], e = rp[i + 1];
    if (excl && excl[i]) {
        for (int32_t k = b; k < e; ++k) sw[k] = 0.0;
        return;
    }
    double mneg = 0.0, mabs = 0.0;
    for (int32_t k = b; k < e; ++k) {
        const int32_t j = ci[k];
        if (j == (int32_t)i || (excl && excl[j])) continue;
        const double s = amg_sym_coupling(rp, ci, a, k, (int32_t)i, j);
        mneg = s > mneg ? s : mneg;
        const double sa = s < 0.0 ? -s : s;
        mabs = sa > mabs ? sa : mabs;
    }
    const bool neg = mneg > 0.0;
    const double thr = kAmgTheta * (neg ? mneg : mabs);
    for (int32_t k = b; k < e; ++k) {
        const int32_t j = ci[k];
        double w = 0.0;
        if (j != (int32_t)i && !(excl && excl[j]) && (neg || mabs > 0.0)) {
            const double s = amg_sym_coupling(rp, ci, a, k, (int32_t)i, j);
            const double v = neg ? s : (s < 0.0 ? -s : s);
            if (v > 0.0) w = v >= thr ? v : -v;   // (negative: a weak coupling, for the relaxed rounds)
        }
        sw[k] = w;
    }
}
// a tie between equally strong couplings is broken by a hash of the index pair -- the same word from both ends: a total order on the edges, so that a
// coupling that is the best of both its ends is proposed from both (breaking ties by the smaller index alone pairs almost nothing on a uniform stencil:
// every node proposes to its smallest neighbour, which proposes further down)
FDAPDE_AMG_RULE uint32_t amg_pair_hash(int32_t i, int32_t j) {
    const uint32_t lo = (uint32_t)(i < j ? i : j), hi = (uint32_t)(i < j ? j : i);
    uint64_t z = ((uint64_t)hi << 32 | lo) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 29, z *= 0xBF58476D1CE4E5B9ull, z ^= z >> 32;
    return (uint32_t)z;
}
// relaxed (the rounds from kAmgStrongRounds on): weak couplings count too -- a node whose strong neighbours have all been taken pairs along a weaker one
// instead of staying single (3-D P1 -Lap, the 250 k interior rows of unit_cube(64): strong couplings only, every round, stalled at 3 829 rows four levels down)
FDAPDE_AMG_RULE int32_t amg_propose_row(int64_t i, const int32_t* rp, const int32_t* ci, const double* sw, const int32_t* mate, int relaxed) {
    if (mate[i] != kMateFree) return -1;
    int32_t best = -1;
    double bw = 0.0;
    uint32_t bh = 0;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
        const int32_t j = ci[k];
        const double w = relaxed ? (sw[k] < 0.0 ? -sw[k] : sw[k]) : sw[k];
        if (!(w > 0.0) || j == (int32_t)i || mate[j] != kMateFree) continue;
        const uint32_t h = amg_pair_hash((int32_t)i, j);
        if (w > bw || (w == bw && (h > bh || (h == bh && j < best)))) bw = w, bh = h, best = j;
    }
    return best;
}
// absorption, after the last round (mate as it left it: no order of execution matters): a row still free picks the PAIRED neighbour it is most strongly coupled
// to -- amg_propose_row's relaxed comparison with "paired" in place of "free" -- and joins that pair's aggregate; -1: none (not free, or no paired neighbour)
FDAPDE_AMG_RULE int32_t amg_absorb_row(int64_t i, const int32_t* rp, const int32_t* ci, const double* sw, const int32_t* mate) {
    if (mate[i] != kMateFree) return -1;
    int32_t best = -1;
    double bw = 0.0;
    uint32_t bh = 0;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
        const int32_t j = ci[k];
        const double w = sw[k] < 0.0 ? -sw[k] : sw[k];
        if (!(w > 0.0) || j == (int32_t)i || mate[j] < 0) continue;
        const uint32_t h = amg_pair_hash((int32_t)i, j);
        if (w > bw || (w == bw && (h > bh || (h == bh && j < best)))) bw = w, bh = h, best = j;
    }
    return best;
}
// host: what amg_absorb_row chose per row, or NULL (a pass that does not absorb).  A row with a host leads no aggregate; hosts are paired rows: no chains
FDAPDE_AMG_RULE bool amg_leader(int64_t i, const int32_t* mate, const int32_t* host) {
    if (host && host[i] >= 0) return false;
    return mate[i] == kMateFree || (mate[i] >= 0 && (int64_t)mate[i] > i);
}
FDAPDE_AMG_RULE int32_t amg_aggregate_of(int64_t i, const int32_t* mate, const int32_t* host, const int32_t* id) {
    const int32_t m = mate[i];
    if (m == kMateExcluded) return -1;
    if (host && host[i] >= 0) {
        const int32_t h = host[i], hm = mate[h];
        return id[h < hm ? h : hm];
    }
    return amg_leader(i, mate, host) ? id[i] : id[m];
}

// ---- the host loops (host_amg.cpp): the same arithmetic in the same order as the device passes of eng_amg.hip ----
struct HostCsr {
    int64_t n = 0;
    std::vector<int32_t> rp, ci;
    std::vector<double> a;
};
// one pairwise pass (absorb: followed by the absorption of the rows it left single): agg (-1 on the rows of excl), nc aggregates
void host_pairwise(const HostCsr& A, const uint8_t* excl, int absorb, std::vector<int32_t>& agg, int32_t& nc);
// C = P^T A P of piecewise-constant P (agg): a stable key sort, every coarse entry the sum of its fine entries in ascending fine-slot order.  pay (or
// NULL): `width` further doubles per entry of A, interleaved, summed under the same keys in the same order into pay_c
void host_galerkin(const HostCsr& A, const std::vector<int32_t>& agg, int32_t nc, HostCsr& C, const double* pay = nullptr, int width = 0,
                   std::vector<double>* pay_c = nullptr);
// one level step: pass 1 on A, pass 2 on the Galerkin matrix of pass 1 (the pair graph T), the coarse matrix N of pass 2, the composite map and its members
struct HostCoarse {
    std::vector<int32_t> agg1, agg2;   // row -> pair-graph row (-1: excluded), pair-graph row -> coarse row
    int32_t n1 = 0, n2 = 0;
    HostCsr T, N;
    std::vector<double> payT, payN;    // the payload on T's and N's entries (width doubles each)
    std::vector<int32_t> agg;          // row -> coarse row (-1: excluded)
    std::vector<int32_t> mptr, midx;   // the rows of every coarse row, ascending (CSR)
};
void host_coarsen(const HostCsr& A, const uint8_t* excl, int absorb, const double* pay, int width, HostCoarse& out);

}   // namespace fdapde_engine
#endif
