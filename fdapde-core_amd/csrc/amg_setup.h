// amg_setup.h -- the set-up passes of the aggregation hierarchies (eng_amg.hip), shared by FDAPDE_SOLVER_AMG and the block form of eng_block_amg.hip:
// pairwise handshake matching (absorb: the rows it leaves single join the pair of their most strongly coupled paired neighbour -- aggregates of any size),
// the Galerkin product of piecewise-constant P, the members of every aggregate -- on the device, and as the host loops
// the knob amg_setup_check compares them with.
#ifndef FDAPDE_AMG_SETUP_H
#define FDAPDE_AMG_SETUP_H

#include <cstdint>
#include <vector>

#include "context.h"

namespace fdapde_engine {

struct AmgLevel {
    int64_t n = 0, nnz = 0;
    DBuf<int32_t> rp_own, ci_own;
    DBuf<double> a_own;
    const int32_t *rp = nullptr, *ci = nullptr;   // level 0: the context's pattern and the caller's values; below: the level's own arrays
    const double* a = nullptr;
    const uint8_t* excl = nullptr;                // rows that belong to no aggregate (level 0's Dirichlet DOFs)
    DBuf<double> dinv;
    double om = 0.0;
    int team = 4, np = 1;
    DBuf<int32_t> agg, mptr, midx;                // row -> row of the next level (-1: none); members of each next-level row, ascending
    DBuf<double> b, zt, cv, v, dv, w, rt, e, part, sc;   // work vectors (b: the restricted right-hand side; e: this level's correction)
};


struct HostCsr {
    int64_t n = 0;
    std::vector<int32_t> rp, ci;
    std::vector<double> a;
};
// what dev_galerkin sorted: entry e of the m sorted ones has key keys[e] and fine slot idx[e]; head[e] = 1 where a coarse entry starts, pos[e] its slot
struct AmgGalerkinMap {
    DBuf<uint64_t> keys;
    DBuf<int32_t> idx, head, pos;
    int64_t m = 0;
    uint64_t nc = 0;
};

void host_pairwise(const HostCsr& A, const uint8_t* excl, int absorb, std::vector<int32_t>& agg, int32_t& nc);
void host_galerkin(const HostCsr& A, const std::vector<int32_t>& agg, int32_t nc, HostCsr& C);
int dev_pairwise(fdapde_ctx* c, int64_t n, int64_t nnz, const int32_t* rp, const int32_t* ci, const double* a, const uint8_t* excl, int absorb, DBuf<int32_t>& agg,
                 int32_t* nc);
int dev_galerkin(fdapde_ctx* c, int64_t n, int64_t nnz, const int32_t* rp, const int32_t* ci, const double* a, const int32_t* agg, int32_t nc, AmgLevel& out,
                 AmgGalerkinMap* keep = nullptr);
int dev_members(fdapde_ctx* c, int64_t n, const int32_t* agg, int32_t nc, DBuf<int32_t>& mptr, DBuf<int32_t>& midx);
// the K-cycle's scalar helpers (k_amg_coef, k_amg_axpy_sc, k_amg_comb2) on vectors of any length
void amg_launch_coef(hipStream_t st, const double* part, int np, int stage, double* sc);
void amg_launch_axpy_sc(hipStream_t st, int64_t n, const double* b, const double* v, const double* sc, double* rt);
void amg_launch_comb2(hipStream_t st, int64_t n, const double* cv, const double* dv, const double* sc, double* e);

}   // namespace fdapde_engine
#endif
