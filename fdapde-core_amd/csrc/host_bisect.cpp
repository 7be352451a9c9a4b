// host_bisect.cpp -- geometric partition of the persistent CG's interior rows (kernels_persist.h): recursive coordinate bisection instead of
// contiguous chunks of the internal (Morton) order.  Chunks of a space-filling curve are ragged unions of octree cells; boxes cut along the
// longest axis have less surface, i.e. fewer entries that cross a block boundary (kept in both rows) and fewer imported / exported vector
// entries -- the part of the per-iteration stream that is not matrix.
//   host_bisect_quantise    integer coordinates of the DOFs: the quantisation of the Morton keys (host_setup.cpp morton_order) at the
//                           resolution of the points' spacing (internal.h persist_bisect_span)
//   host_bisect_partition   the bisection: a permutation of the interior rows with every block contiguous + the blocks' row counts
//   host_build_persist_layout_bisect   the layout builder (host_persist.cpp) fed the system in the permuted numbering, its output mapped back
// Integer work only; dev_persist.hip (dev_build_persist_layout_bisect) produces the same arrays on the device (FDAPDE_SETUP_CHECK compares).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "internal.h"

namespace fdapde_hip {

void host_bisect_quantise(int N, int64_t n, const double* pts_colmajor, const int32_t* i2e, double span, std::vector<uint32_t>& q) {
    q.assign((size_t)3 * (size_t)n, 0u);
    if (n < 1) return;
    for (int d = 0; d < N && d < 3; ++d) {
        const double* x = pts_colmajor + (int64_t)d * n;
        double lo = x[0], hi = x[0];
        for (int64_t i = 1; i < n; ++i) lo = std::min(lo, x[i]), hi = std::max(hi, x[i]);
        for (int64_t i = 0; i < n; ++i) {
            const double p = x[i2e ? i2e[(size_t)i] : i];
            const double w = hi > lo ? (p - lo) / (hi - lo) : 0.0;
            q[(size_t)d * (size_t)n + (size_t)i] = (uint32_t)std::llround(std::min(1.0, std::max(0.0, w)) * span);
        }
    }
}

int host_bisect_partition(int64_t n_int, const int32_t* cost, const uint32_t* qx, const uint32_t* qy, const uint32_t* qz, int G, std::vector<int32_t>& perm,
                          std::vector<int32_t>& block_rows) {
    if (G < 1 || n_int < (int64_t)G) return FDAPDE_EUNSUPPORTED;
    const uint32_t* q[3] = {qx, qy, qz};
    perm.resize((size_t)n_int);
    std::iota(perm.begin(), perm.end(), 0);
    std::vector<int32_t> segb{0, (int32_t)n_int}, segg{G};   // segments in position order: bounds, workgroups they hold
    std::vector<int64_t> pre;
    while (*std::max_element(segg.begin(), segg.end()) > 1) {
        std::vector<int32_t> nb{0}, ng;
        for (size_t s = 0; s < segg.size(); ++s) {
            const int32_t b = segb[s], e = segb[s + 1], g = segg[s];
            if (g == 1) {   // settled: its rows keep their order
                nb.push_back(e), ng.push_back(1);
                continue;
            }
            int axis = 0;   // largest extent, ties to the lowest axis
            uint32_t best = 0;
            for (int d = 0; d < 3; ++d) {
                uint32_t lo = 0xffffffffu, hi = 0;
                for (int32_t p = b; p < e; ++p) lo = std::min(lo, q[d][(size_t)perm[(size_t)p]]), hi = std::max(hi, q[d][(size_t)perm[(size_t)p]]);
                if (hi - lo > best) best = hi - lo, axis = d;
            }
            const uint32_t* qa = q[axis];
            std::stable_sort(perm.begin() + b, perm.begin() + e, [qa](int32_t a, int32_t c) { return qa[(size_t)a] < qa[(size_t)c]; });
            pre.resize((size_t)(e - b) + 1);
            pre[0] = 0;
            for (int32_t p = b; p < e; ++p) pre[(size_t)(p - b) + 1] = pre[(size_t)(p - b)] + cost[(size_t)perm[(size_t)p]];
            const int32_t gl = g / 2, gr = g - gl;
            const int64_t share = pre[(size_t)(e - b)] * gl / g;
            // the first row whose exclusive cost prefix reaches the share starts the right half; neither half with fewer rows than workgroups
            int32_t split = b + (int32_t)(std::lower_bound(pre.begin(), pre.begin() + (e - b), share) - pre.begin());
            split = std::max(b + gl, std::min(e - gr, split));
            nb.push_back(split), ng.push_back(gl), nb.push_back(e), ng.push_back(gr);
        }
        segb.swap(nb), segg.swap(ng);
    }
    block_rows.resize((size_t)G);
    for (int g = 0; g < G; ++g) block_rows[(size_t)g] = segb[(size_t)g + 1] - segb[(size_t)g];
    return FDAPDE_OK;
}

int host_build_persist_layout_bisect(const HostSpace& hs, bool use_bnd, int G, int lds_entries, PersistLayout& pl, int sym_mode, const uint32_t* q,
                                     std::vector<int32_t>* perm_out, std::vector<int32_t>* rows_out) {
    const int64_t nd = hs.n_dofs;
    auto dropped = [&](int64_t d) { return use_bnd && hs.dof_bnd_i[(size_t)d] != 0; };
    // interior rows in internal order, their cost (kept entries + 2) and integer coordinates
    std::vector<int32_t> irow_dof, cost;
    std::vector<uint32_t> qi[3];
    for (int64_t d = 0; d < nd; ++d) {
        if (dropped(d)) continue;
        int32_t len = 0;
        for (int32_t k = hs.rowptr_i[(size_t)d]; k < hs.rowptr_i[(size_t)d + 1]; ++k) {
            const int32_t c = hs.colidx_i[(size_t)k];
            len += c != d && !dropped(c);
        }
        irow_dof.push_back((int32_t)d), cost.push_back(len + 2);
        for (int a = 0; a < 3; ++a) qi[a].push_back(q[(size_t)a * (size_t)nd + (size_t)d]);
    }
    const int64_t n_int = (int64_t)irow_dof.size();
    std::vector<int32_t> perm, rows;
    if (int rc = host_bisect_partition(n_int, cost.data(), qi[0].data(), qi[1].data(), qi[2].data(), G, perm, rows)) return rc;
    // the permuted numbering: interior rows in partition order, the dropped ones behind them in internal order
    std::vector<int32_t> old_of_new((size_t)nd), new_of_old((size_t)nd);
    for (int64_t p = 0; p < n_int; ++p) old_of_new[(size_t)p] = irow_dof[(size_t)perm[(size_t)p]];
    {
        int64_t p = n_int;
        for (int64_t d = 0; d < nd; ++d)
            if (dropped(d)) old_of_new[(size_t)p++] = (int32_t)d;
    }
    for (int64_t p = 0; p < nd; ++p) new_of_old[(size_t)old_of_new[(size_t)p]] = (int32_t)p;
    HostSpace hp;
    hp.n_dofs = nd, hp.nnz = hs.nnz, hp.max_row = hs.max_row;
    hp.dof_bnd_i.assign((size_t)nd, 0);
    for (int64_t p = n_int; p < nd; ++p) hp.dof_bnd_i[(size_t)p] = 1;
    hp.rowptr_i.resize((size_t)nd + 1);
    hp.colidx_i.resize((size_t)hs.nnz + 2);
    hp.colidx_i[(size_t)hs.nnz] = hp.colidx_i[(size_t)hs.nnz + 1] = 0;
    std::vector<int32_t> src((size_t)hs.nnz);   // entry of the permuted pattern -> entry of the real one
    hp.rowptr_i[0] = 0;
    std::vector<std::pair<int32_t, int32_t>> row;
    for (int64_t p = 0; p < nd; ++p) {
        const int32_t d = old_of_new[(size_t)p];
        row.clear();
        for (int32_t k = hs.rowptr_i[(size_t)d]; k < hs.rowptr_i[(size_t)d + 1]; ++k) row.push_back({new_of_old[(size_t)hs.colidx_i[(size_t)k]], k});
        std::sort(row.begin(), row.end());
        int32_t at = hp.rowptr_i[(size_t)p];
        for (const auto& e : row) hp.colidx_i[(size_t)at] = e.first, src[(size_t)at] = e.second, ++at;
        hp.rowptr_i[(size_t)p + 1] = at;
    }
    if (int rc = host_build_persist_layout(hp, true, G, lds_entries, pl, rows.data(), sym_mode, false)) return rc;
    for (int32_t& d : pl.slot_dof)
        if (d >= 0) d = old_of_new[(size_t)d];
    for (int32_t& k : pl.ell_src)
        if (k >= 0) k = src[(size_t)k];
    if (perm_out) *perm_out = std::move(perm);
    if (rows_out) *rows_out = std::move(rows);
    return FDAPDE_OK;
}

}  // namespace fdapde_hip
