// host_obs.cpp -- set-up of the factored data term scale Psi^T W Psi of the 2 x 2 block handle (host_obs.h): validation, Psi in the internal DOF order,
// its transpose, and the dense stage's merged matrix.  Not the hot path: plain loops, once per fdapde_block_set_obs.
#include "host_obs.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace fdapde_hip {

bool obs_validate(int64_t n_dofs, int64_t n_obs, const int64_t* rowptr, const int32_t* colidx, const double* values, const double* weights, double scale,
                  std::string* why) {
    auto no = [&](const std::string& s) {
        if (why) *why = "fdapde_block_set_obs: " + s;
        return false;
    };
    if (!std::isfinite(scale)) return no("scale is not finite");
    if (rowptr[0] != 0) return no("rowptr[0] is not 0");
    for (int64_t k = 0; k < n_obs; ++k)
        if (rowptr[k + 1] < rowptr[k]) return no("rowptr decreases at row " + std::to_string(k));
    const int64_t nnz = rowptr[n_obs];
    if (nnz > INT32_MAX - 64) return no("more than 2^31 - 65 entries");
    if (nnz > 0 && (!colidx || !values)) return no("colidx / values are NULL");
    for (int64_t k = 0; k < n_obs; ++k) {
        for (int64_t e = rowptr[k]; e < rowptr[k + 1]; ++e) {
            if (colidx[e] < 0 || colidx[e] >= n_dofs)
                return no("row " + std::to_string(k) + " names column " + std::to_string(colidx[e]) + ", outside [0, n_dofs)");
            if (e > rowptr[k] && colidx[e] <= colidx[e - 1]) return no("the columns of row " + std::to_string(k) + " are not strictly ascending");
            if (!std::isfinite(values[e])) return no("row " + std::to_string(k) + " holds a value that is not finite");
        }
        if (weights && !std::isfinite(weights[k])) return no("weight " + std::to_string(k) + " is not finite");
    }
    return true;
}

void obs_build(int64_t n_dofs, int64_t n_obs, const int64_t* rowptr, const int32_t* colidx, const double* values, const double* weights,
               const int32_t* dof_e2i, ObsHost* out) {
    ObsHost& P = *out;
    const int64_t nnz = rowptr[n_obs];
    P.n_obs = n_obs, P.n = n_dofs, P.nnz = nnz, P.longest_row = 0, P.longest_col = 0;
    P.rp.resize((size_t)n_obs + 1), P.ci.resize((size_t)nnz), P.v.resize((size_t)nnz);
    P.w.assign((size_t)n_obs, 1.0);
    if (weights) std::copy(weights, weights + n_obs, P.w.begin());
    std::vector<std::pair<int32_t, double>> row;
    for (int64_t k = 0; k < n_obs; ++k) {
        const int64_t rs = rowptr[k], re = rowptr[k + 1];
        P.rp[k] = (int32_t)rs;
        row.clear();
        for (int64_t e = rs; e < re; ++e) row.emplace_back(dof_e2i[colidx[e]], values[e]);
        std::sort(row.begin(), row.end(), [](const auto& a, const auto& b) { return a.first < b.first; });   // (the columns of a row are distinct)
        for (int64_t e = rs; e < re; ++e) P.ci[e] = row[e - rs].first, P.v[e] = row[e - rs].second;
        P.longest_row = std::max<int32_t>(P.longest_row, (int32_t)(re - rs));
    }
    P.rp[n_obs] = (int32_t)nnz;
    // the transpose by counting: rows visited in ascending order, so a row of Psi^T lists its observations ascending
    P.trp.assign((size_t)n_dofs + 1, 0), P.tci.resize((size_t)nnz), P.tv.resize((size_t)nnz);
    for (int64_t e = 0; e < nnz; ++e) ++P.trp[P.ci[e] + 1];
    for (int64_t i = 0; i < n_dofs; ++i) {
        P.longest_col = std::max(P.longest_col, P.trp[i + 1]);
        P.trp[i + 1] += P.trp[i];
    }
    std::vector<int32_t> at(P.trp.begin(), P.trp.end() - 1);
    for (int64_t k = 0; k < n_obs; ++k)
        for (int32_t e = P.rp[k]; e < P.rp[k + 1]; ++e) {
            const int32_t s = at[P.ci[e]]++;
            P.tci[s] = (int32_t)k, P.tv[s] = P.v[e];
        }
}

void obs_coarsen(const ObsHost& fine, const int32_t* agg, int64_t n_coarse, ObsHost* out) {
    ObsHost& P = *out;
    P.n_obs = fine.n_obs, P.n = n_coarse, P.longest_row = 0, P.longest_col = 0;
    P.w = fine.w;
    P.rp.assign((size_t)fine.n_obs + 1, 0), P.ci.clear(), P.v.clear();
    std::vector<double> acc((size_t)n_coarse, 0.0);
    std::vector<uint8_t> seen((size_t)n_coarse, 0);
    std::vector<int32_t> touched;
    for (int64_t k = 0; k < fine.n_obs; ++k) {
        touched.clear();
        for (int32_t e = fine.rp[k]; e < fine.rp[k + 1]; ++e) {   // (ascending fine columns: the order of every sum)
            const int32_t j = agg[fine.ci[e]];
            if (!seen[j]) seen[j] = 1, touched.push_back(j);
            acc[j] += fine.v[e];
        }
        std::sort(touched.begin(), touched.end());
        for (int32_t j : touched) P.ci.push_back(j), P.v.push_back(acc[j]), acc[j] = 0.0, seen[j] = 0;
        P.rp[k + 1] = (int32_t)P.ci.size();
        P.longest_row = std::max<int32_t>(P.longest_row, (int32_t)touched.size());
    }
    P.nnz = (int64_t)P.ci.size();
    P.trp.assign((size_t)n_coarse + 1, 0), P.tci.resize((size_t)P.nnz), P.tv.resize((size_t)P.nnz);
    for (int64_t e = 0; e < P.nnz; ++e) ++P.trp[P.ci[e] + 1];
    for (int64_t i = 0; i < n_coarse; ++i) {
        P.longest_col = std::max(P.longest_col, P.trp[i + 1]);
        P.trp[i + 1] += P.trp[i];
    }
    std::vector<int32_t> at(P.trp.begin(), P.trp.end() - 1);
    for (int64_t k = 0; k < P.n_obs; ++k)
        for (int32_t e = P.rp[k]; e < P.rp[k + 1]; ++e) {
            const int32_t s = at[P.ci[e]]++;
            P.tci[s] = (int32_t)k, P.tv[s] = P.v[e];
        }
}

int obs_team_width(int64_t rows, int64_t nnz, int knob) {
    if (knob == 8 || knob == 64) return knob;
    return nnz > 16 * rows ? 64 : 8;
}

void obs_merge_dense(const int32_t* rowptr, const int32_t* colidx, const double* raw, const ObsHost& P, double scale, std::vector<int32_t>* rowptr2,
                     std::vector<int32_t>* colidx2, std::vector<double>* val2) {
    const int64_t n = P.n;
    rowptr2->assign((size_t)(2 * n + 1), 0), colidx2->clear(), val2->clear();
    std::vector<double> acc((size_t)n, 0.0);   // row i of Psi^T W Psi, dense
    std::vector<uint8_t> seen((size_t)n, 0);
    std::vector<int32_t> touched;
    for (int64_t i = 0; i < n; ++i) {
        touched.clear();
        for (int32_t s = P.trp[i]; s < P.trp[i + 1]; ++s) {
            const int32_t k = P.tci[s];
            const double f = P.w[k] * P.tv[s];
            for (int32_t e = P.rp[k]; e < P.rp[k + 1]; ++e) {
                const int32_t j = P.ci[e];
                if (!seen[j]) seen[j] = 1, touched.push_back(j);
                acc[j] += f * P.v[e];
            }
        }
        std::sort(touched.begin(), touched.end());
        // row 2 i: the union of the pattern row and the term's row
        int32_t k = rowptr[i];
        const int32_t k1 = rowptr[i + 1];
        size_t t = 0;
        while (k < k1 || t < touched.size()) {
            const int32_t jp = k < k1 ? colidx[k] : INT32_MAX, jt = t < touched.size() ? touched[t] : INT32_MAX;
            const int32_t j = std::min(jp, jt);
            const bool on_pattern = jp == j;
            double a11 = 0.0, a12 = 0.0;
            if (on_pattern) a11 = raw[4 * (int64_t)k], a12 = raw[4 * (int64_t)k + 1], ++k;
            if (jt == j) a11 += scale * acc[j], ++t;
            colidx2->push_back(2 * j), val2->push_back(a11);
            if (on_pattern) colidx2->push_back(2 * j + 1), val2->push_back(a12);   // (an entry off the pattern has no a12)
        }
        (*rowptr2)[2 * i + 1] = (int32_t)colidx2->size();
        for (k = rowptr[i]; k < k1; ++k) {   // row 2 i + 1: the pattern row as it is
            colidx2->push_back(2 * colidx[k]), val2->push_back(raw[4 * (int64_t)k + 2]);
            colidx2->push_back(2 * colidx[k] + 1), val2->push_back(raw[4 * (int64_t)k + 3]);
        }
        (*rowptr2)[2 * i + 2] = (int32_t)colidx2->size();
        for (int32_t j : touched) acc[j] = 0.0, seen[j] = 0;
    }
}

}  // namespace fdapde_hip
