// host_kron_obs.cpp -- set-up of the factored data term scale (Phi (x) Psi)^T W (Phi (x) Psi) of the Kronecker-sum handle (host_kron_obs.h): validation, the
// weights' transposition, the form rule and the dense stage's merged matrix.  Not the hot path: plain loops, once per fdapde_kron_set_obs.
#include "host_kron_obs.h"

#include <algorithm>
#include <cmath>

namespace fdapde_hip {

bool kron_obs_validate(int64_t n_dofs, int32_t q, int32_t p, const double* Phi, int64_t n_obs, const int64_t* rowptr, const int32_t* colidx, const double* values,
                       const double* weights, double scale, std::string* why) {
    auto no = [&](const std::string& s) {
        if (why) *why = "fdapde_kron_set_obs: " + s;
        return false;
    };
    if (p < 1 || p > kKronObsMaxP) return no("p must lie in 1 .. 64");
    if (!Phi && p > q) return no("Phi == NULL stands for [I_p 0] and needs p <= q");
    if (Phi)
        for (int64_t e = 0; e < (int64_t)p * q; ++e)
            if (!std::isfinite(Phi[e])) return no("Phi holds an entry that is not finite");
    if (!obs_validate(n_dofs, n_obs, rowptr, colidx, values, nullptr, scale, why)) {
        const std::string theirs = "fdapde_block_set_obs: ";
        if (why && why->compare(0, theirs.size(), theirs) == 0) *why = "fdapde_kron_set_obs: " + why->substr(theirs.size());
        return false;
    }
    if (weights)
        for (int64_t e = 0; e < (int64_t)p * n_obs; ++e)
            if (!std::isfinite(weights[e])) return no("weight " + std::to_string(e) + " is not finite");
    return true;
}

void kron_obs_phi(int32_t q, int32_t p, const double* Phi, std::vector<double>* out) {
    out->assign((size_t)p * q, 0.0);
    if (Phi) std::copy(Phi, Phi + (size_t)p * q, out->begin());
    else
        for (int32_t t = 0; t < p; ++t) (*out)[t + (size_t)t * p] = 1.0;
}

void kron_obs_weights(int32_t p, int64_t n_obs, const double* weights, std::vector<double>* out) {
    out->assign((size_t)p * (size_t)n_obs, 1.0);
    if (!weights) return;
    for (int32_t t = 0; t < p; ++t)
        for (int64_t k = 0; k < n_obs; ++k) (*out)[(size_t)k * p + t] = weights[(size_t)t * n_obs + k];
}

int kron_obs_team_width(int32_t q, int32_t p) {
    int w = 2;
    while (w < std::max(p, q)) w *= 2;
    return w;
}

int kron_obs_form(int64_t rows, int64_t nnz, int knob) {
    if (knob == 1 || knob == 2) return knob;
    return nnz > 16 * rows ? 2 : 1;
}

void kron_obs_merge_dense(int32_t q, const int32_t* rowptr, const int32_t* colidx, const double* val, const ObsHost& P, int32_t p, const double* phi,
                          const double* w, double scale, std::vector<int32_t>* rowptr2, std::vector<int32_t>* colidx2, std::vector<double>* val2) {
    const int64_t n = P.n, nq = (int64_t)q * n;
    std::vector<uint8_t> pair_live((size_t)q * q, 0);   // (r, s): some tau has Phi[tau, r] Phi[tau, s] != 0
    for (int32_t r = 0; r < q; ++r)
        for (int32_t s = 0; s < q; ++s)
            for (int32_t t = 0; t < p; ++t)
                if (phi[t + (size_t)r * p] * phi[t + (size_t)s * p] != 0.0) pair_live[(size_t)r * q + s] = 1;
    std::vector<std::vector<int32_t>> cols((size_t)nq);
    std::vector<std::vector<double>> vals((size_t)nq);
    std::vector<double> acc((size_t)n * p, 0.0), f((size_t)p);   // acc[j p + tau] = sum_k w[k p + tau] Psi[k, i] Psi[k, j] for the DOF i at hand
    std::vector<uint8_t> seen((size_t)n, 0);
    std::vector<int32_t> touched;
    for (int64_t i = 0; i < n; ++i) {
        touched.clear();
        for (int32_t e = P.trp[i]; e < P.trp[i + 1]; ++e) {
            const int32_t k = P.tci[e];
            for (int32_t t = 0; t < p; ++t) f[t] = w[(size_t)k * p + t] * P.tv[e];
            for (int32_t o = P.rp[k]; o < P.rp[k + 1]; ++o) {
                const int32_t j = P.ci[o];
                if (!seen[j]) seen[j] = 1, touched.push_back(j);
                for (int32_t t = 0; t < p; ++t) acc[(size_t)j * p + t] += f[t] * P.v[o];
            }
        }
        std::sort(touched.begin(), touched.end());
        for (int32_t r = 0; r < q; ++r) {
            const int64_t row = (int64_t)r * n + i;
            std::vector<int32_t>& rc = cols[(size_t)row];
            std::vector<double>& rv = vals[(size_t)row];
            int32_t k = rowptr[row];
            const int32_t k1 = rowptr[row + 1];
            for (int32_t s = 0; s < q; ++s) {   // the union of the pattern row and the term's row, block column by block column
                const int64_t c0 = (int64_t)s * n, c1 = c0 + n;
                const bool live = pair_live[(size_t)r * q + s] != 0;
                size_t t = 0;
                const size_t t1 = live ? touched.size() : 0;
                while ((k < k1 && colidx[k] < c1) || t < t1) {
                    const int64_t jp = (k < k1 && colidx[k] < c1) ? colidx[k] : INT64_MAX, jt = t < t1 ? c0 + touched[t] : INT64_MAX;
                    const int64_t j = std::min(jp, jt);
                    double a = 0.0;
                    if (jp == j) a = val[k], ++k;
                    if (jt == j) {
                        const double* aj = acc.data() + (size_t)touched[t] * p;
                        double g = 0.0;
                        for (int32_t tau = 0; tau < p; ++tau) g += (phi[tau + (size_t)r * p] * phi[tau + (size_t)s * p]) * aj[tau];
                        a += scale * g, ++t;
                    }
                    rc.push_back((int32_t)j), rv.push_back(a);
                }
            }
        }
        for (int32_t j : touched) {
            seen[j] = 0;
            for (int32_t t = 0; t < p; ++t) acc[(size_t)j * p + t] = 0.0;
        }
    }
    rowptr2->assign((size_t)nq + 1, 0), colidx2->clear(), val2->clear();
    for (int64_t row = 0; row < nq; ++row) {
        colidx2->insert(colidx2->end(), cols[(size_t)row].begin(), cols[(size_t)row].end());
        val2->insert(val2->end(), vals[(size_t)row].begin(), vals[(size_t)row].end());
        (*rowptr2)[(size_t)row + 1] = (int32_t)colidx2->size();
    }
}

}   // namespace fdapde_hip
