// host_amg.cpp -- the aggregation set-up's level step as host loops over the row rules of amg_rows.h: what the device passes of eng_amg.hip are compared
// with bit for bit under the knob amg_setup_check, and what tests/test_host_amg.py holds to the numpy restatement.  Plain C++: no HIP, no context.
#include <algorithm>
#include <utility>

#include "amg_rows.h"

namespace fdapde_engine {

void host_pairwise(const HostCsr& A, const uint8_t* excl, int absorb, std::vector<int32_t>& agg, int32_t& nc) {
    const int64_t n = A.n;
    const int32_t *rp = A.rp.data(), *ci = A.ci.data();
    std::vector<double> sw(A.a.size());
    for (int64_t i = 0; i < n; ++i) amg_strength_row(i, rp, ci, A.a.data(), excl, sw.data());
    std::vector<int32_t> mate((size_t)n), prop((size_t)n);
    for (int64_t i = 0; i < n; ++i) mate[(size_t)i] = (excl && excl[i]) ? kMateExcluded : kMateFree;
    for (int round = 0; round < kAmgRounds; ++round) {
        for (int64_t i = 0; i < n; ++i) prop[(size_t)i] = amg_propose_row(i, rp, ci, sw.data(), mate.data(), round >= kAmgStrongRounds ? 1 : 0);
        for (int64_t i = 0; i < n; ++i) {   // mutual proposals pair
            if (mate[(size_t)i] != kMateFree) continue;
            const int32_t j = prop[(size_t)i];
            if (j >= 0 && prop[(size_t)j] == (int32_t)i) mate[(size_t)i] = j;
        }
    }
    std::vector<int32_t> host_of;
    if (absorb) {
        host_of.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) host_of[(size_t)i] = amg_absorb_row(i, rp, ci, sw.data(), mate.data());
    }
    const int32_t* host = absorb ? host_of.data() : nullptr;
    std::vector<int32_t> id((size_t)n);
    nc = 0;
    for (int64_t i = 0; i < n; ++i) {
        id[(size_t)i] = nc;
        nc += amg_leader(i, mate.data(), host) ? 1 : 0;
    }
    agg.assign((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i) agg[(size_t)i] = amg_aggregate_of(i, mate.data(), host, id.data());
}

void host_galerkin(const HostCsr& A, const std::vector<int32_t>& agg, int32_t nc, HostCsr& C, const double* pay, int width, std::vector<double>* pay_c) {
    std::vector<std::pair<uint64_t, int32_t>> ent;
    for (int64_t i = 0; i < A.n; ++i)
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k) {
            const int32_t ai = agg[(size_t)i], aj = agg[(size_t)A.ci[(size_t)k]];
            if (ai >= 0 && aj >= 0) ent.emplace_back((uint64_t)ai * (uint64_t)nc + (uint64_t)aj, k);
        }
    std::stable_sort(ent.begin(), ent.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    C.n = nc, C.rp.assign((size_t)nc + 1, 0), C.ci.clear(), C.a.clear();
    if (pay_c) pay_c->clear();
    std::vector<double> ps((size_t)(pay ? width : 0));
    for (size_t e = 0; e < ent.size();) {
        const uint64_t key = ent[e].first;
        double s = 0.0;
        std::fill(ps.begin(), ps.end(), 0.0);
        for (; e < ent.size() && ent[e].first == key; ++e) {
            s += A.a[(size_t)ent[e].second];
            for (size_t q = 0; q < ps.size(); ++q) ps[q] += pay[(size_t)width * (size_t)ent[e].second + q];
        }
        const uint64_t row = key / (uint64_t)nc;
        C.ci.push_back((int32_t)(key - row * (uint64_t)nc)), C.a.push_back(s), ++C.rp[(size_t)row + 1];
        if (pay_c) pay_c->insert(pay_c->end(), ps.begin(), ps.end());
    }
    for (int32_t r = 0; r < nc; ++r) C.rp[(size_t)r + 1] += C.rp[(size_t)r];
}

void host_coarsen(const HostCsr& A, const uint8_t* excl, int absorb, const double* pay, int width, HostCoarse& out) {
    host_pairwise(A, excl, absorb, out.agg1, out.n1);
    host_galerkin(A, out.agg1, out.n1, out.T, pay, width, &out.payT);
    host_pairwise(out.T, nullptr, absorb, out.agg2, out.n2);
    host_galerkin(out.T, out.agg2, out.n2, out.N, pay ? out.payT.data() : nullptr, width, &out.payN);
    const size_t n = (size_t)A.n, nc = (size_t)out.n2;
    out.agg.resize(n);
    for (size_t i = 0; i < n; ++i) out.agg[i] = out.agg1[i] < 0 ? -1 : out.agg2[(size_t)out.agg1[i]];
    out.mptr.assign(nc + 1, 0);
    for (size_t i = 0; i < n; ++i)
        if (out.agg[i] >= 0) ++out.mptr[(size_t)out.agg[i] + 1];
    for (size_t q = 0; q < nc; ++q) out.mptr[q + 1] += out.mptr[q];
    out.midx.resize((size_t)out.mptr[nc]);
    std::vector<int32_t> fill(out.mptr.begin(), out.mptr.end() - 1);
    for (size_t i = 0; i < n; ++i)
        if (out.agg[i] >= 0) out.midx[(size_t)fill[(size_t)out.agg[i]]++] = (int32_t)i;
}

}   // namespace fdapde_engine
