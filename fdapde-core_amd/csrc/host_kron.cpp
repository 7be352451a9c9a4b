// host_kron.cpp -- term merging of the Kronecker-sum handle (host_kron.h); plain C++, no device code (tests/cpp/kron_merge_driver.cpp runs it alone)
#include "host_kron.h"

namespace fdapde_hip {

int kron_merge_terms(int q, int n_terms, const double* const* T, const double* const* S, const double** s_out, double* tm, int32_t* band) {
    const int64_t qq = (int64_t)q * q;
    int ns = 0;
    for (int k = 0; k < n_terms; ++k) {
        int sg = 0;
        while (sg < ns && s_out[sg] != S[k]) ++sg;
        double* t = tm + (int64_t)sg * qq;
        if (sg == ns) {
            s_out[ns++] = S[k];
            for (int64_t e = 0; e < qq; ++e) t[e] = T[k][e];
        } else {
            for (int64_t e = 0; e < qq; ++e) t[e] += T[k][e];
        }
    }
    for (int r = 0; r < q; ++r) {
        int lo = q, hi = -1;
        for (int sg = 0; sg < ns; ++sg)
            for (int s = 0; s < q; ++s)
                if (tm[((int64_t)sg * q + s) * q + r] != 0.0) lo = s < lo ? s : lo, hi = s > hi ? s : hi;
        band[2 * r] = hi < 0 ? 0 : lo, band[2 * r + 1] = hi;
    }
    return ns;
}

}  // namespace fdapde_hip
