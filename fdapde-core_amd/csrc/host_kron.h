// host_kron.h -- host side of fdapde_kron_compute (eng_kron.hip): the terms T_k (x) S_k as handed over -> what the kernels of kernels_kron.h see.
#ifndef FDAPDE_HOST_KRON_H
#define FDAPDE_HOST_KRON_H

#include <cstdint>

namespace fdapde_hip {

// Terms whose S pointers are equal share one spatial factor: their T are summed (in the order handed over).  -> the number n_S of distinct factors;
// s_out[n_S]: their pointers in the order of first appearance, tm[n_S q q]: the summed time factors, column-major as given (tm[(sigma q + s) q + r] =
// T_sigma[r, s]), band[2 q]: for T-row r the first and last column s in which ANY T_sigma[r, s] is not an exact zero (an all-zero row: 0, -1).
// The caller has checked 1 <= q, 1 <= n_terms and that no pointer is NULL; s_out holds n_terms pointers, tm n_terms q q doubles.
int kron_merge_terms(int q, int n_terms, const double* const* T, const double* const* S, const double** s_out, double* tm, int32_t* band);

}  // namespace fdapde_hip
#endif
