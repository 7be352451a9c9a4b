// host_kron_obs.h -- host side of fdapde_kron_set_obs (eng_kron.hip): what the call refuses beyond obs_validate (host_obs.h), the weights in the order the
// kernels of kernels_kron_obs.h read them, the form rule, and the q n-row matrix of the dense stage with scale (Phi (x) Psi)^T W (Phi (x) Psi) merged in.
// Plain loops, no device.
#ifndef FDAPDE_HOST_KRON_OBS_H
#define FDAPDE_HOST_KRON_OBS_H

#include <cstdint>
#include <string>
#include <vector>

#include "host_obs.h"

namespace fdapde_hip {

constexpr int kKronObsMaxP = 64;   // rows of Phi (observation instants)

// What fdapde_kron_set_obs refuses: p outside 1 .. 64, Phi == NULL (which stands for [I_p 0]) with p > q, an entry of Phi that is not finite, one of the
// p n_obs weights that is not finite, and everything obs_validate refuses (rowptr, columns, values, scale).  -> true where the input is well formed, else
// *why says what is not.  The caller has checked n_obs >= 1 and that rowptr is not NULL; Phi and weights may be NULL.
bool kron_obs_validate(int64_t n_dofs, int32_t q, int32_t p, const double* Phi, int64_t n_obs, const int64_t* rowptr, const int32_t* colidx, const double* values,
                       const double* weights, double scale, std::string* why);

// Phi as the kernels read it: the p x q column-major copy, or [I_p 0] where Phi is NULL
void kron_obs_phi(int32_t q, int32_t p, const double* Phi, std::vector<double>* out);

// the weights as handed over (instant tau at location k at weights[tau n_obs + k], the reference's Kronecker order; NULL = ones) -> interleaved per
// observation, out[k p + tau]
void kron_obs_weights(int32_t p, int64_t n_obs, const double* weights, std::vector<double>* out);

// the power of two >= max(p, q), at least 2: the team width of the three kernels
int kron_obs_team_width(int32_t q, int32_t p);

// the form for a CSR matrix of `rows` rows and `nnz` entries: 1 = narrow (a team per row), 2 = wide (a workgroup per row).  A mean row length above 16 takes
// the wide form: the threshold of obs_team_width, inherited and not measured for these kernels.  knob kron_obs_form: 0 this rule, 1, 2.
int kron_obs_form(int64_t rows, int64_t nnz, int knob);

// The dense stage's matrix: the expanded CSR of k_kron_expand (q n rows in the stacked order r n + i, internal DOF numbering, columns ascending within a
// row) with scale sum_tau Phi[tau, r] Phi[tau, s] sum_k w[k p + tau] Psi[k, i] Psi[k, j] added at (r n + i, s n + j); entries off the pattern are inserted,
// columns ascending, the observations summed in ascending order, tau ascending.  A pair (r, s) with Phi[tau, r] Phi[tau, s] = 0 for every tau gets no entry.
// P: Psi and its transpose in the internal order (obs_build); phi: p x q column-major; w: interleaved per observation.
void kron_obs_merge_dense(int32_t q, const int32_t* rowptr, const int32_t* colidx, const double* val, const ObsHost& P, int32_t p, const double* phi,
                          const double* w, double scale, std::vector<int32_t>* rowptr2, std::vector<int32_t>* colidx2, std::vector<double>* val2);

}   // namespace fdapde_hip
#endif
