// host_obs.h -- host side of fdapde_block_set_obs (eng_block.hip): the observation matrix Psi as handed over -> what the kernels of kernels_obs.h see,
// and the 2 n-row matrix of the dense stage with scale Psi^T W Psi merged in.  Plain loops, no device.
#ifndef FDAPDE_HOST_OBS_H
#define FDAPDE_HOST_OBS_H

#include <cstdint>
#include <string>
#include <vector>

namespace fdapde_hip {

// Psi (n_obs x n, CSR) in the solver's internal DOF order, its transpose and the weights: one upload each
struct ObsHost {
    int64_t n_obs = 0, n = 0, nnz = 0;
    int32_t longest_row = 0, longest_col = 0;   // the longest row of Psi / of Psi^T
    std::vector<int32_t> rp, ci;                // Psi: n_obs + 1 row starts, internal DOF ids ascending within a row
    std::vector<double> v;
    std::vector<int32_t> trp, tci;              // Psi^T: n + 1 row starts, observation ids ascending within a row
    std::vector<double> tv;
    std::vector<double> w;                      // n_obs weights (ones where none were given)
};

// What fdapde_block_set_obs refuses: a non-monotone rowptr (or one that does not start at 0, or more than 2^31 - 1 entries), a column outside [0, n_dofs), a
// row whose columns are not strictly ascending, a non-finite value, weight or scale.  -> true where the input is well formed, else *why says what is not.
// The caller has checked n_obs >= 1 and that rowptr is not NULL; colidx / values may be NULL only where rowptr[n_obs] = 0; weights may be NULL (ones).
bool obs_validate(int64_t n_dofs, int64_t n_obs, const int64_t* rowptr, const int32_t* colidx, const double* values, const double* weights, double scale,
                  std::string* why);

// validated input in the reference numbering -> ObsHost: columns through dof_e2i (n_dofs entries), every row sorted again, the transpose by counting
void obs_build(int64_t n_dofs, int64_t n_obs, const int64_t* rowptr, const int32_t* colidx, const double* values, const double* weights,
               const int32_t* dof_e2i, ObsHost* out);

// lanes per row for a CSR matrix of `rows` rows and `nnz` entries: a mean row length above 16 takes 64, otherwise 8 (knob block_obs_team: 0 this rule, 8, 64)
int obs_team_width(int64_t rows, int64_t nnz, int knob);

// Psi of the next level of an aggregation hierarchy, Psi_c = Psi P with P piecewise constant (agg[i] in [0, n_coarse): the coarse column of fine column i):
// the same n_obs rows and weights, the columns through agg, equal columns within a row summed in ascending fine-column order, columns ascending; the
// transpose by counting as obs_build does; longest_row / longest_col set.  A row may collapse to one entry, an empty row stays empty, rows are not compacted:
// Psi_l P = Psi_{l+1} holds row for row.  (Psi_c P_c)^T W (Psi_c P_c) is then the Galerkin product of the term.  out must not be &fine.
void obs_coarsen(const ObsHost& fine, const int32_t* agg, int64_t n_coarse, ObsHost* out);

// The dense stage's matrix: the block CSR (rowptr / colidx of n rows in the internal order, raw = [a11 a12 a21 a22] per entry) expanded to 2 n rows in the
// interleaved order (row 2 i + p, column 2 j + q) with scale Psi^T W Psi added to the (2 i, 2 j) entries; entries off the pattern are inserted, columns
// ascending within a row.  (Psi^T W Psi)[i, j] is summed over the observations in ascending order.
void obs_merge_dense(const int32_t* rowptr, const int32_t* colidx, const double* raw, const ObsHost& P, double scale, std::vector<int32_t>* rowptr2,
                     std::vector<int32_t>* colidx2, std::vector<double>* val2);

}  // namespace fdapde_hip
#endif
