"""Reference side of FDAPDE_SOLVER_BLOCK_AMG with the factored data term carried through the hierarchy (knob block_amg_obs; tests/test_block_obs_amg_cpu.py,
tests/test_gpu_block_obs_amg.py): tests/block_amg_ref.py's restatement -- its pairwise / galerkin / cycle / fgmres, imported, not edited -- with the term
scale [Psi^T W Psi, 0; 0, 0] added to every level's matrix and to D^-1.  P = P_s (x) I_2 is piecewise constant with entries 1, so the Galerkin product of
the term is the term of Psi_{l+1} = Psi_l P_s: the same rows, the columns through the aggregates.  The aggregates are the pattern's: the term does not reach
them.  `coarse_term=False` is the control: the term on level 0 only, the coarse levels the Galerkin products of the pattern part alone."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import block_amg_ref as ba
import block_obs_ref as bo

COARSE_ROWS = ba.COARSE_ROWS
E11 = sp.csr_matrix(np.array([[1.0, 0.0], [0.0, 0.0]]))

# the areal cases of the GPU test beyond block_obs_ref.KRYLOV_CASES: (fixture, order, lambda, tiles per axis)
EXTRA_AREAL = [("unit_square_16", 1, 1e-2, 2), ("unit_square_16", 1, 1e-4, 2), ("unit_square_16", 2, 1e-2, 2), ("unit_square_16", 2, 1e-4, 2),
               ("c_shaped", 2, 1e-2, 3), ("c_shaped", 2, 1e-4, 3)]
AREAL_CASES = list(bo.KRYLOV_CASES) + EXTRA_AREAL


def budget(order):
    return ba.BUDGET_P1 if order == 1 else ba.BUDGET_P2_2D


def scalar_p(P):
    """P_s of P = P_s (x) I_2"""
    return P.tocsr()[::2, :][:, ::2].tocsr()


def coarsen(Psi, Ps):
    """Psi P_s, CSR with ascending columns (scipy's product keeps every structural entry, as obs_coarsen does)"""
    out = (Psi @ Ps).tocsr()
    out.sort_indices()
    return out


def _block_diag_inverse(A, n):
    """D^-1 of the interleaved matrix A, D its 2 x 2 diagonal blocks (the 1e-14 rule of the device)"""
    A = A.tocsr()
    i = np.arange(n)
    a, b, c, e = (np.asarray(A[2 * i + p, 2 * i + q]).ravel() for p, q in ((0, 0), (0, 1), (1, 0), (1, 1)))
    det = a * e - b * c
    mx = np.max(np.abs([a, b, c, e]), axis=0)
    assert np.all(np.abs(det) > 1e-14 * mx * mx), "a singular diagonal block"
    return ba._interleaved(np.arange(n + 1), np.arange(n), [e / det, -b / det, -c / det, a / det], n)


class Hierarchy(ba.Hierarchy):
    """block_amg_ref.Hierarchy of the pattern part, then the term beside it: self.Psi[l] per level, A[l] and D_l^-1 with the term, the last level's LU merged"""

    def __init__(self, rp, ci, blocks, n, Psi, weights=None, scale=-1.0, coarse_rows=COARSE_ROWS, coarse_term=True):
        super().__init__(rp, ci, blocks, n, coarse_rows)
        w = np.ones(Psi.shape[0]) if weights is None else np.asarray(weights, dtype=float)
        self.Psi = [Psi.tocsr()]
        for P in self.P:
            self.Psi.append(coarsen(self.Psi[-1], scalar_p(P)))
        for l in range(len(self.A)):
            if l > 0 and not coarse_term:
                break
            T = (scale * (self.Psi[l].T @ sp.diags(w) @ self.Psi[l])).tocsr()
            self.A[l] = (self.A[l] + sp.kron(T, E11, format="csr")).tocsr()
            if l < len(self.Dinv):
                self.Dinv[l] = _block_diag_inverse(self.A[l], self.rows[l] // 2)
        self.last = spl.splu(self.A[-1].tocsc())


def solve(rp, ci, blocks, n, Psi, b_stacked, weights=None, scale=-1.0, rtol=ba.RTOL, maxit=200, coarse_rows=COARSE_ROWS, coarse_term=True):
    """-> (x stacked, iterations, converged, hierarchy)"""
    H = Hierarchy(rp, ci, blocks, n, Psi, weights, scale, coarse_rows, coarse_term)
    perm = ba.stacked_to_interleaved(n)
    x, it, ok = ba.fgmres(H.A[0], np.asarray(b_stacked, dtype=float)[perm], H.precondition, rtol, maxit)
    out = np.empty(2 * n)
    out[perm] = x
    return out, it, ok, H


def levels_nnz(Psi, aggs):
    """nnz(Psi P_0 ... P_{l-1}) per level from the maps row -> row of the next level (the device's, fdapde_amg_aggregates): structural entries"""
    S = abs(Psi.sign()).tocsr()
    out = [int(S.nnz)]
    for agg in aggs:
        nc = int(agg.max()) + 1
        S = (S @ sp.csr_matrix((np.ones(len(agg)), (np.arange(len(agg)), agg)), shape=(len(agg), nc))).tocsr()
        out.append(int(S.nnz))
    return out
