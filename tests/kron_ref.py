"""Reference side of the Kronecker-sum tests (tests/test_kron_cpu.py, tests/test_gpu_kron.py): A = sum_k T_k (x) S_k with dense q x q time factors and
spatial factors on the FEM pattern -- the reference's Kronecker(A, B) (fdaPDE/linear_algebra/kronecker_product.h:56-80), here scipy.sparse.kron -- in the
reference's order (index r n + i for T-row r and DOF i); the space-time separable smoothing system
    [ -(I_m (x) Psi^T Psi) - lambda_T (P_t (x) R0)    lambda (M_t (x) R1^T) ]
    [  lambda (M_t (x) R1)                            lambda (M_t (x) R0)   ]
with the P1 mass and stiffness matrices of a uniform time grid on [0, 1] as M_t and P_t (the reference's spline basis is not part of this); its q x q
point-block Jacobi preconditioner (q = 2 m), and scipy's restarted GMRES(50) on the explicitly left-preconditioned system -- the iteration the device's
Krylov stage performs."""
import numpy as np
import scipy.sparse as sp

import block_ref as br

RTOL = br.RTOL
MAXIT_CAP = br.MAXIT_CAP   # the budget the GPU test hands over: a cap, not a measurement
PIVOTING_QS = [1, 2, 3, 33, 64]   # the diagonal-inverse cases (pivoting_terms on unit_square_16 P1)
# (fixture, order, m, lambda = lambda_T): the solve cases
SOLVE_CASES = [("unit_square_16", 1, 5, 1e-2), ("unit_square_16", 1, 5, 1e-4), ("unit_sphere", 1, 4, 1e-4), ("c_shaped", 2, 3, 1e-4)]


def explicit(terms, rowptr, colidx, n):
    """sum_k kron(T_k, S_k) as a CSR matrix of q n rows"""
    A = None
    for T, S in terms:
        K = sp.kron(sp.csr_matrix(np.asarray(T, dtype=float)), br.on_pattern(rowptr, colidx, S, n), format="csr")
        A = K if A is None else A + K
    A = A.tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def time_mass(m):
    """P1 mass matrix of m nodes at distance h = 1 / (m - 1) on [0, 1]: tridiagonal, SPD (m = 1, a single time instant: [[1]])"""
    if m == 1:
        return np.ones((1, 1))
    h = 1.0 / (m - 1)
    M = np.zeros((m, m))
    for e in range(m - 1):
        M[e:e + 2, e:e + 2] += h / 6.0 * np.array([[2.0, 1.0], [1.0, 2.0]])
    return M


def time_penalty(m):
    """P1 stiffness matrix of the same grid: tridiagonal, PSD (constants in its kernel; m = 1: [[0]])"""
    if m == 1:
        return np.zeros((1, 1))
    h = 1.0 / (m - 1)
    P = np.zeros((m, m))
    for e in range(m - 1):
        P[e:e + 2, e:e + 2] += 1.0 / h * np.array([[1.0, -1.0], [-1.0, 1.0]])
    return P


def _in_block(T, m, r, c):
    """the m x m time matrix T as block (r, c) of a 2 m x 2 m one"""
    out = np.zeros((2 * m, 2 * m))
    out[r * m:(r + 1) * m, c * m:(c + 1) * m] = T
    return out


def spacetime_terms(rowptr, colidx, R1, R0, obs, lam, lam_t, m):
    """-> [(T, S_values)] of the space-time smoothing system, q = 2 m, four distinct spatial factors (the two terms on R0 share one array)"""
    n = len(rowptr) - 1
    Mt, Pt = time_mass(m), time_penalty(m)
    gram = br.gram_selection_values(rowptr, colidx, obs, n)
    r1 = np.asarray(R1, dtype=float)
    r1t = br.transpose_values(rowptr, colidx, r1, n)
    r0 = np.asarray(R0, dtype=float)
    return [(_in_block(-np.eye(m), m, 0, 0), gram), (_in_block(-lam_t * Pt, m, 0, 0), r0), (_in_block(lam * Mt, m, 0, 1), r1t),
            (_in_block(lam * Mt, m, 1, 0), r1), (_in_block(lam * Mt, m, 1, 1), r0)]


def spacetime_rhs(obs, lam, n, m, seed=1):
    rng = np.random.default_rng(seed)
    b = np.zeros(2 * m * n)
    for r in range(m):
        b[r * n + obs] = -rng.standard_normal(len(obs))
        b[(m + r) * n:(m + r + 1) * n] = lam * 0.1 * rng.standard_normal(n)
    return b


def pivoting_terms(rowptr, colidx, obs, q, seed):
    """A = T_a (x) G + T_b (x) S_d: G the indicator of the observed DOFs on the diagonal, S_d = I + small random off-diagonal entries on the pattern,
    T_a = -e_0 e_0^T, T_b = 3 I + random with T_b[0, 0] = 0.  The leading entry of D_i = T_a G_ii + T_b is EXACTLY zero at every unobserved DOF (what
    lambda_T = 0 does to an unobserved DOF of the space-time system): no inverse without pivoting.  D^-1 A is a small perturbation of the identity, so
    the Krylov stage converges in a few iterations.  q = 1 has nothing to pivot with: T_a = 1, T_b = 2"""
    n = len(rowptr) - 1
    rng = np.random.default_rng(seed)
    gram = br.gram_selection_values(rowptr, colidx, obs, n)
    sd = 0.02 * rng.standard_normal(len(colidx))
    sd[gram_slots(rowptr, colidx, n)] = 1.0
    Ta = np.zeros((q, q))
    Ta[0, 0] = -1.0
    Tb = rng.standard_normal((q, q)) / np.sqrt(q) + 3.0 * np.eye(q)
    Tb[0, 0] = 0.0
    if q == 1:
        Ta[0, 0], Tb[0, 0] = 1.0, 2.0
    return [(Ta, gram), (Tb, sd)]


def gram_slots(rowptr, colidx, n):
    """the slot of the diagonal entry of every row"""
    return np.array([rowptr[i] + np.searchsorted(colidx[rowptr[i]:rowptr[i + 1]], i) for i in range(n)])


def diag_blocks(A, n, q):
    """D_i = A[i :: n, i :: n] for every DOF -> (n, q, q)"""
    A = A.tocsr()
    idx = np.arange(n)
    D = np.zeros((n, q, q))
    for r in range(q):
        for s in range(q):
            D[:, r, s] = np.asarray(A[r * n + idx, s * n + idx]).reshape(-1)
    return D


def block_jacobi_q(A, n, q):
    """D^-1 as a sparse matrix, D = the q x q diagonal block of every DOF in the Kronecker order"""
    Di = np.linalg.inv(diag_blocks(A, n, q))
    idx = np.arange(n)
    rows = np.concatenate([r * n + idx for r in range(q) for _ in range(q)])
    cols = np.concatenate([s * n + idx for _ in range(q) for s in range(q)])
    vals = np.concatenate([Di[:, r, s] for r in range(q) for s in range(q)])
    return sp.csr_matrix((vals, (rows, cols)), shape=(q * n, q * n))


reference_gmres = br.reference_gmres


def scaled_residual_ld(A, Dinv, b, x):
    """|D^-1 (b - A x)| / |D^-1 b| with the products and sums in np.longdouble"""
    A, Dinv = A.tocsr(), Dinv.tocsr()

    def mv(M, v):
        return _row_sums(M, M.data.astype(np.longdouble) * v[M.indices])

    xl, bl = np.asarray(x, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    r = mv(Dinv, bl - mv(A, xl))
    s = mv(Dinv, bl)
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(s * s)))


def matvec_ld(A, x):
    """(A x, |A| |x|) row by row in np.longdouble"""
    A = A.tocsr()
    terms = A.data.astype(np.longdouble) * np.asarray(x, dtype=np.longdouble)[A.indices]
    return _row_sums(A, terms), _row_sums(A, np.abs(terms))


def _row_sums(M, terms):
    """sum of `terms` (one per stored entry of the CSR matrix M) over every row, in the terms' precision; an empty row gives 0"""
    out = np.zeros(M.shape[0], dtype=terms.dtype)
    filled = np.flatnonzero(np.diff(M.indptr) > 0)
    if len(filled):
        out[filled] = np.add.reduceat(terms, M.indptr[filled])
    return out
