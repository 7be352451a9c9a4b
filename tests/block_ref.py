"""Reference side of the 2 x 2 block tests (tests/test_block_cpu.py, tests/test_gpu_block.py): the smoothing system
    [ -Psi^T W Psi   lambda R1^T ] [f]   [ -Psi^T W z ]
    [  lambda R1     lambda R0   ] [g] = [  lambda u   ]
(fdaPDE/linear_algebra/sparse_block_matrix.h:29-128) built with scipy from matrices on the FEM pattern, its 2 x 2 block-Jacobi preconditioner,
and scipy's restarted GMRES(50) on the explicitly left-preconditioned system -- the iteration the device's Krylov stage performs."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

RTOL = 1e-10
MAXIT_CAP = 1000   # the budget the GPU test hands over: a cap, not a measurement
# (fixture, order, lambda, advection in R1): the Krylov cases of the issue
KRYLOV_CASES = [("unit_square_16", 1, 1e-2, False), ("unit_square_16", 1, 1e-4, False), ("unit_square_16", 1, 1e-6, False),
                ("c_shaped", 2, 1e-4, False), ("unit_sphere", 1, 1e-4, False), ("unit_square_16", 1, 1e-4, True)]


def observed_nodes(n_nodes):
    """observations at half of the nodes"""
    return np.sort(np.random.default_rng(0).choice(n_nodes, n_nodes // 2, replace=False))


def on_pattern(rowptr, colidx, values, n):
    return sp.csr_matrix((np.asarray(values, dtype=float), colidx, rowptr), shape=(n, n))


def transpose_values(rowptr, colidx, values, n):
    """values of A^T on the (structurally symmetric) pattern of A, entry for entry"""
    at = on_pattern(rowptr, colidx, values, n).T.tocsr()
    at.sort_indices()
    assert np.array_equal(at.indptr, rowptr) and np.array_equal(at.indices, colidx), "the FEM pattern is structurally symmetric"
    return at.data.copy()


def gram_selection_values(rowptr, colidx, obs, n):
    """Psi^T Psi on the pattern for Psi = rows of the identity at the observed DOFs (W = I): the indicator of `obs` on the diagonal"""
    vals = np.zeros(len(colidx))
    for i in obs:
        k = rowptr[i] + np.searchsorted(colidx[rowptr[i]:rowptr[i + 1]], i)
        assert colidx[k] == i
        vals[k] = 1.0
    return vals


def smoothing_blocks(rowptr, colidx, r1, r0, obs, lam, n):
    """-> (a11, a12, a21, a22) as value arrays on the pattern"""
    return (-gram_selection_values(rowptr, colidx, obs, n), lam * transpose_values(rowptr, colidx, r1, n), lam * np.asarray(r1, dtype=float),
            lam * np.asarray(r0, dtype=float))


def bmat(rowptr, colidx, blocks, n):
    """the 2 n x 2 n matrix in the stacked order; None = a zero block"""
    m = [[None if v is None else on_pattern(rowptr, colidx, v, n) for v in blocks[:2]], [None if v is None else on_pattern(rowptr, colidx, v, n) for v in blocks[2:]]]
    for r in range(2):
        for c in range(2):
            if m[r][c] is None:
                m[r][c] = sp.csr_matrix((n, n))
    return sp.bmat(m, format="csr")


def smoothing_rhs(obs, lam, n, seed=1):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(len(obs))
    u = 0.1 * rng.standard_normal(n)
    b = np.zeros(2 * n)
    b[obs] = -z
    b[n:] = lam * u
    return b


def block_jacobi(A, n):
    """D^-1 as a sparse matrix, D = the 2 x 2 diagonal block of every DOF in the stacked order"""
    d = A.diagonal()
    a, e = d[:n], d[n:]
    b = np.asarray(A[np.arange(n), np.arange(n) + n]).reshape(-1)
    c = np.asarray(A[np.arange(n) + n, np.arange(n)]).reshape(-1)
    det = a * e - b * c
    return sp.bmat([[sp.diags(e / det), sp.diags(-b / det)], [sp.diags(-c / det), sp.diags(a / det)]], format="csr")


def reference_gmres(A, Dinv, b, rtol=RTOL, restart=50, max_cycles=40):
    """scipy's GMRES(restart) on D^-1 A x = D^-1 b -> (x, inner iterations, info)"""
    MA = (Dinv @ A).tocsr()
    Mb = Dinv @ b
    count = [0]

    def cb(_):
        count[0] += 1

    x, info = spl.gmres(MA, Mb, rtol=rtol, atol=0.0, restart=restart, maxiter=max_cycles, callback=cb, callback_type="pr_norm")
    return x, count[0], info


def scaled_residual(A, Dinv, b, x):
    """|D^-1 (b - A x)| / |D^-1 b| with numpy's own summation order"""
    return np.linalg.norm(Dinv @ (b - A @ x)) / np.linalg.norm(Dinv @ b)
