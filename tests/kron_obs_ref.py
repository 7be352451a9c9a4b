"""Reference side of the factored data term of the Kronecker-sum handle (tests/test_kron_obs_cpu.py, tests/test_gpu_kron_obs.py): the explicit system
    A + scale B^T W B,   B = Phi (x) Psi  (scipy.sparse.kron),
A = sum_k T_k (x) S_k (tests/kron_ref.py), Phi dense p x q, Psi n_obs x n of ANY row length (the oracle's, through tests/block_obs_ref.py), W diagonal over
(instant, location) pairs in the reference's Kronecker order (instant tau, location k at tau n_obs + k).  The space-time smoothing system is the last four
terms of kron_ref.spacetime_terms (the time penalty under its own lambda_T) with the data term factored: Phi = [H, 0], H the P1 hat functions of the m
equispaced time nodes of [0, 1] evaluated at p observation instants, W the indicator of the observations that are not missing."""
import numpy as np
import scipy.sparse as sp

import block_obs_ref as bo
import kron_ref as kr

RTOL = kr.RTOL
MAXIT_CAP = kr.MAXIT_CAP   # the budget the GPU test hands over: a cap, not a measurement
# (fixture, order, m, p, lambda, lambda_T, design, miss): the Krylov cases; design = ("points", k) | ("tiles", k per axis) | ("golden",)
SOLVE_CASES = [("unit_square_16", 1, 5, 7, 1e-4, 1e-4, ("points", 400), 0.3), ("unit_square_16", 1, 5, 5, 1e-4, 1e-4, ("points", 400), 0.0),
               ("c_shaped", 2, 3, 5, 1e-4, 1e-4, ("points", 600), 0.3), ("unit_square_16", 1, 5, 7, 1e-2, 1.0, ("tiles", 4), 0.3),
               ("unit_sphere", 1, 4, 6, 1e-4, 1e-4, ("tiles", 2), 0.3), ("quasi_circle", 1, 3, 5, 1e-2, 1e-2, ("golden",), 0.3)]
# the designs the Krylov stage cannot do within the cap (few regions leave the time penalty to carry the first block row): the dense stage's cases
DENSE_CASES = [("unit_square_16", 1, 5, 7, 1e-2, 1e-2, ("tiles", 4), 0.3), ("unit_square_16", 1, 5, 7, 1e-2, 1e-2, ("tiles", 8), 0.3),
               ("quasi_circle", 1, 3, 5, 1e-2, 1e-2, ("golden",), 0.3)]


def hats(m, times):
    """H[tau, r] = the P1 hat function of time node r (m equispaced nodes of [0, 1]) at times[tau] -> (p, m); m = 1: ones"""
    times = np.asarray(times, dtype=float)
    if m == 1:
        return np.ones((len(times), 1))
    nodes = np.linspace(0.0, 1.0, m)
    h = 1.0 / (m - 1)
    return np.maximum(0.0, 1.0 - np.abs(times[:, None] - nodes[None, :]) / h)


def identity_phi(p, q):
    """[I_p 0]: what Phi = NULL stands for"""
    return np.eye(p, q)


def weights_flat(W, p, n_obs):
    """(p, n_obs) or flat or None -> the p n_obs weights in the Kronecker order"""
    return np.ones(p * n_obs) if W is None else np.asarray(W, dtype=float).reshape(-1)


def B_matrix(Phi, Psi):
    return sp.kron(sp.csr_matrix(np.asarray(Phi, dtype=float)), Psi.tocsr(), format="csr")


def term(Phi, Psi, W, scale):
    """scale (Phi (x) Psi)^T W (Phi (x) Psi), explicit, q n x q n"""
    B = B_matrix(Phi, Psi)
    return (scale * (B.T @ sp.diags(weights_flat(W, np.shape(Phi)[0], Psi.shape[0])) @ B)).tocsr()


def system(terms, rowptr, colidx, n, Phi, Psi, W=None, scale=-1.0):
    A = (kr.explicit(terms, rowptr, colidx, n) + term(Phi, Psi, W, scale)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def design_psi(o, mesh, name, order, dofs, nd, design):
    """Psi of a design: ("points", k) -- k locations default_rng(3).uniform(bbox) (some may fall outside: empty rows) --, ("tiles", k) or ("golden",)"""
    if design[0] == "points":
        locs = np.random.default_rng(3).uniform(mesh.nodes.min(axis=0), mesh.nodes.max(axis=0), (design[1], mesh.nodes.shape[1]))
        return bo.pointwise_psi(o, mesh, order, dofs, nd, locs)
    return bo.areal_psi(o, mesh, order, dofs, nd, bo.incidence(o, mesh, name, "golden" if design[0] == "golden" else design[1]))


def spacetime(rowptr, colidx, R1, R0, Psi, lam, lam_t, m, p, miss):
    """-> (terms, Phi, W, b): the four pattern terms (q = 2 m), Phi = [H, 0] (p x 2 m), the weights (p, n_obs) of zeros and ones, and the right-hand side
    [-(B^T W z)[:m n]; lambda 0.1 u]; one generator default_rng(5), drawn in this order: the instants, the missing pattern, z, u"""
    n = len(rowptr) - 1
    rng = np.random.default_rng(5)
    times = np.sort(rng.uniform(0, 1, p))
    W = (rng.uniform(size=(p, Psi.shape[0])) >= miss).astype(float)
    terms = kr.spacetime_terms(rowptr, colidx, R1, R0, np.zeros(0, dtype=np.int64), lam, lam_t, m)[1:]
    Phi = np.hstack([hats(m, times), np.zeros((p, m))])
    return terms, Phi, W, spacetime_rhs(Phi, Psi, W, lam, m, n, rng)


def spacetime_rhs(Phi, Psi, W, lam, m, n, rng):
    """[-(B^T W z)[:m n]; lambda 0.1 u] with z (one value per instant and location), then u, drawn from rng"""
    z = rng.standard_normal(np.shape(Phi)[0] * Psi.shape[0])
    u = rng.standard_normal(m * n)
    B = B_matrix(Phi, Psi)
    return np.concatenate([-(B.T @ (np.asarray(W, dtype=float).reshape(-1) * z))[:m * n], lam * 0.1 * u])


def oracle_case(o, mesh_loader, name, order, m, p, lam, lam_t, design, miss):
    """-> (A, b, n_dofs, Psi, Phi, W, (rowptr, colidx, terms)) from the oracle's matrices"""
    mesh = mesh_loader(name)
    dofs, _, nd, _ = o.enumerate_dofs(mesh, order)
    R1 = o.assemble_operator(mesh, order, dofs, nd, -o.laplacian())
    R0 = o.assemble_operator(mesh, order, dofs, nd, o.reaction(1.0))
    assert np.array_equal(R1.rowptr, R0.rowptr) and np.array_equal(R1.colidx, R0.colidx)
    Psi = design_psi(o, mesh, name, order, dofs, nd, design)
    terms, Phi, W, b = spacetime(R1.rowptr, R1.colidx, R1.values, R0.values, Psi, lam, lam_t, m, p, miss)
    return system(terms, R1.rowptr, R1.colidx, nd, Phi, Psi, W), b, nd, Psi, Phi, W, (R1.rowptr, R1.colidx, terms)


def term_product_ld(Phi, Psi, W, scale, x):
    """-> (z, mag): scale B^T W B x and |scale| |B|^T |W| |B| |x| row by row in np.longdouble, the term applied as its factors"""
    L = np.longdouble
    B = B_matrix(Phi, Psi)
    Bt = B.T.tocsr()
    w = weights_flat(W, np.shape(Phi)[0], Psi.shape[0]).astype(L)
    t, tm = kr.matvec_ld(B, x)
    z, _ = kr.matvec_ld(Bt, w * t)
    _, zm = kr.matvec_ld(Bt, np.abs(w) * tm)
    return L(scale) * z, L(abs(scale)) * zm


def pattern_product_ld(terms, rowptr, colidx, n, x):
    """-> (y, mag): A x and |A| |x| for A = sum_k T_k (x) S_k, row by row in np.longdouble, WITHOUT forming the q n-row matrix: the entry of A at
    (r n + i, s n + j) is sum_k T_k[r, s] S_k[e] for the pattern entry e = (i, j), formed in extended precision one T-row at a time"""
    L = np.longdouble
    q = np.shape(terms[0][0])[0]
    X = np.asarray(x, dtype=L).reshape(q, n)[:, colidx].T          # (nnz, q): x[s n + j] per entry
    Ts = [np.asarray(T, dtype=L) for T, _ in terms]
    Ss = [np.asarray(S, dtype=L) for _, S in terms]
    y, mag = np.zeros((q, n), dtype=L), np.zeros((q, n), dtype=L)
    starts = np.asarray(rowptr[:-1])
    assert (np.diff(rowptr) > 0).all()
    for r in range(q):
        V = sum(S[:, None] * T[r][None, :] for T, S in zip(Ts, Ss))   # (nnz, q)
        y[r] = np.add.reduceat((V * X).sum(axis=1), starts)
        mag[r] = np.add.reduceat((np.abs(V) * np.abs(X)).sum(axis=1), starts)
    return y.reshape(-1), mag.reshape(-1)


def product_reference(A_pattern, n, Phi, Psi, W, scale, x):
    """-> (y, mag): (A + scale B^T W B) x and |A| |x| + |scale| |B|^T |W| |B| |x| row by row in np.longdouble, the term applied as its factors"""
    y, mag = kr.matvec_ld(A_pattern, x)
    z, zm = term_product_ld(Phi, Psi, W, scale, x)
    return y + z, mag + zm


def product_counts(pattern_count, n, q, p, Psi):
    """k per output row (Kronecker order r n + i): the pattern part's count + the row's Psi^T length + the longest Psi row contributing to it + p + q -- the
    rounded operations on the longest path to that output (a derived bound, not a measurement)"""
    row_len = np.diff(Psi.indptr)
    Pt = Psi.T.tocsr()
    col_len = np.diff(Pt.indptr)
    longest = np.zeros(n)
    for i in np.flatnonzero(col_len):
        longest[i] = row_len[Pt.indices[Pt.indptr[i]:Pt.indptr[i + 1]]].max()
    return np.tile(pattern_count + col_len + longest + p + q, q)
