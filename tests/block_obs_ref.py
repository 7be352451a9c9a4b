"""Reference side of the factored data term of the 2 x 2 block handle (tests/test_block_obs_cpu.py, tests/test_gpu_block_obs.py): the smoothing system
    [ scale Psi^T W Psi   lambda R1^T ] [f]   [ scale Psi^T W z ]
    [ lambda R1           lambda R0   ] [g] = [ lambda u        ]
with Psi of ANY row length -- the areal design of fdaPDE basis/lagrangian_basis.h:238-283, whose Psi^T Psi is far off the FEM pattern -- built explicitly with
scipy.  Psi comes from the oracle (oracle.areal_psi, oracle.pointwise_psi); the block-Jacobi preconditioner and scipy's GMRES(50) are tests/block_ref.py's."""
import os

import numpy as np
import scipy.sparse as sp

import block_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = br.RTOL
MAXIT_CAP = br.MAXIT_CAP   # the budget the GPU test hands over: a cap, not a measurement
# (fixture, order, lambda, regions): the Krylov cases of the issue; regions = tiles per axis of the bounding box, or "golden" (quasi_circle's incidence matrix)
KRYLOV_CASES = [("unit_square_16", 1, 1e-2, 4), ("unit_square_16", 1, 1e-4, 4), ("unit_square_16", 2, 1e-4, 4), ("unit_sphere", 1, 1e-2, 2),
                ("unit_sphere", 1, 1e-4, 2), ("quasi_circle", 1, 1e-2, "golden"), ("quasi_circle", 1, 1e-4, "golden")]


def tiles(mesh, k):
    """incidence matrix (regions x cells) of k boxes per axis over the mesh's bounding box: a cell belongs to the region of the box its barycentre falls in;
    boxes without a cell give no region"""
    bary = mesh.nodes[mesh.cells].mean(axis=1)
    lo, hi = mesh.nodes.min(axis=0), mesh.nodes.max(axis=0)
    ijk = np.minimum((k * (bary - lo) / (hi - lo)).astype(np.int64), k - 1)
    box = np.zeros(mesh.n_cells, dtype=np.int64)
    for d in range(mesh.N):
        box = box * k + ijk[:, d]
    ids = np.unique(box)
    inc = np.zeros((len(ids), mesh.n_cells))
    inc[np.searchsorted(ids, box), np.arange(mesh.n_cells)] = 1.0
    return inc


def incidence(o, mesh, name, regions):
    if regions == "golden":
        return o.read_csv(os.path.join(ROOT, "tests", "golden", "mesh", name, "incidence_matrix.csv"))
    return tiles(mesh, regions)


def areal_psi(o, mesh, order, dofs, nd, inc):
    """oracle.areal_psi -> CSR with sorted columns (a stored entry per DOF of the region's cells, zeros of the dense result dropped)"""
    dense, _ = o.areal_psi(mesh, order, dofs, nd, inc)
    P = sp.csr_matrix(dense)
    P.sort_indices()
    return P


def pointwise_psi(o, mesh, order, dofs, nd, locs):
    """oracle.pointwise_psi -> CSR; a location outside the mesh gives an empty row"""
    P = sp.csr_matrix(o.pointwise_psi(mesh, order, dofs, nd, locs))
    P.sort_indices()
    return P


def term(Psi, weights, scale):
    """scale Psi^T W Psi, explicit"""
    w = np.ones(Psi.shape[0]) if weights is None else np.asarray(weights, dtype=float)
    return (scale * (Psi.T @ sp.diags(w) @ Psi)).tocsr()


def system(rowptr, colidx, blocks, nd, Psi, weights=None, scale=-1.0):
    """the 2 n x 2 n matrix in the stacked order: the four blocks on the pattern (None = a zero block) + scale Psi^T W Psi in the (1,1) block"""
    A = br.bmat(rowptr, colidx, blocks, nd)
    T = term(Psi, weights, scale)
    return (A + sp.bmat([[T, None], [None, sp.csr_matrix((nd, nd))]], format="csr")).tocsr()


def smoothing_blocks(rowptr, colidx, r1, r0, lam, nd):
    """(None, lambda R1^T, lambda R1, lambda R0): the (1,1) block is the factored term's alone"""
    return (None, lam * br.transpose_values(rowptr, colidx, r1, nd), lam * np.asarray(r1, dtype=float), lam * np.asarray(r0, dtype=float))


def smoothing_rhs(Psi, lam, nd, seed=1):
    """[-Psi^T z; lambda u] for random z, u (block_ref.smoothing_rhs with Psi in place of the selection)"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(Psi.shape[0])
    u = 0.1 * rng.standard_normal(nd)
    return np.concatenate([-(Psi.T @ z), lam * u])


def oracle_case(o, mesh_loader, name, order, lam, regions):
    """-> (A, b, n_dofs, Psi, (rowptr, colidx, blocks)) from the oracle's matrices"""
    m = mesh_loader(name)
    dofs, _, nd, _ = o.enumerate_dofs(m, order)
    R1 = o.assemble_operator(m, order, dofs, nd, -o.laplacian())
    R0 = o.assemble_operator(m, order, dofs, nd, o.reaction(1.0))
    assert np.array_equal(R1.rowptr, R0.rowptr) and np.array_equal(R1.colidx, R0.colidx)
    Psi = areal_psi(o, m, order, dofs, nd, incidence(o, m, name, regions))
    blocks = smoothing_blocks(R1.rowptr, R1.colidx, R1.values, R0.values, lam, nd)
    return system(R1.rowptr, R1.colidx, blocks, nd, Psi), smoothing_rhs(Psi, lam, nd), nd, Psi, (R1.rowptr, R1.colidx, blocks)


def product_bound(rowptr, colidx, blocks, nd, Psi, weights, scale, x):
    """per row of y = (A + term) x, stacked order: (terms + 1) eps (|A| |x| + |scale| |Psi|^T |W| |Psi| |x_1|), terms = twice the row's pattern entries + its
    Psi^T row length + the longest Psi row that contributes to it (second block row: the pattern entries alone)"""
    eps = np.finfo(float).eps
    absA = abs(br.bmat(rowptr, colidx, blocks, nd))
    aP = abs(Psi).tocsr()
    w = np.ones(Psi.shape[0]) if weights is None else np.abs(weights)
    mag = absA @ np.abs(x)
    mag[:nd] += abs(scale) * (aP.T @ (w * (aP @ np.abs(x[:nd]))))
    row_len = np.diff(Psi.indptr)
    Pt = Psi.T.tocsr()
    col_len = np.diff(Pt.indptr)
    longest = np.zeros(nd)
    for i in np.flatnonzero(col_len):
        longest[i] = row_len[Pt.indices[Pt.indptr[i]:Pt.indptr[i + 1]]].max()
    pat = np.diff(rowptr)
    terms = np.concatenate([2 * pat + col_len + longest, 2 * pat])
    return (terms + 1) * eps * mag


def product_reference(rowptr, colidx, blocks, nd, Psi, weights, scale, x):
    """(A + term) x in extended precision, the term as the explicit (dense) matrix scale Psi^T W Psi"""
    L = np.longdouble
    xl = x.astype(L)
    y = np.zeros(2 * nd, dtype=L)
    A = br.bmat(rowptr, colidx, blocks, nd).tocsr()
    rows = np.repeat(np.arange(2 * nd), np.diff(A.indptr))
    np.add.at(y, rows, A.data.astype(L) * xl[A.indices])
    T = np.zeros((nd, nd), dtype=L)
    for k in range(Psi.shape[0]):   # (the columns of a row are distinct: the indexed += adds every entry once)
        cols = Psi.indices[Psi.indptr[k]:Psi.indptr[k + 1]]
        if len(cols):
            v = Psi.data[Psi.indptr[k]:Psi.indptr[k + 1]].astype(L)
            T[np.ix_(cols, cols)] += (L(1.0) if weights is None else L(weights[k])) * np.outer(v, v)
    y[:nd] += L(scale) * (T @ xl[:nd])
    return y
