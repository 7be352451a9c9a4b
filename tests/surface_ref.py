"""Float64 numpy assembler for surface meshes (Triangulation<2,3>): the checker of the surface tests (a helper module, not a conftest).

Written from the reference's formulas, not from the HIP code:
  * per cell (fdaPDE/geometry/simplex.h:184-195, the branch embed_dim != local_dim):  J = [x1 - x0, x2 - x0] (3 x 2),
    invJ = (J^T J)^{-1} J^T (2 x 3),  |e| = |(x1 - x0) x (x2 - x0)| / 2;
  * physical gradients g_i = invJ^T dpsi_i (3-vectors, fem_assembler.h:81), and the weak forms of the planar case:
    laplacian.h:43 -(g_i . g_j), diffusion.h:54 -(g_i . K g_j) with K 3 x 3, advection.h:55 psi_i (g_j . b) with b in R^3,
    reaction.h:52 c psi_i psi_j, dt.h 0;  A_ij += |e| sum_q w_q form(q);
  * an expression without an advection leaf is one the reference takes for symmetric (diffusion.h:42): only the pairs dof_i >= dof_j are
    integrated and the lower triangle is mirrored (fem_assembler.h:94-102, 116-117) -- which matters for a non-symmetric K only;
  * forcing b_i += |e| sum_q f_q psi_i(p_q) w_q (fem_assembler.h:122-136); Dirichlet rows zeroed with a unit diagonal (fem_solver_base.h:142-155).
Quadrature, reference basis and DOF numbering come from the CPU oracle (oracle.quadrature / basis_tables / enumerate_dofs): they depend on
the local dimension and the connectivity only.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from oracle import oracle as o


def load_surface_fixture(root):
    """the reference's 2.5-D fixture (test/data/mesh/surface): 340 nodes in R^3, 616 triangles, 64 boundary nodes"""
    import os

    return o.load_mesh(os.path.join(root, "tests", "golden", "mesh", "surface"))


def mesh_of(nodes, cells, boundary):
    return o.Mesh(np.ascontiguousarray(nodes, dtype=float), np.ascontiguousarray(cells, dtype=np.int32), np.ascontiguousarray(boundary, dtype=np.uint8))


def geometry(nodes, cells):
    """-> J (m,N,2), invJ (m,2,N), measure (m,); N = 2 or 3"""
    x0 = nodes[cells[:, 0]]
    J = np.stack([nodes[cells[:, 1]] - x0, nodes[cells[:, 2]] - x0], axis=2)
    if nodes.shape[1] == 2:
        invJ = np.linalg.inv(J)
        meas = np.abs(np.linalg.det(J)) / 2.0
    else:
        JtJ = np.einsum("mki,mkj->mij", J, J)
        invJ = np.linalg.inv(JtJ) @ np.transpose(J, (0, 2, 1))
        meas = 0.5 * np.linalg.norm(np.cross(J[:, :, 0], J[:, :, 1]), axis=1)
    return J, invJ, meas


def tables(order):
    qn, qw = o.quadrature(2, order)
    psi, dpsi = o.basis_tables(2, order)   # (nb, nq), (nb, nq, 2)
    return qn, qw, psi, dpsi


def has_advection(op):
    return any(k == o.ADVECTION for (k, _, _, _) in op.terms)


def local_matrices(nodes, cells, order, op):
    """-> (m, nb, nb): [c, i, j] = |e| sum_q w_q form(psi_i test, psi_j trial)(p_q) of cell c"""
    _, invJ, meas = geometry(nodes, cells)
    qn, qw, psi, dpsi = tables(order)
    m, N = cells.shape[0], nodes.shape[1]
    nb, nq = psi.shape
    g = np.einsum("mkr,iqk->miqr", invJ, dpsi)   # physical gradients (m, nb, nq, N)
    out = np.zeros((m, nb, nb))
    for (kind, coef, cst, data) in op.terms:
        if kind == o.DT:
            continue
        if kind == o.LAPLACIAN:
            v = -np.einsum("miqr,mjqr->mijq", g, g)
        elif kind == o.DIFFUSION:
            K = (np.broadcast_to(np.asarray(cst, float).reshape(N, N), (m, nq, N, N)) if data is None
                 else np.asarray(data, float).reshape(m, nq, N, N))
            v = -np.einsum("miqr,mqrs,mjqs->mijq", g, K, g)
        elif kind == o.ADVECTION:
            b = (np.broadcast_to(np.asarray(cst, float).reshape(N), (m, nq, N)) if data is None else np.asarray(data, float).reshape(m, nq, N))
            v = np.einsum("iq,mjqr,mqr->mijq", psi, g, b)
        elif kind == o.REACTION:
            c = np.broadcast_to(np.asarray(cst, float).reshape(1)[0], (m, nq)) if data is None else np.asarray(data, float).reshape(m, nq)
            v = np.einsum("mq,iq,jq->mijq", c, psi, psi)
        else:
            raise ValueError(kind)
        out += coef * np.einsum("mijq,q->mij", v, qw)
    return out * meas[:, None, None]


def assemble(nodes, cells, dofs, n_dofs, order, op):
    """global matrix as scipy CSR (sorted columns; pattern = every pair of DOFs that share a cell), reference numbering"""
    loc = local_matrices(nodes, cells, order, op)
    nb = dofs.shape[1]
    rows = np.repeat(dofs, nb, axis=1).reshape(-1)
    cols = np.tile(dofs, (1, nb)).reshape(-1)
    vals = loc.reshape(-1)
    if not has_advection(op):   # the reference's symmetric path: pairs dof_i >= dof_j, mirrored
        keep = rows >= cols
        r, c, v = rows[keep], cols[keep], vals[keep]
        L = sp.coo_matrix((v, (r, c)), shape=(n_dofs, n_dofs)).tocsr()
        D = sp.diags(L.diagonal())
        A = (L + L.T - D).tocsr()
    else:
        A = sp.coo_matrix((vals, (rows, cols)), shape=(n_dofs, n_dofs)).tocsr()
    P = sp.coo_matrix((np.zeros(rows.size), (rows, cols)), shape=(n_dofs, n_dofs)).tocsr()   # the full pattern (explicit zeros kept)
    A = (A + P).tocsr()
    A.sort_indices()
    return A


def forcing(nodes, cells, dofs, n_dofs, order, f_q):
    _, _, meas = geometry(nodes, cells)
    _, qw, psi, _ = tables(order)
    nq = psi.shape[1]
    f = np.asarray(f_q, float).reshape(cells.shape[0], nq)
    loc = np.einsum("mq,iq,q->mi", f, psi, qw) * meas[:, None]
    return np.bincount(dofs.reshape(-1), weights=loc.reshape(-1), minlength=n_dofs)


def quadrature_nodes(nodes, cells, order):
    """(m nq, N): x0 + J p_q, rows nq cell + q"""
    J, _, _ = geometry(nodes, cells)
    qn, _, _, _ = tables(order)
    x = nodes[cells[:, 0]][:, None, :] + np.einsum("mdk,qk->mqd", J, qn)
    return x.reshape(-1, nodes.shape[1])


def dof_coords(nodes, cells, dofs, n_dofs, order):
    """vertices, then every edge DOF from the FIRST cell that visits it: x0 + sum_k (x_{k+1} - x0) ref_k (lagrangian_basis.h:159-183)"""
    out = np.zeros((n_dofs, nodes.shape[1]))
    out[: nodes.shape[0]] = nodes
    if order == 2:
        ref = o.reference_nodes(2, 2)
        seen = np.zeros(n_dofs, dtype=bool)
        seen[: nodes.shape[0]] = True
        for c in range(cells.shape[0]):
            x0 = nodes[cells[c, 0]]
            for j in range(3, dofs.shape[1]):
                d = dofs[c, j]
                if not seen[d]:
                    acc = np.zeros(nodes.shape[1])
                    for k in range(2):
                        acc = acc + (nodes[cells[c, k + 1]] - x0) * ref[j, k]
                    out[d] = acc + x0
                    seen[d] = True
    return out


def set_dirichlet(A, b, boundary, g):
    """rows of the boundary DOFs zeroed, unit diagonal, b = g there (fem_solver_base.h:142-155) -> (A', b')"""
    A = A.tolil(copy=True)
    b = np.array(b, dtype=float)
    for i in np.nonzero(boundary)[0]:
        A.rows[i] = [i]
        A.data[i] = [1.0]
        b[i] = g[i]
    return A.tocsr(), b


def values_in_pattern(A, rowptr, colidx):
    """A's entries in a CSR pattern (rowptr, colidx) -- that of fdapde_pattern_get"""
    A = A.tocsr()
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    return np.asarray(A[rows, colidx]).reshape(-1)
