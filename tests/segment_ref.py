"""Float64 numpy assembler for 1-D meshes (Triangulation<1,1> intervals, Triangulation<1,2> linear networks): the checker of the network
tests (a helper module, not a conftest).

Written from the reference's formulas, not from the HIP code:
  * quadrature: IntegratorTable<1,2> (P1) and IntegratorTable<1,3> (P2), utils/integration/integrator_tables.h, the 15-digit constants as
    printed there (the reference element is [0, 1], weights sum to 1);
  * basis: ReferenceElement<1,R> (finite_elements/basis/reference_element.h:31-48), nodes 0, 1 (and 0.5 for P2), in barycentric form
    P1 lambda_k, P2 vertex lambda (2 lambda - 1), midpoint 4 lambda_0 lambda_1;
  * per cell (geometry/simplex.h:184-193): J = x1 - x0 (N x 1); N = 1: invJ = 1 / J, measure = |J|; N = 2 (the manifold branch):
    invJ = (J^T J)^{-1} J^T = J^T / |J|^2, measure = |J|;
  * physical gradients g_i = invJ^T dpsi_i (N-vectors) and the weak forms laplacian.h -(g_i . g_j), diffusion.h -(g_i . K g_j) with K N x N,
    advection.h psi_i (g_j . b) with b in R^N, reaction.h c psi_i psi_j, dt.h 0;  A_ij += |e| sum_q w_q form(q);
  * an expression without an advection leaf is one the reference takes for symmetric: pairs dof_i >= dof_j, mirrored (fem_assembler.h:94-117);
  * forcing b_i += |e| sum_q f_q psi_i(p_q) w_q; Dirichlet rows zeroed with a unit diagonal (fem_solver_base.h:142-155).
DOF numbering: order 1 the nodes; order 2 the row of cell c is [v0, v1, n_nodes + c] (the segment is its own edge), midpoint J 0.5 + x0.
"""
from __future__ import annotations

import os

import numpy as np
import scipy.sparse as sp

from oracle import oracle as o

QUAD = {1: (np.array([0.211324865405187, 0.788675134594812]), np.array([0.500000000000000, 0.500000000000000])),
        2: (np.array([0.112701665379258, 0.500000000000000, 0.887298334620741]), np.array([0.277777777777778, 0.444444444444444, 0.277777777777778]))}


def load_network_fixture(root):
    """the reference's linear network (test/data/mesh/network): 201 nodes in R^2, 200 segments -> (nodes (n,2), cells (m,2) int32, boundary (n,) uint8)"""
    m = o.load_mesh(os.path.join(root, "tests", "golden", "mesh", "network"))
    return m.nodes, m.cells, m.boundary


def tables(order):
    """-> qn (nq,), qw (nq,), psi (nb, nq), dpsi (nb, nq): reference basis values and d/dxi at the quadrature nodes"""
    qn, qw = QUAD[order]
    l0, l1 = 1.0 - qn, qn
    if order == 1:
        psi = np.stack([l0, l1])
        dpsi = np.stack([-np.ones_like(qn), np.ones_like(qn)])
    else:
        psi = np.stack([l0 * (2 * l0 - 1), l1 * (2 * l1 - 1), 4 * l0 * l1])
        dpsi = np.stack([-(4 * l0 - 1), 4 * l1 - 1, 4 * (l0 - l1)])
    return qn, qw, psi, dpsi


def geometry(nodes, cells):
    """-> J (m,N), invJ (m,N), measure (m,)"""
    nodes = np.asarray(nodes, float).reshape(len(nodes), -1)
    J = nodes[cells[:, 1]] - nodes[cells[:, 0]]
    if nodes.shape[1] == 1:
        return J, 1.0 / J, np.abs(J[:, 0])
    l2 = np.einsum("md,md->m", J, J)
    return J, J / l2[:, None], np.sqrt(l2)


def dofs(cells, n_nodes, boundary, order):
    """-> (dof table (m, nb), boundary DOFs (n_dofs,), n_dofs)"""
    cells = np.asarray(cells, np.int32)
    if order == 1:
        return cells.copy(), np.asarray(boundary, np.uint8).copy(), n_nodes
    m = cells.shape[0]
    d = np.concatenate([cells, (n_nodes + np.arange(m, dtype=np.int32))[:, None]], axis=1)
    return d, np.concatenate([np.asarray(boundary, np.uint8), np.zeros(m, np.uint8)]), n_nodes + m


def dof_coords(nodes, cells, order):
    nodes = np.asarray(nodes, float).reshape(len(nodes), -1)
    if order == 1:
        return nodes.copy()
    x0 = nodes[cells[:, 0]]
    return np.concatenate([nodes, (nodes[cells[:, 1]] - x0) * 0.5 + x0], axis=0)


def quadrature_nodes(nodes, cells, order):
    """(m nq, N): x0 + J p_q, rows nq cell + q"""
    nodes = np.asarray(nodes, float).reshape(len(nodes), -1)
    J, _, _ = geometry(nodes, cells)
    qn = QUAD[order][0]
    return (nodes[cells[:, 0]][:, None, :] + J[:, None, :] * qn[None, :, None]).reshape(-1, nodes.shape[1])


def has_advection(op):
    return any(k == o.ADVECTION for (k, _, _, _) in op.terms)


def local_matrices(nodes, cells, order, op):
    """-> (m, nb, nb): [c, i, j] = |e| sum_q w_q form(psi_i test, psi_j trial)(p_q) of cell c"""
    nodes = np.asarray(nodes, float).reshape(len(nodes), -1)
    _, invJ, meas = geometry(nodes, cells)
    _, qw, psi, dpsi = tables(order)
    m, N = cells.shape[0], nodes.shape[1]
    nb, nq = psi.shape
    g = np.einsum("mr,iq->miqr", invJ, dpsi)   # physical gradients (m, nb, nq, N)
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


def assemble(nodes, cells, dof_table, n_dofs, order, op):
    """global matrix as scipy CSR (sorted columns; pattern = every pair of DOFs that share a cell), reference numbering"""
    loc = local_matrices(nodes, cells, order, op)
    nb = dof_table.shape[1]
    rows = np.repeat(dof_table, nb, axis=1).reshape(-1)
    cols = np.tile(dof_table, (1, nb)).reshape(-1)
    vals = loc.reshape(-1)
    if not has_advection(op):
        keep = rows >= cols
        L = sp.coo_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n_dofs, n_dofs)).tocsr()
        A = (L + L.T - sp.diags(L.diagonal())).tocsr()
    else:
        A = sp.coo_matrix((vals, (rows, cols)), shape=(n_dofs, n_dofs)).tocsr()
    P = sp.coo_matrix((np.zeros(rows.size), (rows, cols)), shape=(n_dofs, n_dofs)).tocsr()
    A = (A + P).tocsr()
    A.sort_indices()
    return A


def forcing(nodes, cells, dof_table, n_dofs, order, f_q):
    _, _, meas = geometry(nodes, cells)
    _, qw, psi, _ = tables(order)
    f = np.asarray(f_q, float).reshape(cells.shape[0], psi.shape[1])
    loc = np.einsum("mq,iq,q->mi", f, psi, qw) * meas[:, None]
    return np.bincount(dof_table.reshape(-1), weights=loc.reshape(-1), minlength=n_dofs)


def set_dirichlet(A, b, boundary, g):
    """rows of the boundary DOFs zeroed, unit diagonal, b = g there -> (A', b')"""
    A = A.tolil(copy=True)
    b = np.array(b, dtype=float)
    for i in np.nonzero(boundary)[0]:
        A.rows[i] = [i]
        A.data[i] = [1.0]
        b[i] = g[i]
    return A.tocsr(), b


def values_in_pattern(A, rowptr, colidx):
    A = A.tocsr()
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    return np.asarray(A[rows, colidx]).reshape(-1)


def locate(nodes, cells, locs, tol=1e-12):
    """the point-location rule of fdapde_eval_pointwise on segments: the lowest-id cell whose line is within tol max(1, |J|) of p and whose
    barycentric coordinates xi = invJ (p - x0), 1 - xi are >= -tol, else -1 -> (cell ids, xi)"""
    nodes = np.asarray(nodes, float).reshape(len(nodes), -1)
    locs = np.asarray(locs, float).reshape(len(locs), -1)
    J, invJ, meas = geometry(nodes, cells)
    x0 = nodes[cells[:, 0]]
    out, xis = np.full(len(locs), -1, np.int64), np.zeros(len(locs))
    for i, p in enumerate(locs):
        d = p[None, :] - x0
        t = np.einsum("md,md->m", invJ, d)
        r = d - t[:, None] * J
        ok = (t >= -tol) & (1.0 - t >= -tol)
        if nodes.shape[1] > 1:
            ok &= np.sqrt(np.einsum("md,md->m", r, r)) <= tol * np.maximum(1.0, meas)
        hit = np.nonzero(ok)[0]
        if hit.size:
            out[i], xis[i] = hit[0], t[hit[0]]
    return out, xis


def basis_at(order, xi):
    l0, l1 = 1.0 - xi, xi
    if order == 1:
        return np.stack([l0, l1], axis=-1)
    return np.stack([l0 * (2 * l0 - 1), l1 * (2 * l1 - 1), 4 * l0 * l1], axis=-1)
