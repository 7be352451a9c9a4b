"""Surface meshes (Triangulation<2,3>), CPU side: pins the numpy surface assembler (tests/surface_ref.py) -- the checker of
tests/test_gpu_surface.py -- to the CPU oracle and through it to the reference, and the mesh generators of meshgen.py.
  * a planar fixture moved into R^3 by a rigid motion x -> Q x + t (Q 3 x 2, orthonormal columns) must give, through surface_ref, the
    oracle's planar matrices and load vectors, with K3 = Q K2 Q^T and b3 = Q b2 (the surface formulas reduce to the planar ones);
  * the oracle's topology of the reference's surface fixture matches its neigh.csv / edges.csv, and its P2 DOF count;
  * the generators' sizes and invariants."""
import os

import numpy as np
import pytest

import surface_ref as sr

TOL = 1e-13


def _ops2(o, K, b, rows, rng):
    """(name, operator) of tests/test_gpu_parity.py with 2-D coefficients, and space-varying leaves (one row per quadrature node) -- a
    non-symmetric K field among them, alone (the reference's mirrored lower triangle) and next to advection"""
    Kn = K + np.array([[0.0, 0.4], [-0.2, 0.0]])
    A = rng.standard_normal((rows, 2, 2)) * 0.3
    Kq = np.einsum("rij,rkj->rik", A, A) + np.eye(2)[None]
    Kqn = Kq + rng.uniform(-0.3, 0.3, (rows, 1, 1)) * np.array([[0.0, 1.0], [-1.0, 0.0]])[None]
    bq, cq = rng.standard_normal((rows, 2)), rng.uniform(0.5, 2.0, rows)
    fields = [("var_kbc", o.diffusion_field(Kq.reshape(rows, 4)) + o.advection_field(bq) + o.reaction_field(cq)),
              ("var_k_nonsym_mirrored", o.diffusion_field(Kqn.reshape(rows, 4)) + o.reaction_field(cq)),
              ("var_k_nonsym_adv", -o.laplacian() + o.diffusion_field(Kqn.reshape(rows, 4)) + o.advection(b)),
              ("var_b_const_k", o.diffusion(K) + o.advection_field(bq))]
    return fields + [("neg_laplacian", -o.laplacian()), ("mass", o.reaction(1.0)), ("adr", -o.laplacian() + o.advection(b) + o.reaction(1.5)),
            ("diffusion", o.diffusion(K) + 0.5 * o.reaction(2.0)), ("laplacian_minus_dt", o.laplacian() - o.dt()),
            ("diffusion_nonsym", o.diffusion(Kn) + o.advection(b) + o.reaction(0.5)), ("diffusion_nonsym_mirrored", o.diffusion(Kn) + o.reaction(0.5))]


def _lift(o, op, Q):
    """the same operator with its coefficients pushed forward: K3 = Q K2 Q^T, b3 = Q b2 -- constants, and fields row by row (rows of 9 / 3
    values, row-major per quadrature node, as the C ABI takes them)"""
    terms = []
    for (k, c, cst, d) in op.terms:
        if k == o.DIFFUSION:
            if d is None:
                cst = Q @ np.asarray(cst).reshape(2, 2) @ Q.T
            else:
                d = np.einsum("ik,rkl,jl->rij", Q, np.asarray(d).reshape(-1, 2, 2), Q).reshape(-1, 9)
        elif k == o.ADVECTION:
            if d is None:
                cst = Q @ np.asarray(cst).reshape(2)
            else:
                d = np.asarray(d).reshape(-1, 2) @ Q.T
        terms.append((k, c, cst, d))
    return o.Operator(terms)


def _embedding(seed):
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import meshgen

    R = meshgen.rotation(seed)
    t = np.random.default_rng(seed).uniform(-2, 2, 3)
    return R[:, :2], t, meshgen


@pytest.mark.parametrize("name", ["unit_square_16", "quasi_circle"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rigid_motion_of_a_planar_fixture_gives_the_planar_oracle(oracle, mesh_loader, name, order, seed):
    o = oracle
    m = mesh_loader(name)
    Q, t, meshgen = _embedding(seed)
    nodes3 = meshgen.embed_planar(m.nodes, Q, t)
    dofs, bnd, nd, _ = o.enumerate_dofs(m, order)
    K = np.array([[2.0, 0.3], [0.3, 1.0]])
    b = np.array([0.7, -0.2])
    nq = sr.tables(order)[0].shape[0]
    for label, op in _ops2(o, K, b, nq * m.n_cells, np.random.default_rng(100 + seed)):
        ref = o.assemble_operator(m, order, dofs, nd, op).to_scipy().toarray()
        got = sr.assemble(nodes3, m.cells, dofs, nd, order, _lift(o, op, Q)).toarray()
        scale = np.abs(ref).max()
        assert np.abs(got - ref).max() <= TOL * scale, (name, order, seed, label, np.abs(got - ref).max() / scale)
    nq = sr.tables(order)[0].shape[0]
    fq = np.random.default_rng(seed).standard_normal(nq * m.n_cells)
    fr = o.assemble_forcing(m, order, dofs, nd, fq)
    fs = sr.forcing(nodes3, m.cells, dofs, nd, order, fq)
    assert np.abs(fs - fr).max() <= TOL * np.abs(fr).max()
    # quadrature nodes and DOF coordinates move with the mesh
    qp = o.quadrature_nodes(m, order)
    assert np.abs(sr.quadrature_nodes(nodes3, m.cells, order) - (qp @ Q.T + t)).max() <= 1e-14
    dc = o.dofs_coords(m, order, dofs, nd)
    assert np.abs(sr.dof_coords(nodes3, m.cells, dofs, nd, order) - (dc @ Q.T + t)).max() <= 1e-14


def test_surface_fixture_topology_matches_the_reference_files(oracle, golden_dir):
    o = oracle
    m = o.load_mesh(os.path.join(golden_dir, "mesh", "surface"))
    assert (m.n_nodes, m.n_cells, int(m.boundary.sum()), m.M, m.N) == (340, 616, 64, 2, 3)
    t = o.topology(m)
    d = os.path.join(golden_dir, "mesh", "surface")
    neigh = o.read_csv(os.path.join(d, "neigh.csv")).astype(np.int64)
    assert np.array_equal(np.where(neigh > 0, neigh - 1, -1), t["neighbors"])
    edges = np.sort(o.read_csv(os.path.join(d, "edges.csv")).astype(np.int64) - 1, axis=1)
    assert len(edges) == len(t["facet_nodes"]) and set(map(tuple, edges)) == set(map(tuple, t["facet_nodes"]))
    dofs, bnd, nd, ne = o.enumerate_dofs(m, 2)
    assert nd == 1296 and int(bnd.sum()) == 128


def test_surface_fixture_measures_are_cross_products(oracle, golden_dir):
    m = oracle.load_mesh(os.path.join(golden_dir, "mesh", "surface"))
    J, invJ, meas = sr.geometry(m.nodes, m.cells)
    assert np.all(meas > 0)
    # invJ is a left inverse of J, and the area is sqrt(det J^T J) / 2
    assert np.abs(invJ @ J - np.eye(2)).max() < 1e-12
    assert np.abs(meas - 0.5 * np.sqrt(np.linalg.det(np.einsum("mki,mkj->mij", J, J)))).max() < 1e-14


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
def test_unit_sphere_surface_sizes(level):
    _, _, meshgen = _embedding(1)
    n, c, b = meshgen.unit_sphere_surface(level)
    assert n.shape == (10 * 4**level + 2, 3) and c.shape == (20 * 4**level, 3) and b.sum() == 0
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-15
    e = np.sort(np.concatenate([c[:, [0, 1]], c[:, [1, 2]], c[:, [0, 2]]]), axis=1)
    _, cnt = np.unique(e[:, 0] * n.shape[0] + e[:, 1], return_counts=True)
    assert np.all(cnt == 2)   # closed: every edge between two triangles
    # total area converges to 4 pi from below
    if level >= 3:
        _, _, meas = sr.geometry(n, c)
        assert 4 * np.pi * (1 - 0.01) < meas.sum() < 4 * np.pi


def test_height_field_surface_and_embedding():
    Q, t, meshgen = _embedding(5)
    n, c, b = meshgen.height_field_surface(10, reorient=True)
    n0, c0, b0 = meshgen.height_field_surface(10)
    assert n.shape == (121, 3) and c.shape == (200, 3) and int(b.sum()) == 40
    assert np.array_equal(np.sort(c, axis=1), np.sort(c0, axis=1)) and not np.array_equal(c, c0)
    p = np.random.default_rng(0).standard_normal((7, 2))
    x = meshgen.embed_planar(p, Q, t)
    assert np.abs(np.linalg.norm(x[:, None] - x[None], axis=2) - np.linalg.norm(p[:, None] - p[None], axis=2)).max() < 1e-13
