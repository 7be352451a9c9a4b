"""1-D meshes (Triangulation<1,1> intervals, Triangulation<1,2> networks), CPU side: pins the numpy segment assembler (tests/segment_ref.py) --
the checker of tests/test_gpu_network.py -- to the closed-form element matrices of a segment of length h, checks that a straight polyline in
R^2 assembles to the matrix of the interval of its arc length, and the 1-D mesh generators of meshgen.py."""
import os

import numpy as np
import pytest

import segment_ref as sg
from oracle import oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-13


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("h", [1.0, 0.37, 2.5e-3, 17.0])
@pytest.mark.parametrize("N", [1, 2])
def test_closed_form_element_matrices(h, N):
    if N == 1:
        nodes = np.array([[0.3], [0.3 + h]])
    else:
        d = np.array([0.6, -0.8])
        nodes = np.array([[1.0, 2.0], [1.0, 2.0]]) + np.array([[0.0, 0.0], h * d])
    cells = np.array([[0, 1]], np.int32)
    K1 = sg.local_matrices(nodes, cells, 1, -o.laplacian())[0]
    M1 = sg.local_matrices(nodes, cells, 1, o.reaction(1.0))[0]
    K2 = sg.local_matrices(nodes, cells, 2, -o.laplacian())[0]
    M2 = sg.local_matrices(nodes, cells, 2, o.reaction(1.0))[0]
    assert _rel(K1, np.array([[1, -1], [-1, 1]]) / h) <= TOL
    assert _rel(M1, h / 6 * np.array([[2, 1], [1, 2]])) <= TOL
    assert _rel(K2, np.array([[7, 1, -8], [1, 7, -8], [-8, -8, 16]]) / (3 * h)) <= TOL
    assert _rel(M2, h / 30 * np.array([[4, -1, 2], [-1, 4, 2], [2, 2, 16]])) <= TOL


def test_quadrature_tables_are_the_references():
    for order, nq in [(1, 2), (2, 3)]:
        qn, qw, psi, dpsi = sg.tables(order)
        assert qn.size == nq and abs(qw.sum() - 1.0) <= 1e-15
        assert np.allclose(psi.sum(axis=0), 1.0, atol=1e-14) and np.allclose(dpsi.sum(axis=0), 0.0, atol=1e-13)
    assert sg.QUAD[1][0][0] == 0.211324865405187 and sg.QUAD[2][1][1] == 0.444444444444444


@pytest.mark.parametrize("order", [1, 2])
def test_straight_polyline_equals_interval(order):
    rng = np.random.default_rng(3)
    s = np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 0.3, 20))])
    d = np.array([np.cos(0.7), np.sin(0.7)])
    plane = np.array([-1.0, 4.0])[None, :] + s[:, None] * d[None, :]
    cells = np.stack([np.arange(20), np.arange(1, 21)], axis=1).astype(np.int32)
    flip = rng.random(20) < 0.5
    cells2 = cells.copy()
    cells2[flip] = cells2[flip][:, ::-1]   # orientation is free
    bnd = np.zeros(21, np.uint8)
    dt, _, nd = sg.dofs(cells, 21, bnd, order)
    dt2, _, _ = sg.dofs(cells2, 21, bnd, order)
    b = 0.8
    for op1, op2 in [(-o.laplacian(), -o.laplacian()), (o.reaction(1.0), o.reaction(1.0)),
                     (o.diffusion(np.array([[2.0]])) + o.advection(np.array([b])), o.diffusion(2.0 * np.outer(d, d) + 0.3 * np.eye(2) - 0.3 * np.outer(d, d)) + o.advection(b * d))]:
        A1 = sg.assemble(s, cells, dt, nd, order, op1).toarray()
        A2 = sg.assemble(plane, cells2, dt2, nd, order, op2).toarray()
        assert np.abs(A1 - A2).max() <= 1e-12 * np.abs(A1).max()


def test_network_fixture_and_generators():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import meshgen

    nodes, cells, bnd = sg.load_network_fixture(ROOT)
    assert nodes.shape == (201, 2) and cells.shape == (200, 2) and int(bnd.sum()) == 2
    assert np.all(np.bincount(cells.reshape(-1), minlength=201) > 0)
    n, c, b = meshgen.interval(10, 0.0, 2.0, jitter=0.3, permute=True, seed=4)
    assert n.shape == (11, 1) and c.shape == (10, 2) and b.sum() == 2
    assert abs(sg.geometry(n, c)[2].sum() - 2.0) <= 1e-14
    assert set(np.round(n[b == 1, 0], 14)) == {0.0, 2.0}
    L = np.array([1.0, 2.0, 0.5])
    n, c, b = meshgen.star(3, L, k=4)
    assert n.shape == (13, 2) and c.shape == (12, 2) and b.sum() == 3 and abs(sg.geometry(n, c)[2].sum() - L.sum()) <= 1e-14
    n, c, b = meshgen.street_grid(6, 5, k=3, seed=2, drop=0.2)
    deg = np.bincount(c.reshape(-1), minlength=n.shape[0])
    assert np.all(deg > 0) and np.array_equal(b, (deg == 1).astype(np.uint8))
    n2, c2, b2 = meshgen.street_grid(6, 5, k=3, seed=2, drop=0.2)
    assert np.array_equal(n, n2) and np.array_equal(c, c2)
    n, c, b = meshgen.street_grid(4, 4, k=4, drop=0.0, jitter=0.0, permute=False)
    assert np.array_equal(n * 4, np.round(n * 4)) and c.shape[0] == 2 * 4 * 5 * 4


def test_locate_rule():
    nodes = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]])
    cells = np.array([[0, 1], [1, 2]], np.int32)
    ids, xi = sg.locate(nodes, cells, np.array([[0.5, 0.0], [1.0, 0.0], [1.0, 0.25], [0.5, 1e-6], [2.0, 0.0]]))
    assert list(ids) == [0, 0, 1, -1, -1]
    assert abs(xi[0] - 0.5) < 1e-15 and abs(xi[2] - 0.25) < 1e-15
