"""fdapde_project on the device: every point onto its nearest cell, on every mesh kind, orders 1 and 2.

The tolerance is the project's own location tolerance tau = 1e-12 max(1, L), L the largest absolute coordinate of mesh and points.
Per point, against the mesh in reference numbering (_check):
 (a) q is the closest point of the RETURNED cell: in mpmath (project_ref.closest_point_defects) it lies in the cell, in its plane or line, and no
     vertex is on the far side of the plane through q normal to p - q, each within tau in length units;
 (b) dist = |p - q| within tau;
 (c) dist <= the brute-force minimum over all cells (project_ref.brute_force, certified by tests/test_project_ref_cpu.py) + tau;
 (d) every row of Psi sums to 1 within 1e-13 (at most 10 terms of magnitude <= 1), P1 values are in [0, 1], Psi . dof_coords = q within tau."""
import os

import numpy as np
import pytest

import project_ref as pr
import segment_ref as sg
import surface_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = [1, 2]


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, meshgen


@pytest.fixture(scope="module")
def surface():
    from oracle import oracle as o

    o.build()
    m = sr.load_surface_fixture(ROOT)
    return np.ascontiguousarray(m.nodes), np.ascontiguousarray(m.cells, dtype=np.int32), np.ascontiguousarray(m.boundary)


@pytest.fixture(scope="module")
def network():
    from oracle import oracle as o

    o.build()
    return sg.load_network_fixture(ROOT)


def _ctx(capi, nodes, cells, bnd, order, **kw):
    c = capi.Context(**kw) if kw else capi.Context(device=0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(order)
    return c


def _tau(nodes, pts):
    return 1e-12 * max(1.0, float(np.abs(nodes).max()), float(np.abs(pts).max()))


def _check(c, nodes, cells, pts, order, out=None):
    """checks (a) - (d) for every point; -> (psi, cell, q, dist)"""
    nodes = np.asarray(nodes, dtype=float).reshape(len(nodes), -1)
    pts = np.asarray(pts, dtype=float).reshape(len(pts), -1)
    psi, cell, q, dist = out if out is not None else c.project(pts)
    tau = _tau(nodes, pts)
    n = len(pts)
    assert cell.shape == (n,) and q.shape == pts.shape and dist.shape == (n,) and psi.shape[0] == n
    assert cell.min() >= 0 and cell.max() < len(cells)   # every row is filled
    worst = dict(outside=0.0, offplane=0.0, normal=0.0)
    for i in range(n):   # (a)
        d = pr.closest_point_defects(pts[i], nodes[cells[cell[i]]], q[i])
        for k in worst:
            worst[k] = max(worst[k], d[k])
    b = np.abs(dist - np.linalg.norm(pts - q, axis=1)).max()   # (b)
    _, _, _, ref_dist = pr.brute_force(nodes, cells, pts)
    cgap = (dist - ref_dist).max()   # (c)
    _, _, coords = c.dofs_get()
    rows = np.abs(np.asarray(psi.sum(axis=1)).reshape(-1) - 1.0).max()   # (d)
    rep = np.abs(psi @ coords.reshape(len(coords), -1) - q).max()
    print(f"    n={n} tau={tau:.2e} (a) {worst} (b) {b:.2e} (c) {cgap:.2e} (d) rows {rows:.2e} reproduce {rep:.2e}")
    for k, v in worst.items():
        assert v <= tau, (k, v, tau)
    assert b <= tau
    assert cgap <= tau
    assert rows <= 1e-13
    if order == 1:
        assert psi.data.min() >= 0.0 and psi.data.max() <= 1.0
    assert rep <= tau
    return psi, cell, q, dist


def _lowest_incident(cells, n_nodes):
    low = np.full(n_nodes, len(cells), dtype=np.int64)
    for k in range(cells.shape[1]):
        np.minimum.at(low, cells[:, k], np.arange(len(cells)))
    return low


def _check_nodes(c, nodes, cells, order):
    """every node: dist == 0.0, q == p bit for bit, the lowest reference id among the incident cells, the Psi row exactly 1.0 at the node's DOF"""
    psi, cell, q, dist = _check(c, nodes, cells, nodes, order)
    assert np.array_equal(dist, np.zeros(len(nodes))) and np.array_equal(q, nodes)
    assert np.array_equal(cell, _lowest_incident(cells, len(nodes)))
    dofs, _, _ = c.dofs_get()
    psi = psi.tocsr()
    psi.eliminate_zeros()
    assert psi.nnz == len(nodes) and np.array_equal(psi.data, np.ones(len(nodes)))
    local = np.argmax(cells[cell] == np.arange(len(nodes))[:, None], axis=1)   # (the vertex DOFs come first in a row of the DOF table)
    assert np.array_equal(psi.indices, dofs[cell, local])


def _normals(nodes, cells):
    n = np.cross(nodes[cells[:, 1]] - nodes[cells[:, 0]], nodes[cells[:, 2]] - nodes[cells[:, 0]])
    return n / np.linalg.norm(n, axis=1)[:, None]


def _mean_edge(nodes, cells):
    return float(np.mean([np.linalg.norm(nodes[cells[:, i]] - nodes[cells[:, j]], axis=1).mean() for i in range(cells.shape[1]) for j in range(i)]))


def _surface_points(nodes, cells, which):
    h, nrm = _mean_edge(nodes, cells), _normals(nodes, cells)
    lo, hi = nodes.min(axis=0), nodes.max(axis=0)
    if which == "barycentres":
        bc = nodes[cells].mean(axis=1)
        return np.concatenate([bc + 0.3 * h * nrm, bc - 0.3 * h * nrm])
    if which == "edges":
        e = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]])
        key, first = np.unique(np.sort(e, axis=1), axis=0, return_index=True)
        mid = 0.5 * (nodes[key[:, 0]] + nodes[key[:, 1]])
        sign = np.where(np.arange(len(key)) % 2 == 0, 1.0, -1.0)[:, None]
        return mid + 0.25 * h * sign * nrm[first % len(cells)]
    if which == "box":
        w = hi - lo
        return np.random.default_rng(21).uniform(lo - 0.25 * w, hi + 0.25 * w, (200, 3))   # the bounding box widened by 50 %
    if which == "far":
        return (0.5 * (lo + hi) + 10.0 * np.linalg.norm(hi - lo) * np.array([0.6, -0.48, 0.64]))[None, :]   # 10 box diameters away
    if which == "centre":
        return (0.5 * (lo + hi))[None, :]
    raise KeyError(which)


# ---- 1. one cell, one point per Voronoi region, answers known by construction ----------------------------------------------------------------
ONE = {"seg1": np.array([[0.25], [1.5]]), "seg2": np.array([[0.0, 0.5], [2.0, 1.5]]),
       "acute": np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 1.0], [1.5, 3.0, 2.0]]), "obtuse": np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.5], [0.5, 0.5, 1.0]]),
       "tet": np.array([[0.0, 0.0, 0.0], [1.0, 0.125, 0.0], [0.25, 1.0, 0.125], [0.125, 0.25, 1.0]])}


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", list(ONE))
def test_one_cell_every_voronoi_region(env, name, order):
    capi, _ = env
    X = ONE[name]
    cells = np.arange(len(X), dtype=np.int32)[None, :]
    c = _ctx(capi, X, cells, np.ones(len(X), dtype=np.uint8), order)
    regions = pr.region_points(X)
    assert len(regions) == 2 ** len(X) - 1
    pts = np.array([r[1] for r in regions])
    psi, cell, q, dist = _check(c, X, cells, pts, order)
    tau = _tau(X, pts)
    dofs, _, _ = c.dofs_get()
    for i, (rname, p, q_known, lam_known, S) in enumerate(regions):
        assert cell[i] == 0
        assert np.abs(q[i] - q_known).max() <= tau and abs(dist[i] - np.linalg.norm(p - q_known)) <= tau, rname
        if len(S) == 1:   # a vertex region returns the vertex bit for bit, and a unit row
            assert np.array_equal(q[i], X[S[0]]), rname
            row = psi.getrow(i).toarray().reshape(-1)
            assert row[dofs[0, S[0]]] == 1.0 and np.count_nonzero(row) == 1
        if order == 1:
            row = psi.getrow(i).toarray().reshape(-1)[dofs[0, :len(X)]]
            assert np.abs(row - lam_known).max() <= 1e-12 and tuple(np.nonzero(row > 0)[0]) == S, rname   # the region hit is the one constructed
    c.close()


# ---- 2. the reference's surface fixture -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("which", ["nodes", "barycentres", "edges", "box", "far", "centre"])
def test_surface_fixture(env, surface, which, order):
    capi, _ = env
    nodes, cells, bnd = surface
    c = _ctx(capi, nodes, cells, bnd, order)
    if which == "nodes":
        _check_nodes(c, nodes, cells, order)
    else:
        _check(c, nodes, cells, _surface_points(nodes, cells, which), order)
    c.close()


# ---- 3. a closed sphere: the centre (every cell nearly equidistant: the whole grid is scanned), inside and outside ------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_sphere_centre_and_radii(env, order):
    capi, meshgen = env
    nodes, cells, bnd = meshgen.unit_sphere_surface(3)
    c = _ctx(capi, nodes, cells, bnd, order)
    d = np.random.default_rng(5).standard_normal((60, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = np.concatenate([np.zeros((1, 3)), 0.5 * d, 2.0 * d])
    _, cell, q, dist = _check(c, nodes, cells, pts, order)
    assert 0.9 < dist[0] < 1.0 and np.all(np.abs(dist[1:61] - 0.5) < 0.05) and np.all(np.abs(dist[61:] - 1.0) < 0.05)
    c.close()


# ---- 4. internal numbering differs from the reference numbering; repeatability ----------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_permuted_height_field(env, order):
    capi, meshgen = env
    nodes, cells, bnd = meshgen.height_field_surface(12, permute=True)
    c = _ctx(capi, nodes, cells, bnd, order)
    _check_nodes(c, nodes, cells, order)
    pts = _surface_points(nodes, cells, "barycentres")[::3]
    a = c.project(pts)
    b = c.project(pts)
    cl = c.clone()
    d = cl.project(pts)
    for other in (b, d):
        assert abs(a[0] - other[0]).max() == 0.0 and all(np.array_equal(x, y) for x, y in zip(a[1:], other[1:]))
    _check(c, nodes, cells, pts, order, out=a)
    cl.close()
    c.close()


# ---- 5. grids with an axis of zero extent -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", ["sheet", "line"])
def test_flat_axis(env, kind, order):
    capi, meshgen = env
    rng = np.random.default_rng(8)
    if kind == "sheet":   # a horizontal planar sheet uploaded as a surface
        n2, cells, bnd = meshgen.unit_square(5)
        nodes = np.ascontiguousarray(np.column_stack([n2, np.full(len(n2), 0.25)]))
        pts = np.concatenate([rng.uniform(-0.5, 1.5, (80, 3)), np.column_stack([rng.uniform(0, 1, (20, 2)), np.full(20, 0.25)]),
                              [[0.5, 0.5, 30.0], [-20.0, 0.3, 0.25]]])
    else:   # a network on one horizontal line
        x = np.sort(np.concatenate([[0.0, 3.0], rng.uniform(0.1, 2.9, 9)]))
        nodes = np.ascontiguousarray(np.column_stack([x, np.full(len(x), 0.5)]))
        cells = np.stack([np.arange(len(x) - 1), np.arange(1, len(x))], axis=1).astype(np.int32)
        bnd = np.zeros(len(x), dtype=np.uint8)
        bnd[[0, -1]] = 1
        pts = np.concatenate([rng.uniform(-1.0, 4.0, (60, 2)), np.column_stack([rng.uniform(0, 3, 20), np.full(20, 0.5)]), [[1.5, 40.0], [-30.0, 0.5]]])
    c = _ctx(capi, nodes, cells, bnd, order)
    _, cell, q, dist = _check(c, nodes, cells, pts, order)
    if kind == "sheet":
        assert np.abs(q[:, 2] - 0.25).max() <= 1e-12
        assert np.abs(q[:, :2] - np.clip(pts[:, :2], 0.0, 1.0)).max() <= 1e-12
    else:
        assert np.abs(q - np.column_stack([np.clip(pts[:, 0], 0.0, 3.0), np.full(len(pts), 0.5)])).max() <= 1e-12
    _check_nodes(c, nodes, cells, order)
    c.close()


# ---- 6. planar and volume meshes: inside = fdapde_eval_pointwise, outside = the clipped point ----------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", ["square", "cube"])
def test_planar_and_volume(env, kind, order):
    capi, meshgen = env
    nodes, cells, bnd = meshgen.unit_square(6) if kind == "square" else meshgen.unit_cube(3)
    N = nodes.shape[1]
    c = _ctx(capi, nodes, cells, bnd, order)
    rng = np.random.default_rng(13)
    pick = rng.integers(0, len(cells), 150)
    lam = rng.dirichlet(np.ones(N + 1), 150)
    lam = np.maximum(lam, 0.01)
    lam /= lam.sum(axis=1)[:, None]   # all barycentric coordinates >= 0.01 / (1 + 0.01 (N + 1)) > 1e-6
    inside = np.einsum("ij,ijk->ik", lam, nodes[cells[pick]])
    psi, cell, q, dist = _check(c, nodes, cells, inside, order)
    epsi, _, ecell = c.eval_pointwise(inside)
    assert np.array_equal(cell, ecell) and np.array_equal(cell, pick)
    assert np.array_equal(q, inside) and np.array_equal(dist, np.zeros(len(inside)))
    assert abs(psi - epsi).max() <= 1e-12
    outside = rng.uniform(-1.0, 2.0, (150, N))
    outside = outside[((outside < 0) | (outside > 1)).any(axis=1)]
    _, _, q, dist = _check(c, nodes, cells, outside, order)
    assert np.abs(q - np.clip(outside, 0.0, 1.0)).max() <= _tau(nodes, outside)
    if kind == "square":   # (a node of a tetrahedron may be taken as an inside point: its coordinates are then 1 and 0 to rounding only)
        _check_nodes(c, nodes, cells, order)
    c.close()


# ---- 7. 1-D meshes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", ["network", "star", "interval"])
def test_one_dimensional_meshes(env, network, kind, order):
    capi, meshgen = env
    rng = np.random.default_rng(17)
    if kind == "network":
        nodes, cells, bnd = network
    elif kind == "star":
        nodes, cells, bnd = meshgen.star(5, [1.0, 0.7, 1.3, 0.9, 1.1], k=3)
    else:
        nodes, cells, bnd = meshgen.interval(8, jitter=0.3)
    nodes = np.asarray(nodes, dtype=float).reshape(len(nodes), -1)
    N = nodes.shape[1]
    c = _ctx(capi, nodes, cells, bnd, order)
    lo, hi = nodes.min(axis=0), nodes.max(axis=0)
    t = rng.uniform(0.05, 0.95, (len(cells), 1))
    on = (1 - t) * nodes[cells[:, 0]] + t * nodes[cells[:, 1]]   # points of the segments (to rounding)
    around = rng.uniform(lo - 0.3 * (hi - lo) - 0.1, hi + 0.3 * (hi - lo) + 0.1, (120, N))
    pts = np.concatenate([on, around])
    _, cell, q, dist = _check(c, nodes, cells, pts, order)
    _, _, found = c.eval_pointwise(pts)
    assert (found[:len(on)] >= 0).all()
    assert dist[found >= 0].max() <= _tau(nodes, pts)   # what point location finds, projection finds at distance 0 (to tau)
    if kind == "interval":
        _, cell, q, dist = c.project(np.array([[-0.5], [1.7]]))
        assert np.array_equal(q, [[0.0], [1.0]]) and np.allclose(dist, [0.5, 0.7], atol=1e-15)
        assert np.array_equal(cell, [np.nonzero((nodes[cells] == 0.0).any(axis=(1, 2)))[0][0], np.nonzero((nodes[cells] == 1.0).any(axis=(1, 2)))[0][0]])
    if kind == "star":   # beyond the leaf of every arm, along the arm: the leaf node itself
        leaves = np.nonzero(bnd)[0]
        beyond = nodes[leaves] * 1.5
        _, cell, q, dist = c.project(beyond)
        assert np.array_equal(q, nodes[leaves])
        assert all(leaves[i] in cells[cell[i]] for i in range(len(leaves)))
    _check_nodes(c, nodes, cells, order)
    c.close()


# ---- 8. projected metres: scaled by 100 and shifted by (5e5, 4.5e6, 100) -------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_scaled_and_shifted_fixture(env, surface, order):
    capi, meshgen = env
    n0, cells, bnd = surface
    nodes = meshgen.transform(n0, scale=100, shift=(5e5, 4.5e6, 100))
    c = _ctx(capi, nodes, cells, bnd, order)
    pts = np.concatenate([_surface_points(nodes, cells, "barycentres")[::4], _surface_points(nodes, cells, "box")[:100], nodes[::5]])
    _check(c, nodes, cells, pts, order)
    c.close()


# ---- 9. shapes; a two-rank context ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pts", [1, 255, 257])
def test_point_counts(env, surface, n_pts):
    capi, _ = env
    nodes, cells, bnd = surface
    c = _ctx(capi, nodes, cells, bnd, 1)
    allp = _surface_points(nodes, cells, "barycentres")
    full = c.project(allp[:300])
    part = _check(c, nodes, cells, allp[:n_pts], 1)
    assert abs(full[0][:n_pts] - part[0]).max() == 0.0 and all(np.array_equal(x[:n_pts], y) for x, y in zip(full[1:], part[1:]))
    c.close()


@pytest.mark.parametrize("order", ORDERS)
def test_two_rank_context_equals_one_device(env, order):
    capi, meshgen = env
    nodes, cells, bnd = meshgen.unit_square(12)
    pts = np.random.default_rng(4).uniform(-0.3, 1.3, (200, 2))
    one = _ctx(capi, nodes, cells, bnd, order)
    grp = _ctx(capi, nodes, cells, bnd, order, devices=[0, 0])
    a, b = one.project(pts), grp.project(pts)
    assert abs(a[0] - b[0]).max() == 0.0 and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    _check(one, nodes, cells, pts, order, out=a)
    grp.close()
    one.close()


# ---- 10. argument errors ----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(env, surface):
    capi, _ = env
    nodes, cells, bnd = surface
    c = capi.Context(device=0)
    c.mesh_upload(nodes, cells, bnd)
    with pytest.raises(capi.FdapdeError) as e:
        c.project(nodes[:3])
    assert e.value.status == capi.ENOTINIT
    c.dofs_build(1)
    bad = nodes[:5].copy()
    bad[3, 1] = np.nan
    with pytest.raises(capi.FdapdeError) as e:
        c.project(bad)
    assert e.value.status == capi.EINVAL and "non-finite" in str(e.value)
    bad[3, 1] = np.inf
    with pytest.raises(capi.FdapdeError) as e:
        c.project(bad)
    assert e.value.status == capi.EINVAL
    import ctypes as C

    one = np.zeros(3)
    cid, d = np.zeros(1, dtype=np.int32), np.zeros(1)
    assert c.lib.fdapde_project(c._ctx, C.c_int64(0), capi._dp(one), capi._ip(cid), capi._dp(one), capi._dp(d), None) == capi.EINVAL
    assert c.lib.fdapde_project(c._ctx, C.c_int64(1), None, capi._ip(cid), capi._dp(one), capi._dp(d), None) == capi.EINVAL
    assert c.lib.fdapde_project(c._ctx, C.c_int64(1), capi._dp(one), None, capi._dp(one), capi._dp(d), None) == capi.EINVAL
    pts = _surface_points(nodes, cells, "box")
    with_v, without = c.project(pts), c.project(pts, values=False)
    assert without[0] is None and all(np.array_equal(x, y) for x, y in zip(with_v[1:], without[1:]))
    c.close()
