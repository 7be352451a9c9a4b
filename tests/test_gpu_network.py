"""1-D meshes on the device -- intervals (Triangulation<1,1>) and linear networks in the plane (Triangulation<1,2>): fdapde_mesh_upload(ctx, 1, N, ...)
and everything downstream of it, against the float64 segment assembler of tests/segment_ref.py (pinned to closed-form element matrices by
tests/test_segment_cpu.py) and scipy's sparse LU.

Fixtures: the reference's network test/data/mesh/network (201 nodes, 200 segments), seeded intervals, stars and street grids (meshgen.interval,
meshgen.star, meshgen.street_grid).
Bars: entries <= 1e-13 max(1, |.|max); solutions <= 1e-8 relative to spsolve; symmetric operators bitwise symmetric; runs bitwise reproducible."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import segment_ref as sg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETOL = 1e-13
STOL = 1e-8


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, meshgen


@pytest.fixture(scope="module")
def network():
    return sg.load_network_fixture(ROOT)


def _ctx(capi, nodes, cells, bnd, order):
    c = capi.Context(device=0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(order)
    return c


def _ops(m, N, rng=None, rows=None):
    """the operator set of tests/test_gpu_surface.py with N-dimensional tensors and vectors (+ space-varying ones when rows is given)"""
    K = np.array([[2.0, 0.3], [0.3, 1.0]])[:N, :N]
    b = np.array([0.7, -0.2])[:N]
    Kn = K + np.array([[0.0, 0.4], [-0.2, 0.0]])[:N, :N] + (np.array([[0.25]]) if N == 1 else 0.0)
    ops = {"neg_laplacian": -m.laplacian(), "mass": m.reaction(1.0), "adr": -m.laplacian() + m.advection(b) + m.reaction(1.5),
           "diffusion": m.diffusion(K) + 0.5 * m.reaction(2.0), "laplacian_minus_dt": m.laplacian() - m.dt(),
           "diffusion_nonsym": m.diffusion(Kn) + m.advection(b) + m.reaction(0.5), "diffusion_nonsym_mirrored": m.diffusion(Kn) + m.reaction(0.5)}
    if rows is not None:
        A = rng.standard_normal((rows, N, N)) * 0.3
        Kq = np.einsum("rij,rkj->rik", A, A) + np.eye(N)[None]
        bq = rng.standard_normal((rows, N))
        cq = rng.uniform(0.5, 2.0, rows)
        ops["var_k"] = -m.laplacian() + m.diffusion_field(Kq.reshape(rows, N * N))
        ops["var_kbc"] = m.diffusion_field(Kq.reshape(rows, N * N)) + m.advection_field(bq) + m.reaction_field(cq)
        ops["var_c"] = -m.laplacian() + m.reaction_field(cq)
        ops["var_b_const_k"] = m.diffusion(K) + m.advection_field(bq)
        if N == 2:
            S = rng.uniform(-0.4, 0.4, (rows, N, N))
            Kqn = (Kq + (S - np.transpose(S, (0, 2, 1)))).reshape(rows, N * N)
            ops["var_k_nonsym_mirrored"] = m.diffusion_field(Kqn) + m.reaction_field(cq)
            ops["var_k_nonsym_adv"] = m.diffusion_field(Kqn) + m.advection(b) + m.reaction(1.0)
    return ops


def _dev_csr(c, which):
    rp, ci = c.pattern_get()
    v = c.matrix_values(which)
    n = rp.size - 1
    return sp.csr_matrix((v, ci, rp), shape=(n, n))


def _ref_solution(nodes, cells, bnd, order, op_o, fq, g):
    dt, dbnd, nd = sg.dofs(cells, len(nodes), bnd, order)
    A = sg.assemble(nodes, cells, dt, nd, order, op_o)
    b = sg.forcing(nodes, cells, dt, nd, order, fq)
    if g is not None:
        A, b = sg.set_dirichlet(A, b, dbnd, g)
    return spla.spsolve(A.tocsc(), b)


def _meshes(meshgen, network):
    return {"fixture": network, "interval": meshgen.interval(37, 0.0, 2.0, jitter=0.3, permute=True, seed=5),
            "grid": meshgen.street_grid(6, 5, k=3, seed=11, drop=0.15)}


# ---- 1. DOF table, boundary DOFs, coordinates, quadrature nodes -------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("which", ["fixture", "interval", "grid"])
def test_dof_table_and_coordinates(env, network, order, which):
    capi, meshgen = env
    nodes, cells, bnd = _meshes(meshgen, network)[which]
    c = _ctx(capi, nodes, cells, bnd, order)
    dofs, dbnd, coords = c.dofs_get()
    rd, rb, nd = sg.dofs(cells, len(nodes), bnd, order)
    assert c.sizes()["n_dofs"] == nd and np.array_equal(dofs, rd) and np.array_equal(dbnd, rb)
    assert int(dbnd.sum()) == int(bnd.sum())
    N = nodes.reshape(len(nodes), -1).shape[1]
    assert coords.shape == (nd, N) and np.array_equal(coords, sg.dof_coords(nodes, cells, order))
    qn = c.quadrature_nodes()
    assert np.abs(qn - sg.quadrature_nodes(nodes, cells, order)).max() <= 1e-15 * max(1.0, np.abs(qn).max())
    c.close()


# ---- 2. device set-up = host set-up ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("which", ["fixture", "interval", "grid", "star2000", "grid_large"])
def test_device_setup_equals_host_setup(env, network, order, which, monkeypatch):
    capi, meshgen = env
    if which == "star2000":
        mesh = meshgen.star(2000, np.random.default_rng(1).uniform(0.5, 2.0, 2000), k=2, permute=True)
    elif which == "grid_large":
        mesh = meshgen.street_grid(60, 50, k=8, seed=3, drop=0.1)
    else:
        mesh = _meshes(meshgen, network)[which]
    monkeypatch.setenv("FDAPDE_SETUP_CHECK", "1")
    c = _ctx(capi, *mesh, order)   # (a mismatch fails fdapde_dofs_build)
    dev = (c.dofs_get(), c.pattern_get())
    c.close()
    monkeypatch.delenv("FDAPDE_SETUP_CHECK")
    monkeypatch.setenv("FDAPDE_SETUP", "host")
    h = _ctx(capi, *mesh, order)
    host = (h.dofs_get(), h.pattern_get())
    h.close()
    for a, b in zip(dev[0] + dev[1], host[0] + host[1]):
        assert np.array_equal(a, b)


# ---- 3. entry parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("which", ["fixture", "interval", "grid"])
def test_entry_parity(env, network, order, which):
    from oracle import oracle as o

    capi, meshgen = env
    nodes, cells, bnd = _meshes(meshgen, network)[which]
    N = nodes.reshape(len(nodes), -1).shape[1]
    nq = sg.tables(order)[0].size
    rows = nq * cells.shape[0]
    c = _ctx(capi, nodes, cells, bnd, order)
    rp, ci = c.pattern_get()
    dt, _, nd = sg.dofs(cells, len(nodes), bnd, order)
    ops_c, ops_o = _ops(capi, N, np.random.default_rng(9), rows), _ops(o, N, np.random.default_rng(9), rows)
    qn = c.quadrature_nodes()
    fq = np.sin(3 * qn[:, 0]) + (qn[:, 1] if N == 2 else 0.0)
    for name in ops_c:
        c.set_operator(ops_c[name])
        c.set_forcing(fq)
        c.init()
        got = c.matrix_values(capi.MAT_STIFF)
        ref = sg.values_in_pattern(sg.assemble(nodes, cells, dt, nd, order, ops_o[name]), rp, ci)
        assert np.abs(got - ref).max() <= ETOL * max(1.0, np.abs(ref).max()), (name, np.abs(got - ref).max())
        if not sg.has_advection(ops_o[name]):
            A = _dev_csr(c, capi.MAT_STIFF)
            assert (A != A.T).nnz == 0, name   # bitwise symmetric
        mass = c.matrix_values(capi.MAT_MASS)
        mref = sg.values_in_pattern(sg.assemble(nodes, cells, dt, nd, order, o.reaction(1.0)), rp, ci)
        assert np.abs(mass - mref).max() <= ETOL * max(1.0, np.abs(mref).max())
        fref = sg.forcing(nodes, cells, dt, nd, order, fq)
        assert np.abs(c.force() - fref).max() <= ETOL * max(1.0, np.abs(fref).max())
    c.close()


# ---- 4. invariance: rigid motions of the plane, segment orientation -------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_rigid_motion_and_orientation_invariance(env, network, order):
    capi, _ = env
    nodes, cells, bnd = network
    th = 0.83
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    moved = nodes @ R.T + np.array([3.0, -7.5])
    flip = np.random.default_rng(2).random(cells.shape[0]) < 0.5
    flipped = cells.copy()
    flipped[flip] = flipped[flip][:, ::-1]
    op = -capi.laplacian() + capi.reaction(2.0)
    out = []
    for nn, cc in ((nodes, cells), (moved, cells), (nodes, flipped)):
        c = _ctx(capi, nn, cc, bnd, order)
        c.set_operator(op)
        c.init()
        out.append((_dev_csr(c, capi.MAT_STIFF).toarray(), _dev_csr(c, capi.MAT_MASS).toarray(), c.dofs_get()[0]))
        c.close()
    A0 = out[0][0]
    assert np.abs(out[1][0] - A0).max() <= ETOL * np.abs(A0).max() and np.abs(out[1][1] - out[0][1]).max() <= ETOL * np.abs(out[0][1]).max()
    assert np.array_equal(out[1][2], out[0][2])
    # re-oriented segments: the same matrices (the midpoint DOF ids are by cell in both), the vertex columns of the DOF table swapped where flipped
    assert np.abs(out[2][0] - A0).max() <= ETOL * np.abs(A0).max() and np.abs(out[2][1] - out[0][1]).max() <= ETOL * np.abs(out[0][1]).max()
    assert np.array_equal(out[2][2][:, :2], np.where(flip[:, None], out[0][2][:, 1::-1], out[0][2][:, :2]))
    assert order == 1 or np.array_equal(out[2][2][:, 2], out[0][2][:, 2])


# ---- 5. Kirchhoff exactness on stars -------------------------------------------------------------------------------------------------
# (hubs far beyond one team pass of the SpMV, served by its long-row loop: 5000 arms at P1 -> a row of 5001 entries, 3000 at P2 -> 6001)
@pytest.mark.parametrize("order,arms,env_vars", [(1, 3, {}), (2, 3, {}), (1, 7, {}), (2, 7, {}), (1, 2000, {}), (2, 2000, {}), (1, 5000, {}), (2, 3000, {}),
                                                  (2, 3000, {"FDAPDE_SETUP": "host"}),
                                                  (1, 5000, {"FDAPDE_SETUP_CHECK": "1"})])
def test_star_kirchhoff_exact(env, order, arms, env_vars, monkeypatch):
    capi, meshgen = env
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(arms)
    L = rng.uniform(0.5, 2.0, arms)
    nodes, cells, bnd = meshgen.star(arms, L, k=3)
    g_leaf = rng.uniform(-1.0, 1.0, arms)
    cval = np.sum((g_leaf + L ** 2 / 2) / L) / np.sum(1 / L)
    c = _ctx(capi, nodes, cells, bnd, order)
    _, dbnd, coords = c.dofs_get()
    r = np.linalg.norm(coords, axis=1)
    ang = np.mod(np.round(np.arctan2(coords[:, 1], coords[:, 0]) / (2 * np.pi / arms)).astype(int), arms)
    # u on arm i at distance s from the centre: c + (g_i - c + L_i^2 / 2) s / L_i - s^2 / 2   (-u'' = 1, u(0) = c, u(L_i) = g_i)
    exact = cval + (g_leaf[ang] - cval + L[ang] ** 2 / 2) * r / L[ang] - r ** 2 / 2
    exact[r < 1e-14] = cval
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(sg.tables(order)[0].size * cells.shape[0]))
    c.set_dirichlet(np.where(dbnd == 1, exact, 0.0))
    c.init()
    info = c.solve(rtol=1e-13, maxit=20000)
    assert info.converged == 1
    u = c.solution()
    assert np.abs(u - exact).max() <= 1e-10 * np.abs(exact).max(), np.abs(u - exact).max()
    c.close()


# ---- 6. convergence on [0, 1] --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_convergence_on_the_unit_interval(env, order):
    capi, meshgen = env
    errs, hs = [], []
    for n in (16, 32, 64, 128):
        nodes, cells, bnd = meshgen.interval(n, permute=True, seed=n)   # (uniform: the rates of nested meshes)
        c = _ctx(capi, nodes, cells, bnd, order)
        qn = c.quadrature_nodes()[:, 0]
        c.set_operator(-capi.laplacian())
        c.set_forcing(np.pi ** 2 * np.sin(np.pi * qn))
        c.set_dirichlet(np.zeros(c.sizes()["n_dofs"]))
        c.init()
        assert c.solve(rtol=1e-14, maxit=20000).converged == 1
        u = c.solution()
        dt, _, _ = sg.dofs(cells, len(nodes), bnd, order)
        # L2 error by a 5-point Gauss rule per cell
        gp, gw = np.polynomial.legendre.leggauss(5)
        t = (gp + 1) / 2
        x0, x1 = nodes[cells[:, 0], 0], nodes[cells[:, 1], 0]
        x = x0[:, None] + (x1 - x0)[:, None] * t[None, :]
        uh = np.einsum("mqi,mi->mq", sg.basis_at(order, t)[None].repeat(len(cells), 0), u[dt])
        e2 = np.sum(np.abs(x1 - x0)[:, None] * gw[None, :] / 2 * (uh - np.sin(np.pi * x)) ** 2)
        errs.append(np.sqrt(e2)), hs.append(1.0 / n)
        c.close()
    rates = np.diff(np.log(errs)) / np.diff(np.log(hs))
    assert rates.min() >= (1.9 if order == 1 else 2.9), rates


# ---- 7. every solver method against spsolve ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("which", ["fixture", "grid50k"])
def test_every_method(env, network, order, which):
    from oracle import oracle as o

    capi, meshgen = env
    nodes, cells, bnd = network if which == "fixture" else meshgen.street_grid(50, 50, k=10 if order == 1 else 5, seed=8, drop=0.1)
    c = _ctx(capi, nodes, cells, bnd, order)
    _, _, coords = c.dofs_get()
    qn = c.quadrature_nodes()
    g = coords[:, 0] * 0.1 + coords[:, 1] * 0.2
    fq = np.cos(qn[:, 0]) + qn[:, 1]
    op_c, op_o = -capi.laplacian() + capi.reaction(1.0), -o.laplacian() + o.reaction(1.0)
    ref = _ref_solution(nodes, cells, bnd, order, op_o, fq, g)
    methods = ["AUTO", "CG", "CG_SR", "CG_FUSED", "BICGSTAB", "GMRES", "AMG"] + (["DENSE"] if which == "fixture" else []) + (["PMG"] if order == 2 else [])
    for meth in methods:
        c.set_operator(op_c)
        c.set_forcing(fq)
        c.set_dirichlet(g)
        c.init()
        info = c.solve(method=getattr(capi, "SOLVER_" + meth), rtol=1e-12, maxit=200000)
        assert info.converged == 1, meth
        u = c.solution()
        assert np.linalg.norm(u - ref) / np.linalg.norm(ref) <= STOL, (meth, np.linalg.norm(u - ref) / np.linalg.norm(ref))
    c.close()


# ---- 8. parabolic stepper, factor-once handle, lumping, cell integrals --------------------------------------------------------------
def test_parabolic_on_the_network(env, network):
    from oracle import oracle as o

    capi, _ = env
    nodes, cells, bnd = network
    order = 1
    c = _ctx(capi, nodes, cells, bnd, order)
    times = np.linspace(0.0, 0.2, 21)
    nq = sg.tables(order)[0].size
    c.set_operator(capi.dt() - capi.laplacian())
    c.set_forcing(np.zeros((nq * cells.shape[0], times.size)))
    c.init()
    u0 = np.sin(nodes[:, 0]) + nodes[:, 1]
    sol, info = c.solve_parabolic(times, u0, rtol=1e-12)
    dt_, _, nd = sg.dofs(cells, len(nodes), bnd, order)
    A = sg.assemble(nodes, cells, dt_, nd, order, o.dt() - o.laplacian())
    Mm = sg.assemble(nodes, cells, dt_, nd, order, o.reaction(1.0))
    dt = times[1] - times[0]
    lu = spla.splu((Mm / dt + A).tocsc())
    ref = np.zeros_like(sol)
    ref[:, 0] = u0
    for i in range(times.size - 1):
        ref[:, i + 1] = lu.solve(Mm @ ref[:, i] / dt)
    assert np.linalg.norm(sol - ref) / np.linalg.norm(ref) <= STOL
    c.close()


@pytest.mark.parametrize("order", [1, 2])
def test_factor_once_handle_lumping_and_cell_integrals(env, network, order):
    from oracle import oracle as o

    capi, _ = env
    nodes, cells, bnd = network
    c = _ctx(capi, nodes, cells, bnd, order)
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.init()
    dt, _, nd = sg.dofs(cells, len(nodes), bnd, order)
    A = sg.assemble(nodes, cells, dt, nd, order, -o.laplacian() + o.reaction(1.0))
    Mm = sg.assemble(nodes, cells, dt, nd, order, o.reaction(1.0))
    rng = np.random.default_rng(4)
    for which, R in ((capi.MAT_STIFF, A), (capi.MAT_MASS, Mm)):
        c.lin_compute(which, symmetric=True)
        for ncol in (1, 8):
            B = rng.standard_normal((nd, ncol)) if ncol > 1 else rng.standard_normal(nd)
            X, info = c.lin_solve(B, rtol=1e-12)
            ref = spla.spsolve(R.tocsc(), B)
            assert np.linalg.norm(X - ref) / np.linalg.norm(ref) <= STOL, (which, ncol)
    assert np.abs(c.lump(capi.MAT_MASS) - np.asarray(Mm.sum(axis=1)).ravel()).max() <= ETOL * np.abs(Mm).max()
    meas = np.zeros(cells.shape[0])
    pint = np.zeros((cells.shape[0], c.sizes()["n_basis"]))
    c._check(c.lib.fdapde_cell_integrals(c._ctx, meas.ctypes.data_as(C.POINTER(C.c_double)), pint.ctypes.data_as(C.POINTER(C.c_double))))
    h = sg.geometry(nodes, cells)[2]
    assert np.abs(meas - h).max() <= 1e-15 * h.max()
    w = np.array([0.5, 0.5]) if order == 1 else np.array([1 / 6, 1 / 6, 2 / 3])
    assert np.abs(pint - h[:, None] * w[None, :]).max() <= 1e-14 * h.max()
    c.close()


# ---- 9. point evaluation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("which", ["fixture", "interval", "grid", "exact_grid"])
def test_eval_pointwise(env, network, order, which):
    capi, meshgen = env
    meshes = _meshes(meshgen, network)
    meshes["exact_grid"] = meshgen.street_grid(8, 8, k=4, drop=0.2, jitter=0.0, seed=6)
    nodes, cells, bnd = meshes[which]
    nodes2 = nodes.reshape(len(nodes), -1)
    N = nodes2.shape[1]
    rng = np.random.default_rng(13)
    # random points on segments (away from the ends), every vertex, points off the network
    k = rng.integers(0, cells.shape[0], 300)
    t = rng.uniform(0.01, 0.99, 300)
    on = nodes2[cells[k, 0]] + t[:, None] * (nodes2[cells[k, 1]] - nodes2[cells[k, 0]])
    pts = [on, nodes2]
    if N == 2:
        n = np.stack([-(nodes2[cells[k, 1]] - nodes2[cells[k, 0]])[:, 1], (nodes2[cells[k, 1]] - nodes2[cells[k, 0]])[:, 0]], axis=1)
        n /= np.linalg.norm(n, axis=1)[:, None]
        off = on + n * rng.uniform(1e-6, 1e-3, 300)[:, None]
        # (an off point may still lie on another segment: the reference rule decides, not the construction)
        pts.append(off)
    else:
        pts.append(np.array([[nodes2.min() - 1e-3], [nodes2.max() + 1e-5]]))
    if which == "exact_grid":   # exact coordinates on the lattice: crossings, quarter points
        pts.append(np.array([[1.0, 2.0], [1.25, 3.0], [4.0, 0.5], [0.75, 8.0]]))
    locs = np.concatenate(pts, axis=0)
    c = _ctx(capi, nodes, cells, bnd, order)
    psi, _, got = c.eval_pointwise(locs)
    ref, xi = sg.locate(nodes2, cells, locs)
    assert np.array_equal(got, ref)
    assert np.all(got[: len(on) + len(nodes2)] >= 0)
    n_off = len(pts[2])
    assert np.mean(got[len(on) + len(nodes2): len(on) + len(nodes2) + n_off] == -1) >= 0.9   # (an off point may lie on another segment)
    if which == "exact_grid":
        assert np.all(got[-4:] >= 0)
    # the vertices resolve to the lowest-id segment meeting there
    vid = np.arange(len(nodes2))
    low = np.full(len(nodes2), cells.shape[0])
    np.minimum.at(low, cells[:, 0], np.arange(cells.shape[0]))
    np.minimum.at(low, cells[:, 1], np.arange(cells.shape[0]))
    assert np.array_equal(got[len(on):len(on) + len(nodes2)], low[vid])
    dt, _, nd = sg.dofs(cells, len(nodes), bnd, order)
    ok = ref >= 0
    vals = sg.basis_at(order, xi[ok])
    dense = psi.toarray()[ok]
    expect = np.zeros_like(dense)
    np.add.at(expect, (np.repeat(np.arange(ok.sum()), dt.shape[1]), dt[ref[ok]].reshape(-1)), vals.reshape(-1))
    assert np.abs(dense - expect).max() <= 1e-12
    c.close()


# ---- 10. determinism and clone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_determinism_and_clone(env, order):
    capi, meshgen = env
    nodes, cells, bnd = meshgen.street_grid(20, 20, k=4, seed=5, drop=0.1)
    runs = []
    for _ in range(2):
        c = _ctx(capi, nodes, cells, bnd, order)
        _, _, coords = c.dofs_get()
        qn = c.quadrature_nodes()
        c.set_operator(capi.diffusion(np.diag([1.0, 2.0])) + capi.reaction(1.0))
        c.set_forcing(np.sin(qn[:, 0] + qn[:, 1]))
        c.set_dirichlet(coords[:, 1])
        c.init()
        c.solve(rtol=1e-12)
        runs.append((c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS), c.force(), c.solution()))
        if len(runs) == 2:
            d = c.clone()
            d.solve(rtol=1e-12)
            runs.append((d.matrix_values(capi.MAT_STIFF), d.matrix_values(capi.MAT_MASS), d.force(), d.solution()))
            d.close()
        c.close()
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b)


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------
def _status(fn):
    from fdapde_core_amd import capi

    with pytest.raises(capi.FdapdeError) as e:
        fn()
    return e.value.status, str(e.value)


def test_refusals(env, network):
    capi, _ = env
    nodes, cells, bnd = network
    g = capi.Context(devices=[0, 0])
    st, msg = _status(lambda: g.mesh_upload(nodes, cells, bnd))
    assert st == capi.EUNSUPPORTED and "1-D" in msg
    g.close()
    h = capi.Context(0)
    st, msg = _status(lambda: h.mesh_upload(np.concatenate([nodes, np.zeros((len(nodes), 1))], axis=1), cells, bnd))
    assert st == capi.EUNSUPPORTED and "Triangulation<1,2>" in msg   # (1, 3)
    st, msg = _status(lambda: h.mesh_upload(nodes, np.zeros((3, 5), np.int32), bnd))
    assert st == capi.EUNSUPPORTED   # wrong column count
    z = nodes.copy()
    z[cells[5, 1]] = z[cells[5, 0]]
    st, msg = _status(lambda: h.mesh_upload(z, cells, bnd))
    assert st == capi.EINVAL and "zero length" in msg
    iso = np.concatenate([nodes, [[50.0, 50.0]]], axis=0)   # a node on no segment: its DOF would have an empty row
    st, msg = _status(lambda: h.mesh_upload(iso, cells, np.concatenate([bnd, [0]]).astype(np.uint8)))
    assert st == capi.EUNSUPPORTED and "no segment" in msg
    rep = np.concatenate([cells, cells[7:8, ::-1]], axis=0)   # a segment listed twice (either orientation)
    st, msg = _status(lambda: h.mesh_upload(nodes, rep, bnd))
    assert st == capi.EUNSUPPORTED and "twice" in msg
    h.close()
    c = _ctx(capi, nodes, cells, bnd, 1)
    st, msg = _status(lambda: c.topology())
    assert st == capi.EUNSUPPORTED and "1-D" in msg
    c.set_operator(-capi.laplacian())
    for v in (capi.ASSEMBLY_ATOMIC, capi.ASSEMBLY_COLOURED, capi.ASSEMBLY_PARTITIONED, capi.ASSEMBLY_WAVE):
        st, msg = _status(lambda: c.init(assembly=v))
        assert st == capi.EUNSUPPORTED and "row-owner" in msg, v
    c.init()
    st, msg = _status(lambda: c.partition_build(2))
    assert st == capi.EUNSUPPORTED and "1-D" in msg
    c.close()


# ---- 12. fuzz ---------------------------------------------------------------------------------------------------------------------------
def _fuzz_ops(m, rng, rows):
    K = np.diag(rng.uniform(0.5, 2.0, 2))
    K[0, 1] = K[1, 0] = rng.uniform(-0.2, 0.2)
    b = rng.uniform(-1, 1, 2)
    Kn = K + np.array([[0.0, 0.2], [-0.1, 0.0]])
    A = rng.standard_normal((rows, 2, 2)) * 0.3
    Kq = (np.einsum("rij,rkj->rik", A, A) + np.eye(2)[None]).reshape(rows, 4)
    bq, cq = rng.standard_normal((rows, 2)), rng.uniform(0.5, 2.0, rows)
    c = float(rng.uniform(0.5, 2.0))
    return {"lap": -m.laplacian() + m.reaction(c), "diff": -m.diffusion(K) + m.reaction(c), "adr": -m.laplacian() + m.advection(b) + m.reaction(c),
            "nonsym_mirrored": -m.diffusion(Kn) + m.reaction(c), "nonsym_adv": -m.diffusion(Kn) + m.advection(b) + m.reaction(c),
            "var_kbc": -m.diffusion_field(Kq) + m.advection_field(bq) + m.reaction_field(cq), "var_c": -m.laplacian() + m.reaction_field(cq)}


def test_fuzz_random_street_grids(env):
    from oracle import oracle as o

    capi, meshgen = env
    rng = np.random.default_rng(2025)
    worst_e = worst_s = 0.0
    for case in range(40):
        nodes, cells, bnd = meshgen.street_grid(int(rng.integers(2, 12)), int(rng.integers(2, 12)), k=int(rng.integers(1, 6)),
                                                seed=int(rng.integers(1 << 30)), drop=float(rng.uniform(0, 0.3)))
        order = int(rng.integers(1, 3))
        rows = sg.tables(order)[0].size * cells.shape[0]
        s = int(rng.integers(1 << 30))
        names = list(_fuzz_ops(capi, np.random.default_rng(s), rows))
        name = names[int(rng.integers(len(names)))]
        op_c, op_o = _fuzz_ops(capi, np.random.default_rng(s), rows)[name], _fuzz_ops(o, np.random.default_rng(s), rows)[name]
        fq = rng.standard_normal(rows)
        c = _ctx(capi, nodes, cells, bnd, order)
        _, _, coords = c.dofs_get()
        g = coords.sum(axis=1) if bnd.any() else None
        c.set_operator(op_c)
        c.set_forcing(fq)
        if g is not None:
            c.set_dirichlet(g)
        c.init()
        rp, ci = c.pattern_get()
        dt, _, nd = sg.dofs(cells, len(nodes), bnd, order)
        ref = sg.values_in_pattern(sg.assemble(nodes, cells, dt, nd, order, op_o), rp, ci)
        e = np.abs(c.matrix_values(capi.MAT_STIFF) - ref).max() / max(1.0, np.abs(ref).max())
        info = c.solve(rtol=1e-12, maxit=100000)
        u = c.solution()
        uref = _ref_solution(nodes, cells, bnd, order, op_o, fq, g)
        se = np.linalg.norm(u - uref) / np.linalg.norm(uref)
        worst_e, worst_s = max(worst_e, e), max(worst_s, se)
        assert e <= ETOL and info.converged == 1 and se <= STOL, (case, order, name, e, se)
        c.close()
    print(f"network fuzz: 40 cases, worst entry error {worst_e:.2e}, worst solution error {worst_s:.2e}")
