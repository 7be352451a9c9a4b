"""Surface meshes (Triangulation<2,3>) on the device: fdapde_mesh_upload(ctx, 2, 3, ...) and everything downstream of it, against the float64
surface assembler of tests/surface_ref.py (pinned to the CPU oracle by tests/test_surface_cpu.py) and scipy's sparse LU.

Fixtures: the reference's 2.5-D mesh test/data/mesh/surface (340 nodes, 616 triangles, open, 64 boundary nodes), icosahedral spheres
(meshgen.unit_sphere_surface) and seeded height fields z = h(x, y) (meshgen.height_field_surface).
Bars: entries <= 1e-13 max(1, |.|max); solutions <= 1e-8 relative to spsolve; symmetric operators bitwise symmetric; runs bitwise reproducible."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import surface_ref as sr

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
def fixture_mesh():
    from oracle import oracle as o

    o.build()
    return sr.load_surface_fixture(ROOT)


def _ctx(capi, nodes, cells, bnd, order):
    c = capi.Context(device=0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(order)
    return c


def _ops3(capi_or_oracle, rng=None, rows=None):
    """the operator expressions of tests/test_gpu_parity.py with 3-D coefficients (+ space-varying ones when rows is given)"""
    m = capi_or_oracle
    K = np.array([[2.0, 0.3, 0.1], [0.3, 1.0, 0.2], [0.1, 0.2, 1.5]])
    b = np.array([0.7, -0.2, 0.4])
    Kn = K + np.array([[0.0, 0.4, 0.0], [-0.2, 0.0, 0.3], [0.1, -0.3, 0.0]])
    ops = {"neg_laplacian": -m.laplacian(), "mass": m.reaction(1.0), "adr": -m.laplacian() + m.advection(b) + m.reaction(1.5),
           "diffusion": m.diffusion(K) + 0.5 * m.reaction(2.0), "laplacian_minus_dt": m.laplacian() - m.dt(),
           "diffusion_nonsym": m.diffusion(Kn) + m.advection(b) + m.reaction(0.5), "diffusion_nonsym_mirrored": m.diffusion(Kn) + m.reaction(0.5)}
    if rows is not None:
        A = rng.standard_normal((rows, 3, 3)) * 0.3
        Kq = np.einsum("rij,rkj->rik", A, A) + np.eye(3)[None]
        bq = rng.standard_normal((rows, 3))
        cq = rng.uniform(0.5, 2.0, rows)
        ops["var_k"] = -m.laplacian() + m.diffusion_field(Kq.reshape(rows, 9))
        ops["var_kbc"] = m.diffusion_field(Kq.reshape(rows, 9)) + m.advection_field(bq) + m.reaction_field(cq)
        ops["var_c"] = -m.laplacian() + m.reaction_field(cq)          # (the split form: constant diffusion, varying reaction)
        ops["var_b_const_k"] = m.diffusion(K) + m.advection_field(bq)
        # a NON-symmetric K field: alone, the reference integrates the pairs dof_i >= dof_j and mirrors them (DevOp::mirror via field_nonsym);
        # next to advection, every pair
        S = rng.uniform(-0.4, 0.4, (rows, 3, 3))
        Kqn = (Kq + (S - np.transpose(S, (0, 2, 1)))).reshape(rows, 9)
        ops["var_k_nonsym_mirrored"] = m.diffusion_field(Kqn) + m.reaction_field(cq)
        ops["var_k_nonsym_adv"] = m.diffusion_field(Kqn) + m.advection(b) + m.reaction(1.0)
    return ops


def _entry_ok(got, ref):
    return np.abs(got - ref).max() <= ETOL * max(1.0, np.abs(ref).max())


def _dev_csr(c, which):
    rp, ci = c.pattern_get()
    v = c.matrix_values(which)
    n = rp.size - 1
    return sp.csr_matrix((v, ci, rp), shape=(n, n))


def _meshes(meshgen, fixture_mesh):
    sph = meshgen.unit_sphere_surface(4)
    hf = meshgen.height_field_surface(16, seed=7, reorient=True)
    return {"fixture": (fixture_mesh.nodes, fixture_mesh.cells, fixture_mesh.boundary), "sphere4": sph, "height16": hf}


# ---- 1. topology of the fixture ---------------------------------------------------------------------------------------------
def test_topology_of_the_surface_fixture(env, fixture_mesh):
    from oracle import oracle as o

    capi, _ = env
    m = fixture_mesh
    c = capi.Context(0)
    c.mesh_upload(m.nodes, m.cells, m.boundary)
    t = c.topology()
    ref = o.topology(m)
    for k in ["neighbors", "cell_facets", "facet_nodes", "facet_cells", "facet_boundary"]:
        assert np.array_equal(t[k], ref[k]), k
    d = os.path.join(ROOT, "tests", "golden", "mesh", "surface")
    neigh = o.read_csv(os.path.join(d, "neigh.csv")).astype(np.int64)
    assert np.array_equal(np.where(neigh > 0, neigh - 1, -1), t["neighbors"])
    edges = np.sort(o.read_csv(os.path.join(d, "edges.csv")).astype(np.int64) - 1, axis=1)
    assert set(map(tuple, edges)) == set(map(tuple, np.sort(t["facet_nodes"], axis=1))) and len(edges) == len(t["facet_nodes"])
    c.close()


# ---- 2. DOF table, boundary DOFs, coordinates, quadrature nodes ---------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_dof_table_and_coordinates(env, fixture_mesh, order):
    from oracle import oracle as o

    capi, _ = env
    m = fixture_mesh
    c = _ctx(capi, m.nodes, m.cells, m.boundary, order)
    dofs, bnd, coords = c.dofs_get()
    odofs, obnd, ond, _ = o.enumerate_dofs(m, order)
    assert c.sizes()["n_dofs"] == ond == (340 if order == 1 else 1296)
    assert np.array_equal(dofs, odofs) and np.array_equal(bnd, obnd) and int(bnd.sum()) == (64 if order == 1 else 128)
    assert coords.shape == (ond, 3)
    assert np.abs(coords - sr.dof_coords(m.nodes, m.cells, odofs, ond, order)).max() <= 1e-15
    qn = c.quadrature_nodes()
    assert qn.shape == (m.n_cells * sr.tables(order)[0].shape[0], 3)
    assert np.abs(qn - sr.quadrature_nodes(m.nodes, m.cells, order)).max() <= 1e-15
    c.close()


# ---- 3. device set-up = host set-up -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("which", ["fixture", "sphere5", "height200k"])
def test_device_setup_equals_host_setup(env, fixture_mesh, order, which, monkeypatch):
    capi, meshgen = env
    if which == "fixture":
        mesh = (fixture_mesh.nodes, fixture_mesh.cells, fixture_mesh.boundary)
    elif which == "sphere5":
        mesh = meshgen.unit_sphere_surface(5, permute=True)
    else:
        mesh = meshgen.height_field_surface(317, seed=3, reorient=True)   # 200 978 triangles
    monkeypatch.setenv("FDAPDE_SETUP_CHECK", "1")
    c = _ctx(capi, *mesh, order)   # (a mismatch fails fdapde_dofs_build)
    c.close()


# ---- 4. entry parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("which", ["fixture", "sphere4", "height16"])
def test_entry_parity(env, fixture_mesh, order, which):
    from oracle import oracle as o

    capi, meshgen = env
    nodes, cells, bnd = _meshes(meshgen, fixture_mesh)[which]
    m = sr.mesh_of(nodes, cells, bnd)
    dofs, _, nd, _ = o.enumerate_dofs(m, order)
    nq = sr.tables(order)[0].shape[0]
    rows = nq * m.n_cells
    rng = np.random.default_rng(11)
    c = _ctx(capi, nodes, cells, bnd, order)
    rp, ci = c.pattern_get()
    ops_c = _ops3(capi, np.random.default_rng(5), rows)
    ops_o = _ops3(o, np.random.default_rng(5), rows)
    fq = rng.standard_normal(rows)
    Mref = sr.assemble(nodes, cells, dofs, nd, order, o.reaction(1.0))
    assert np.array_equal(Mref.indptr, rp) and np.array_equal(Mref.indices, ci)
    fref = sr.forcing(nodes, cells, dofs, nd, order, fq)
    for name in ops_c:
        c.set_operator(ops_c[name])
        c.set_forcing(fq)
        c.init()
        A = sr.assemble(nodes, cells, dofs, nd, order, ops_o[name])
        got = c.matrix_values(capi.MAT_STIFF)
        assert _entry_ok(got, sr.values_in_pattern(A, rp, ci)), (which, order, name)
        assert _entry_ok(c.matrix_values(capi.MAT_MASS), sr.values_in_pattern(Mref, rp, ci)), (which, order, name)
        assert _entry_ok(c.force(), fref), (which, order, name)
        if not any(t[0] == capi.ADVECTION for t in ops_c[name].terms):   # symmetric operators: bitwise A_ij == A_ji
            S = _dev_csr(c, capi.MAT_STIFF)
            assert (S != S.T).nnz == 0, (which, order, name)
        # fdapde_assemble_operator: the same sweep without forcing
        c.assemble_operator(capi.MAT_STIFF, ops_c[name])
        assert np.array_equal(c.matrix_values(capi.MAT_STIFF), got)
    c.close()


# ---- 5. rigid-motion invariance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_rigid_motion_invariance(env, order):
    """unit_square(64) against its embedding: stiffness, mass and force at both orders; the solutions through the dense direct solver (n <= 8192:
    unit_square(64) at P1, 4 225 DOFs; unit_square(44) at P2, 7 921 DOFs -- at 64 the P2 space has 16 641), so that what is compared is the
    assembled systems, not two Krylov iterations stopped at a tolerance"""
    capi, meshgen = env
    R = meshgen.rotation(4)
    Q, t = R[:, :2], np.array([0.3, -1.2, 2.0])
    K2 = np.array([[1.5, 0.2], [0.2, 0.8]])
    for nx, with_solution in ((64, order == 1),) + (((44, True),) if order == 2 else ()):
        p, cells, bnd = meshgen.unit_square(nx, seed=9)
        p3 = meshgen.embed_planar(p, Q, t)
        out = []
        for nodes, K in ((p, K2), (p3, Q @ K2 @ Q.T)):
            c = _ctx(capi, nodes, cells, bnd, order)
            _, _, coords = c.dofs_get()
            xy = (coords - t) @ Q if nodes.shape[1] == 3 else coords   # (planar coordinates of every DOF)
            qn = c.quadrature_nodes()
            qxy = (qn - t) @ Q if nodes.shape[1] == 3 else qn
            c.set_operator(capi.diffusion(K) + capi.reaction(1.0))
            c.set_forcing(np.sin(3 * qxy[:, 0]) * np.cos(2 * qxy[:, 1]))
            c.set_dirichlet(xy[:, 0] ** 2 - xy[:, 1])
            c.init()
            A, Mm, f = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS), c.force()
            u = None
            if with_solution:
                info = c.solve(method=capi.SOLVER_DENSE)
                assert info.converged == 1 and info.method_used == capi.SOLVER_DENSE
                u = c.solution()
            out.append((A, Mm, f, u))
            c.close()
        for k in range(3):
            assert np.abs(out[0][k] - out[1][k]).max() <= 1e-13 * np.abs(out[0][k]).max(), (nx, k)
        if with_solution:
            u0, u1 = out[0][3], out[1][3]
            assert np.linalg.norm(u0 - u1) / np.linalg.norm(u0) <= 1e-11, (nx, np.linalg.norm(u0 - u1) / np.linalg.norm(u0))


# ---- 6. orientation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_orientation_does_not_matter(env, order):
    capi, meshgen = env
    nodes, cells, bnd = meshgen.height_field_surface(24, seed=2)
    flip = np.random.default_rng(3).random(cells.shape[0]) < 0.5
    cells2 = cells.copy()
    cells2[flip] = cells2[flip][:, ::-1]
    op = -capi.laplacian() + capi.advection(np.array([0.3, -0.1, 0.2])) + capi.reaction(1.0)
    mats = []
    for cl in (cells, cells2):
        c = _ctx(capi, nodes, cl, bnd, order)
        c.set_operator(op)
        c.init()
        _, _, coords = c.dofs_get()
        S, Mm = _dev_csr(c, capi.MAT_STIFF), _dev_csr(c, capi.MAT_MASS)
        mats.append((S, Mm, coords))
        c.close()
    # P2: the edge DOFs are numbered in the cells' vertex order -- match them by their coordinates
    (S0, M0, X0), (S1, M1, X1) = mats
    key = lambda X: np.lexsort(np.round(X, 10).T[::-1])   # (an edge midpoint computed from the other end may differ in its last bit)
    k0 = key(X0), key(X1)
    assert np.abs(X0[k0[0]] - X1[k0[1]]).max() <= 1e-15
    P = sp.csr_matrix((np.ones(X0.shape[0]), (k0[0], k0[1])), shape=(X0.shape[0],) * 2)   # dof of run 1 -> dof of run 0
    for A0, A1 in ((S0, S1), (M0, M1)):
        B = (P @ A1 @ P.T).toarray()
        assert np.abs(B - A0.toarray()).max() <= 1e-14 * np.abs(A0).max()


# ---- 7. convergence on the sphere ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_elliptic_convergence_on_the_sphere(env, order):
    capi, meshgen = env
    errs = []
    for L in (3, 4, 5, 6):
        nodes, cells, bnd = meshgen.unit_sphere_surface(L)
        c = _ctx(capi, nodes, cells, bnd, order)
        qn = c.quadrature_nodes()
        c.set_operator(-capi.laplacian() + capi.reaction(1.0))
        c.set_forcing(3.0 * qn[:, 0])
        c.init()
        info = c.solve(rtol=1e-12)
        assert info.converged == 1
        u = c.solution()[: nodes.shape[0]]   # vertex DOFs
        errs.append(np.abs(u - nodes[:, 0]).max())
        c.close()
    rates = np.log2(np.array(errs[:-1]) / np.array(errs[1:]))
    print(f"P{order} sphere max errors {errs}, observed orders {rates}")
    assert rates[-1] >= 1.8 and errs[-1] < 1e-3


def test_parabolic_on_the_sphere(env):
    from oracle import oracle as o

    capi, meshgen = env
    nodes, cells, bnd = meshgen.unit_sphere_surface(4)
    order = 1
    c = _ctx(capi, nodes, cells, bnd, order)
    times = np.linspace(0.0, 0.2, 41)
    nq = sr.tables(order)[0].shape[0]
    c.set_operator(capi.dt() - capi.laplacian())
    c.set_forcing(np.zeros((nq * cells.shape[0], times.size)))
    c.init()
    u0 = nodes[:, 0].copy()
    sol, info = c.solve_parabolic(times, u0, rtol=1e-12)
    m = sr.mesh_of(nodes, cells, bnd)
    dofs, _, nd, _ = o.enumerate_dofs(m, order)
    A = sr.assemble(nodes, cells, dofs, nd, order, o.dt() - o.laplacian())
    Mm = sr.assemble(nodes, cells, dofs, nd, order, o.reaction(1.0))
    dt = times[1] - times[0]
    lu = spla.splu((Mm / dt + A).tocsc())
    ref = np.zeros_like(sol)
    ref[:, 0] = u0
    for i in range(times.size - 1):
        ref[:, i + 1] = lu.solve(Mm @ ref[:, i] / dt)
    assert np.linalg.norm(sol - ref) / np.linalg.norm(ref) <= STOL
    exact = np.exp(-2.0 * times[-1]) * u0
    assert np.linalg.norm(sol[:, -1] - exact) / np.linalg.norm(exact) < 0.02   # implicit Euler, dt = 5e-3
    c.close()


# ---- 8. open surface with Dirichlet data: every method ----------------------------------------------------------------------
def _ref_solution(nodes, cells, bnd, order, op_o, fq, g):
    from oracle import oracle as o

    m = sr.mesh_of(nodes, cells, bnd)
    dofs, dbnd, nd, _ = o.enumerate_dofs(m, order)
    A = sr.assemble(nodes, cells, dofs, nd, order, op_o)
    b = sr.forcing(nodes, cells, dofs, nd, order, fq)
    if g is not None:
        A, b = sr.set_dirichlet(A, b, dbnd, g)
    return spla.spsolve(A.tocsc(), b)


@pytest.mark.parametrize("order", [1, 2])
def test_open_surface_every_method(env, fixture_mesh, order):
    from oracle import oracle as o

    capi, _ = env
    m = fixture_mesh
    c = _ctx(capi, m.nodes, m.cells, m.boundary, order)
    _, _, coords = c.dofs_get()
    qn = c.quadrature_nodes()
    g = coords[:, 0] * coords[:, 1] + coords[:, 2]
    fq = np.cos(qn[:, 0]) + qn[:, 2]
    for label, op_c, op_o in (("lap", -capi.laplacian(), -o.laplacian()),
                              ("adr", -capi.laplacian() + capi.advection(np.array([0.5, -0.3, 0.2])) + capi.reaction(1.0),
                               -o.laplacian() + o.advection(np.array([0.5, -0.3, 0.2])) + o.reaction(1.0))):
        ref = _ref_solution(m.nodes, m.cells, m.boundary, order, op_o, fq, g)
        sym = label == "lap"
        methods = [capi.SOLVER_AUTO, capi.SOLVER_BICGSTAB, capi.SOLVER_GMRES, capi.SOLVER_DENSE] + ([capi.SOLVER_CG] if sym else [])
        for meth in methods:
            c.set_operator(op_c)
            c.set_forcing(fq)
            c.set_dirichlet(g)
            c.init()
            info = c.solve(method=meth, rtol=1e-12)
            assert info.converged == 1, (label, meth)
            u = c.solution()
            assert np.linalg.norm(u - ref) / np.linalg.norm(ref) <= STOL, (label, meth, np.linalg.norm(u - ref) / np.linalg.norm(ref))
    c.close()


@pytest.mark.parametrize("method", ["PMG", "AMG"])
def test_multilevel_solvers_on_a_sphere(env, method):
    from oracle import oracle as o

    capi, meshgen = env
    nodes, cells, bnd = meshgen.unit_sphere_surface(5)
    order = 2 if method == "PMG" else 1
    c = _ctx(capi, nodes, cells, bnd, order)
    qn = c.quadrature_nodes()
    fq = 3.0 * qn[:, 0] + qn[:, 1] * qn[:, 2]
    c.set_operator(-capi.laplacian() + capi.reaction(2.0))
    c.set_forcing(fq)
    c.init()
    info = c.solve(method=getattr(capi, "SOLVER_" + method), rtol=1e-12)
    assert info.converged == 1 and info.method_used == getattr(capi, "SOLVER_" + method)
    ref = _ref_solution(nodes, cells, bnd, order, -o.laplacian() + o.reaction(2.0), fq, None)
    assert np.linalg.norm(c.solution() - ref) / np.linalg.norm(ref) <= STOL
    if method == "AMG":   # ... and AMG on the P2 space of a smaller sphere
        c.close()
        nodes, cells, bnd = meshgen.unit_sphere_surface(4)
        c = _ctx(capi, nodes, cells, bnd, 2)
        qn = c.quadrature_nodes()
        fq = 3.0 * qn[:, 0]
        c.set_operator(-capi.laplacian() + capi.reaction(2.0))
        c.set_forcing(fq)
        c.init()
        assert c.solve(method=capi.SOLVER_AMG, rtol=1e-12).converged == 1
        ref = _ref_solution(nodes, cells, bnd, 2, -o.laplacian() + o.reaction(2.0), fq, None)
        assert np.linalg.norm(c.solution() - ref) / np.linalg.norm(ref) <= STOL
    c.close()


@pytest.mark.parametrize("order", [1, 2])
def test_factor_once_handle_and_lumping(env, fixture_mesh, order):
    from oracle import oracle as o

    capi, _ = env
    m = fixture_mesh
    c = _ctx(capi, m.nodes, m.cells, m.boundary, order)
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.init()
    dofs, _, nd, _ = o.enumerate_dofs(m, order)
    A = sr.assemble(m.nodes, m.cells, dofs, nd, order, -o.laplacian() + o.reaction(1.0))
    Mm = sr.assemble(m.nodes, m.cells, dofs, nd, order, o.reaction(1.0))
    rng = np.random.default_rng(4)
    for which, R in ((capi.MAT_STIFF, A), (capi.MAT_MASS, Mm)):
        c.lin_compute(which, symmetric=True)
        for ncol in (1, 8):
            B = rng.standard_normal((nd, ncol)) if ncol > 1 else rng.standard_normal(nd)
            X, info = c.lin_solve(B, rtol=1e-12)
            ref = spla.spsolve(R.tocsc(), B)
            assert np.linalg.norm(X - ref) / np.linalg.norm(ref) <= STOL, (which, ncol)
    assert np.abs(c.lump(capi.MAT_MASS) - np.asarray(Mm.sum(axis=1)).ravel()).max() <= ETOL * np.abs(Mm).max()
    c.close()


# ---- 9. cell integrals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_cell_integrals(env, fixture_mesh, order):
    capi, meshgen = env
    nodes, cells, bnd = meshgen.unit_sphere_surface(6)
    c = _ctx(capi, nodes, cells, bnd, order)
    psi, D = c.eval_areal(np.ones((1, cells.shape[0]), dtype=int))
    assert abs(D[0] - 4 * np.pi) < 2e-3
    c.close()
    m = fixture_mesh
    c = _ctx(capi, m.nodes, m.cells, m.boundary, order)
    meas = np.zeros(m.n_cells)
    pint = np.zeros((m.n_cells, c.sizes()["n_basis"]))
    import ctypes as C

    c._check(c.lib.fdapde_cell_integrals(c._ctx, meas.ctypes.data_as(C.POINTER(C.c_double)), pint.ctypes.data_as(C.POINTER(C.c_double))))
    _, _, rmeas = sr.geometry(m.nodes, m.cells)
    _, qw, tpsi, _ = sr.tables(order)
    assert np.abs(meas - rmeas).max() <= 1e-15
    assert np.abs(pint - rmeas[:, None] * (tpsi @ qw)[None, :]).max() <= 1e-14
    c.close()


# ---- 10. determinism and clone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_determinism_and_clone(env, order):
    capi, meshgen = env
    nodes, cells, bnd = meshgen.height_field_surface(40, seed=5, reorient=True)
    runs = []
    for _ in range(2):
        c = _ctx(capi, nodes, cells, bnd, order)
        _, _, coords = c.dofs_get()
        qn = c.quadrature_nodes()
        c.set_operator(capi.diffusion(np.diag([1.0, 2.0, 0.5])) + capi.reaction(1.0))
        c.set_forcing(np.sin(qn[:, 0] + qn[:, 2]))
        c.set_dirichlet(coords[:, 2])
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


# ---- 11. refusals --------------------------------------------------------------------------------------------------------------------
def _status(fn):
    from fdapde_core_amd import capi

    with pytest.raises(capi.FdapdeError) as e:
        fn()
    return e.value.status, str(e.value)


def test_refusals(env, fixture_mesh):
    capi, meshgen = env
    m = fixture_mesh
    c = _ctx(capi, m.nodes, m.cells, m.boundary, 1)
    st, msg = _status(lambda: c.eval_pointwise(m.nodes[:3]))
    assert st == capi.EUNSUPPORTED and "surface" in msg
    c.set_operator(-capi.laplacian())
    for v in (capi.ASSEMBLY_ATOMIC, capi.ASSEMBLY_COLOURED, capi.ASSEMBLY_PARTITIONED, capi.ASSEMBLY_WAVE):
        st, msg = _status(lambda: c.init(assembly=v))
        assert st == capi.EUNSUPPORTED and "row-owner" in msg, v
        st, msg = _status(lambda: c.assemble_operator(capi.MAT_STIFF, -capi.laplacian(), assembly=v))
        assert st == capi.EUNSUPPORTED, v
    c.init()   # (the row-owner sweep still works after the refusals)
    st, msg = _status(lambda: c.partition_build(2))
    assert st == capi.EUNSUPPORTED and "surface" in msg
    c.close()
    g = capi.Context(devices=[0, 0])
    st, msg = _status(lambda: g.mesh_upload(m.nodes, m.cells, m.boundary))
    assert st == capi.EUNSUPPORTED and "surface" in msg
    g.close()
    h = capi.Context(0)
    for nodes, cells in ((m.nodes[:, :1], m.cells), (m.nodes[:, :2], np.zeros((2, 4), np.int32)), (m.nodes[:, :2], m.cells[:, :2]),
                         (np.zeros((4, 4)), np.array([[0, 1, 2, 3]], np.int32)), (m.nodes, m.cells[:, :2])):
        st, _ = _status(lambda: h.mesh_upload(nodes, cells, np.zeros(nodes.shape[0], np.uint8)))
        assert st == capi.EUNSUPPORTED, (nodes.shape, cells.shape)
    h.close()


# ---- 12. fuzz ----------------------------------------------------------------------------------------------------------------------
def _fuzz_ops(m, rng, rows):
    """random coercive operators (a positive reaction: solvable on closed surfaces too), constant and space-varying, with the mirrored quirk"""
    K = np.diag(rng.uniform(0.5, 2.0, 3))
    K[0, 1] = K[1, 0] = rng.uniform(-0.2, 0.2)
    b = rng.uniform(-1, 1, 3)
    Kn = K + np.array([[0.0, 0.2, 0.0], [-0.1, 0.0, 0.1], [0.05, -0.1, 0.0]])
    A = rng.standard_normal((rows, 3, 3)) * 0.3
    Kq = (np.einsum("rij,rkj->rik", A, A) + np.eye(3)[None]).reshape(rows, 9)
    bq, cq = rng.standard_normal((rows, 3)), rng.uniform(0.5, 2.0, rows)
    c = float(rng.uniform(0.5, 2.0))
    return {"lap": -m.laplacian() + m.reaction(c), "diff": -m.diffusion(K) + m.reaction(c), "adr": -m.laplacian() + m.advection(b) + m.reaction(c),
            "nonsym_mirrored": -m.diffusion(Kn) + m.reaction(c), "nonsym_adv": -m.diffusion(Kn) + m.advection(b) + m.reaction(c),
            "var_kbc": -m.diffusion_field(Kq) + m.advection_field(bq) + m.reaction_field(cq), "var_c": -m.laplacian() + m.reaction_field(cq)}


def test_fuzz_random_surfaces(env):
    from oracle import oracle as o

    capi, meshgen = env
    rng = np.random.default_rng(2024)
    worst_e = worst_s = 0.0
    for case in range(30):
        kind = rng.integers(3)
        if kind == 0:
            nodes, cells, bnd = meshgen.height_field_surface(int(rng.integers(4, 14)), seed=int(rng.integers(1 << 30)), amplitude=float(rng.uniform(0, 0.6)),
                                                             reorient=bool(rng.integers(2)))
        elif kind == 1:
            p, cells, bnd = meshgen.unit_square(int(rng.integers(4, 14)), seed=int(rng.integers(1 << 30)))
            R = meshgen.rotation(int(rng.integers(1 << 30)))
            nodes = meshgen.embed_planar(p, R[:, :2], rng.uniform(-3, 3, 3))
        else:
            nodes, cells, bnd = meshgen.unit_sphere_surface(int(rng.integers(1, 4)), seed=int(rng.integers(1 << 30)), permute=True)
            nodes = nodes * rng.uniform(0.5, 2.0)
        order = int(rng.integers(1, 3))
        nq = sr.tables(order)[0].shape[0]
        rows = nq * cells.shape[0]
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
        m = sr.mesh_of(nodes, cells, bnd)
        dofs, _, nd, _ = o.enumerate_dofs(m, order)
        A = sr.assemble(nodes, cells, dofs, nd, order, op_o)
        ref = sr.values_in_pattern(A, rp, ci)
        e = np.abs(c.matrix_values(capi.MAT_STIFF) - ref).max() / max(1.0, np.abs(ref).max())
        info = c.solve(rtol=1e-12)
        u = c.solution()
        uref = _ref_solution(nodes, cells, bnd, order, op_o, fq, g)
        se = np.linalg.norm(u - uref) / np.linalg.norm(uref)
        worst_e, worst_s = max(worst_e, e), max(worst_s, se)
        assert e <= ETOL and info.converged == 1 and se <= STOL, (case, kind, order, name, e, se)
        c.close()
    print(f"surface fuzz: 30 cases, worst entry error {worst_e:.2e} (relative to max(1, |A|max)), worst solution error {worst_s:.2e}")
