"""The absorption pass of the multilevel set-ups (csrc/eng_amg.hip: k_amg_absorb, the knob `amg_absorb`) and the query fdapde_amg_hierarchy, on the device:
FDAPDE_SOLVER_AMG through fdapde_solve, fdapde_lin_solve and fdapde_solve_parabolic and FDAPDE_SOLVER_BLOCK_AMG through fdapde_block_solve, against scipy's
SuperLU and against the numpy restatement (tests/amg_absorb_ref.py, which tests/test_amg_absorb_cpu.py holds to HALF of every cap handed over here).  Every small
case switches `amg_setup_check` on: the device-built aggregates, patterns, values and members are compared bit for bit with the host loops."""
import os

import numpy as np
import pytest

import amg_absorb_ref as ab
import block_amg_ref as ar
import block_ref as br

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen, workloads

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, meshgen, workloads


def _mesh(env, mesh):
    _, meshgen, workloads = env
    if isinstance(mesh, str):
        return workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", mesh))
    return getattr(meshgen, mesh[0])(mesh[1])


def _ctx(env, mesh, order, absorb, coarse_rows=ab.COARSE_ROWS, check=1):
    capi = env[0]
    nodes, cells, bnd = _mesh(env, mesh)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(order)
    c.tune("amg_setup_check", check)
    c.tune("amg_coarse_rows", coarse_rows)
    c.tune("amg_absorb", absorb)
    return c, nd, nodes


def _csr(c, capi, nd, which=None):
    import scipy.sparse as sp

    rp, ci = c.pattern_get()
    return sp.csr_matrix((c.matrix_values(capi.MAT_STIFF if which is None else which), ci, rp), shape=(nd, nd))


def _kept(h):
    return ab.kept(h["rows"])


# ---- FDAPDE_SOLVER_AMG with absorption on every level ------------------------------------------------------------------------------------------------
def _lu_problem(env, mesh, order, kind, dirichlet, absorb=1):
    capi = env[0]
    c, nd, nodes = _ctx(env, mesh, order, absorb)
    dim = nodes.shape[1]
    _, bd, coords = c.dofs_get()
    b = [3.0, -1.5] if dim == 2 else [1.0, 0.5, 0.25]
    c.set_operator({"lap": -capi.laplacian(), "reaction": -capi.laplacian() + capi.reaction(2.0),
                    "adr": -capi.laplacian() + capi.advection(b) + capi.reaction(1.0)}[kind])
    qn = c.quadrature_nodes()
    c.set_forcing(1.0 + np.sin(3.0 * qn[:, 0]) * qn[:, 1])
    if dirichlet == "zero":
        c.set_dirichlet(np.zeros(nd))
    elif dirichlet == "data":
        c.set_dirichlet(0.3 * np.cos(2.0 * coords[:, 0]) + coords[:, -1])
    c.init()
    return c, nd, nd - (int(np.count_nonzero(bd)) if dirichlet != "none" else 0)


LU_CASES = [(("unit_cube", 8), 1, "lap", "zero", True), (("unit_cube", 16), 1, "reaction", "data", True), (("unit_square", 32), 1, "lap", "zero", True),
            ("unit_sphere", 1, "reaction", "data", False), ("c_shaped", 2, "reaction", "zero", False), (("unit_square", 48), 1, "adr", "data", False)]


@pytest.mark.parametrize("mesh,order,kind,dirichlet,keep", LU_CASES, ids=[f"{m if isinstance(m, str) else m[0] + str(m[1])}-P{o}-{k}" for m, o, k, _, _ in LU_CASES])
def test_against_lu(env, mesh, order, kind, dirichlet, keep):
    """`amg_absorb` 1, `amg_coarse_rows` 256, the tolerances of tests/test_gpu_amg.py::test_against_lu (rtol 1e-11, at most 60 iterations, 1e-8 of the LU
    solution, a second solve with the same count and bits).  The hierarchy as fdapde_amg_hierarchy reports it: absorbed, several levels, and -- on the
    meshes whose restatement tests/test_amg_absorb_cpu.py checks (keep) -- no level keeps more than 0.35 of the rows above it; the shares are printed for the others."""
    import scipy.sparse.linalg as spl

    capi = env[0]
    c, nd, free = _lu_problem(env, mesh, order, kind, dirichlet)
    info = c.solve(method=capi.SOLVER_AMG, rtol=1e-11)
    assert info.method_used == capi.SOLVER_AMG and info.converged == 1 and info.relres <= 1e-11
    assert info.persistent == 0 and info.iters <= 60, info.iters
    u = c.solution()
    ref = spl.spsolve(_csr(c, capi, nd).tocsc(), c.force())
    h = c.amg_hierarchy(capi.AMG_OF_SOLVE)
    print(f"{mesh} P{order} {kind}: {nd} DOFs, rows {h['rows']}, kept {[round(k, 3) for k in _kept(h)]}, entries {h['nnz']}, set-up {h['setup_ms']:.1f} ms, {info.iters} iterations")
    assert np.linalg.norm(u - ref) <= 1e-8 * np.linalg.norm(ref)
    assert h["absorbed"] == 1 and len(h["rows"]) >= 2 and h["rows"][0] == nd and h["rows"][-1] <= ab.COARSE_ROWS and h["setup_ms"] > 0.0
    assert h["nnz"][0] == c.sizes()["nnz"] and all(z > 0 for z in h["nnz"])
    if keep:   # (level 0's share is taken of its free rows: the Dirichlet rows belong to no aggregate)
        assert max(ab.kept([free] + h["rows"][1:])) <= ab.KEEP, (free, h["rows"])
    again = c.solve(method=capi.SOLVER_AMG, rtol=1e-11)
    assert again.iters == info.iters and np.array_equal(c.solution(), u)
    c.close()


def _ladder(env, ladder):
    """P1 -Lap, zero Dirichlet data, the seeded load of the restatement, rtol 1e-10 -> (iterations, hierarchy) per mesh"""
    capi = env[0]
    out = []
    for mesh in ladder:
        c, nd, _ = _ctx(env, mesh, 1, 1)
        c.set_operator(-capi.laplacian())
        c.set_forcing(ab.ladder_forcing(c.quadrature_nodes().shape[0]))
        c.set_dirichlet(np.zeros(nd))
        c.init()
        info = c.solve(method=capi.SOLVER_AMG, rtol=1e-10)
        assert info.method_used == capi.SOLVER_AMG and info.converged == 1
        out.append((info.iters, c.amg_hierarchy(capi.AMG_OF_SOLVE)))
        c.close()
    return out


@pytest.mark.parametrize("ladder,cap", [(ab.LADDER_3D, ab.CAP_3D), (ab.LADDER_2D, ab.CAP_2D)], ids=["unit_cube", "unit_square"])
def test_ladders_caps_and_kept_rows(env, ladder, cap):
    """unit_cube(8, 16, 32) within 40 and unit_square(32, 64, 128) within 50 iterations (the restatement: 14 / 17 / 18 and 22 / 22 / 23), the largest mesh's
    count <= 1.5 x the smallest's + 2, and every level keeps at most 0.35 of the rows above it.  Level 0 counts its Dirichlet rows, which belong to no
    aggregate: its share is taken of the free rows."""
    runs = _ladder(env, ladder)
    counts = [it for it, _ in runs]
    for mesh, (it, h) in zip(ladder, runs):
        print(f"{mesh[0]}({mesh[1]}): rows {h['rows']}, kept {[round(k, 3) for k in _kept(h)]}, {it} iterations (cap {cap})")
    assert max(counts) <= cap, counts
    assert counts[-1] <= 1.5 * counts[0] + 2, counts
    for mesh, (_, h) in zip(ladder, runs):
        dim = 3 if mesh[0] == "unit_cube" else 2
        rows = [(mesh[1] - 1) ** dim] + h["rows"][1:]   # the free rows of level 0
        assert h["absorbed"] == 1 and len(rows) >= 2 and max(ab.kept(rows)) <= ab.KEEP, (mesh, rows)


def test_handle_with_absorption(env):
    """fdapde_lin_solve: the mass matrix of unit_square(32) P1, three columns against SuperLU; the handle's hierarchy is `which` 1"""
    import scipy.sparse.linalg as spl

    capi = env[0]
    c, nd, _ = _lu_problem(env, ("unit_square", 32), 1, "reaction", "none")
    with pytest.raises(capi.FdapdeError) as e:
        c.amg_hierarchy(capi.AMG_OF_HANDLE)
    assert e.value.status == capi.ENOTINIT
    A = _csr(c, capi, nd, capi.MAT_MASS)
    B = np.random.default_rng(7).standard_normal((nd, 3))
    c.lin_compute(values=A.data, symmetric=True)
    X, info = c.lin_solve(B, method=capi.SOLVER_AMG)
    assert info.method_used == capi.SOLVER_AMG and info.converged == 1
    ref = spl.splu(A.tocsc()).solve(B)
    for j in range(3):
        assert np.linalg.norm(X[:, j] - ref[:, j]) <= 1e-8 * np.linalg.norm(ref[:, j])
    h = c.amg_hierarchy(capi.AMG_OF_HANDLE)
    print(f"handle: rows {h['rows']}, kept {[round(k, 3) for k in _kept(h)]}")
    assert h["absorbed"] == 1 and h["rows"][0] == nd and len(h["rows"]) >= 2 and h["rows"][-1] <= ab.COARSE_ROWS
    with pytest.raises(capi.FdapdeError) as e:   # (fdapde_solve has not built one)
        c.amg_hierarchy(capi.AMG_OF_SOLVE)
    assert e.value.status == capi.ENOTINIT
    c.close()


def test_stepper_with_absorption(env):
    """fdapde_solve_parabolic by name on unit_square(32) P1, 6 steps with Dirichlet data: every column against SuperLU stepping of the same implicit Euler
    system (the stepper's hierarchy belongs to the call: none is live afterwards)"""
    import scipy.sparse.linalg as spl

    capi = env[0]
    c, nd, _ = _ctx(env, ("unit_square", 32), 1, 1)
    _, bd, coords = c.dofs_get()
    c.set_operator(-capi.laplacian() + capi.advection([1.0, 0.5]) + capi.dt())
    times = np.linspace(0.0, 0.3, 6)
    qn = c.quadrature_nodes()
    c.set_forcing(np.stack([np.sin(2.0 * qn[:, 0]) * (1.0 + t) for t in times], axis=1))
    c.init()
    u0 = np.sin(np.pi * coords[:, 0]) * np.sin(np.pi * coords[:, 1])
    g = np.stack([0.1 * t * coords[:, 0] for t in times], axis=1)
    U, info = c.solve_parabolic(times, u0, dirichlet=g, method=capi.SOLVER_AMG, rtol=1e-12)
    assert info.method_used == capi.SOLVER_AMG and info.converged == 1
    dt = times[1] - times[0]
    M = _csr(c, capi, nd, capi.MAT_MASS)
    K = (M / dt + _csr(c, capi, nd, capi.MAT_STIFF)).tolil()
    b_rows = np.flatnonzero(bd)
    for i in b_rows:
        K.rows[i], K.data[i] = [int(i)], [1.0]
    lu = spl.splu(K.tocsc())
    F = c.force(len(times)).reshape(len(times), nd).T
    u = u0.copy()
    for i in range(len(times) - 1):
        rhs = M @ u / dt + F[:, i + 1]
        rhs[b_rows] = g[b_rows, i + 1]
        u = lu.solve(rhs)
        assert np.linalg.norm(U[:, i + 1] - u) <= 1e-8 * np.linalg.norm(u), i
    with pytest.raises(capi.FdapdeError) as e:
        c.amg_hierarchy(capi.AMG_OF_SOLVE)
    assert e.value.status == capi.ENOTINIT
    c.close()


def test_two_fresh_contexts_give_the_same_bits(env):
    capi = env[0]
    out = []
    for _ in range(2):
        c, nd, _ = _lu_problem(env, ("unit_cube", 16), 1, "reaction", "data")
        info = c.solve(method=capi.SOLVER_AMG)
        out.append((info.iters, c.solution(), c.amg_hierarchy(capi.AMG_OF_SOLVE)))
        c.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    assert out[0][2]["rows"] == out[1][2]["rows"] and out[0][2]["nnz"] == out[1][2]["nnz"]


# ---- the default changes nothing for what is solved today ---------------------------------------------------------------------------------------------
def _block_system(env, mesh, lam, absorb, coarse_rows, dense_rows=None):
    """the smoothing system on the device's own P1 matrices -> (context with the handle computed, A, b, n_dofs, blocks, rowptr, colidx)"""
    capi = env[0]
    c, nd, nodes = _ctx(env, mesh, 1, absorb, coarse_rows)
    if dense_rows is not None:
        c.tune("dense_rows", dense_rows)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    rp, ci = c.pattern_get()
    obs = br.observed_nodes(nodes.shape[0])
    blocks = br.smoothing_blocks(rp, ci, c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS), obs, lam, nd)
    c.block_compute(*blocks, symmetric=True)
    return c, br.bmat(rp, ci, blocks, nd), br.smoothing_rhs(obs, lam, nd), nd, blocks, rp, ci


def test_the_default_keeps_todays_scalar_hierarchy_and_bits(env):
    """unit_cube(16): `amg_absorb` 2 against 0 -- array_equal solutions, the same levels, absorbed == 0; and it differs from 1 (the knob reaches the set-up).
    The knob is switched on ONE context too: the live hierarchy is dropped and built again."""
    capi = env[0]
    got = {}
    for absorb in (0, 2, 1):
        c, nd, _ = _lu_problem(env, ("unit_cube", 16), 1, "reaction", "data", absorb)
        info = c.solve(method=capi.SOLVER_AMG)
        got[absorb] = (info.iters, c.solution(), c.amg_hierarchy(capi.AMG_OF_SOLVE))
        if absorb == 1:
            c.tune("amg_absorb", 2)
            with pytest.raises(capi.FdapdeError):
                c.amg_hierarchy(capi.AMG_OF_SOLVE)
            info = c.solve(method=capi.SOLVER_AMG)
            assert info.iters == got[2][0] and np.array_equal(c.solution(), got[2][1]) and c.amg_hierarchy(capi.AMG_OF_SOLVE)["absorbed"] == 0
        c.close()
    print({k: (v[0], v[2]["rows"]) for k, v in got.items()})
    assert got[2][0] == got[0][0] and np.array_equal(got[2][1], got[0][1])
    assert got[2][2]["absorbed"] == 0 == got[0][2]["absorbed"] and got[2][2]["rows"] == got[0][2]["rows"] and got[2][2]["nnz"] == got[0][2]["nnz"]
    assert got[1][2]["absorbed"] == 1 and got[1][2]["rows"] != got[0][2]["rows"]


def test_the_default_keeps_todays_block_hierarchy_and_bits(env):
    """the block system on unit_square(32), lambda 1e-4, `amg_coarse_rows` 256: x under `amg_absorb` 2 is array_equal to x under 0, absorbed == 0"""
    capi = env[0]
    got = {}
    for absorb in (0, 2):
        c, A, b, nd, *_ = _block_system(env, ("unit_square", 32), 1e-4, absorb, ar.COARSE_ROWS)
        with pytest.raises(capi.FdapdeError) as e:
            c.amg_hierarchy(capi.AMG_OF_BLOCK)
        assert e.value.status == capi.ENOTINIT
        x, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ar.RTOL, maxit=ar.BUDGET_P1)
        assert info.converged == 1
        got[absorb] = (info.iters, x, c.amg_hierarchy(capi.AMG_OF_BLOCK))
        c.close()
    print({k: (v[0], v[2]["rows"]) for k, v in got.items()})
    assert got[2][0] == got[0][0] and np.array_equal(got[2][1], got[0][1])
    assert got[2][2]["absorbed"] == 0 == got[0][2]["absorbed"] and got[2][2]["rows"] == got[0][2]["rows"] and got[2][2]["rows"][0] == 2 * 33 * 33


# ---- the smallest refusal ---------------------------------------------------------------------------------------------------------------------------------
def test_the_smallest_refusal_is_solved_by_the_default(env):
    """The block system on unit_cube(16), lambda 1e-4, `amg_coarse_rows` 32, `dense_rows` 48.  `amg_absorb` 0: FDAPDE_EUNSUPPORTED, coarsening stalls above
    48 rows (the restatement, in the caller's numbering, at 2 n_l = 86).  The default: converges within BUDGET_P1 (the restatement: 21), against LU by the rule
    of test_gpu_block_amg._against_lu, reports absorbed == 1 and a last level of at most 32 rows, and its x is array_equal to the one under `amg_absorb` 1."""
    import scipy.sparse.linalg as spl

    capi = env[0]
    mesh, _, lam, _ = ab.BLOCK_CASE
    c, A, b, nd, blocks, rp, ci = _block_system(env, mesh, lam, 0, ab.BLOCK_COARSE_ROWS, ab.BLOCK_DENSE_ROWS)
    with pytest.raises(capi.FdapdeError) as e:
        c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ar.RTOL, maxit=ab.CAP_BLOCK)
    assert e.value.status == capi.EUNSUPPORTED and "stalled" in str(e.value)
    assert str(e.value) == (f"[status {capi.EUNSUPPORTED}] FDAPDE_SOLVER_BLOCK_AMG: coarsening stalled above the dense limit (a level kept more than 0.8 of its rows): "
                            "the strength block has too few strong couplings for pairwise aggregation")
    c.close()
    x_lu = spl.splu(A.tocsc()).solve(b)
    x_ref, it_ref, ok_ref, rows_ref = ab.block_solve(rp, ci, blocks, nd, b, True, ab.BLOCK_COARSE_ROWS, ab.BLOCK_DENSE_ROWS)
    assert ok_ref
    e_ref = np.linalg.norm(x_ref - x_lu) / np.linalg.norm(x_lu)
    got = {}
    for absorb in (2, 1):
        c, *_ = _block_system(env, mesh, lam, absorb, ab.BLOCK_COARSE_ROWS, ab.BLOCK_DENSE_ROWS)
        x, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ar.RTOL, maxit=ab.CAP_BLOCK, raise_on_noconv=False)
        h = c.amg_hierarchy(capi.AMG_OF_BLOCK)
        err, res = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu), np.linalg.norm(b - A @ x) / np.linalg.norm(b)
        print(f"amg_absorb {absorb}: rows {h['rows']}, kept {[round(k, 3) for k in _kept(h)]}, iterations {info.iters} (restatement {it_ref}, rows {rows_ref}, "
              f"cap {ab.CAP_BLOCK}), relres {info.relres:.2e}, recomputed {res:.2e}, error against LU {err:.2e} (restatement {e_ref:.2e}), set-up {h['setup_ms']:.1f} ms")
        assert info.converged == 1 and info.method_used == capi.SOLVER_BLOCK_AMG and info.iters <= ab.CAP_BLOCK
        assert info.relres <= ar.RTOL and res <= 10 * ar.RTOL and err <= 10 * e_ref
        assert h["absorbed"] == 1 and h["rows"][0] == 2 * nd and h["rows"][-1] <= ab.BLOCK_COARSE_ROWS and max(_kept(h)) <= ab.KEEP
        got[absorb] = (info.iters, x, h)
        c.close()
    assert got[2][0] == got[1][0] and np.array_equal(got[2][1], got[1][1]) and got[2][2]["rows"] == got[1][2]["rows"]


# ---- full size: the documented device refusal ---------------------------------------------------------------------------------------------------------
def test_c3_is_solved_by_the_default(env):
    """unit_cube(119), P1 -Lap, Dirichlet, the manufactured solution of tests/test_gpu_fullsize.py (the scalar stall limit is a constant: no smaller shape is
    refused; `amg_setup_check` off).  `amg_absorb` 0: FDAPDE_EUNSUPPORTED.  The default: true relres <= 1e-10 within 38 iterations (the restatement: 19), the
    error bound test_fullsize_properties uses for C3, at least 5 levels, absorbed, a last level of at most 1 024 rows.  Then, on the same context, the
    smoothing system (lambda 1e-4, observations at half of the nodes) through FDAPDE_SOLVER_BLOCK_AMG within the solver's default maxit, its residual
    recomputed with scipy from matrix_values (-Lap's stiffness matrix is bitwise symmetric -- test_fullsize_properties -- so the (1,2) block is the (2,1)
    block); no count is claimed for it: printed."""
    import scipy.sparse as sp

    capi, meshgen, _ = env
    nodes, cells, bnd = meshgen.unit_cube(119)
    h_mesh = 1.0 / 119
    u_exact, f = meshgen.manufactured(3)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    _, bdofs, coords = c.dofs_get()
    qn = c.quadrature_nodes()
    c.set_operator(-capi.laplacian())
    c.set_forcing(f(qn))
    c.init()
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)   # (before the Dirichlet rows are zeroed)
    c.set_dirichlet(np.zeros(nd))
    c.init()
    c.tune("amg_absorb", 0)
    with pytest.raises(capi.FdapdeError) as e:
        c.solve(method=capi.SOLVER_AMG, rtol=1e-10)
    assert e.value.status == capi.EUNSUPPORTED and "stalled" in str(e.value)
    assert str(e.value) == (f"[status {capi.EUNSUPPORTED}] FDAPDE_SOLVER_AMG: coarsening stalled above the dense limit (a level kept more than 0.8 of its rows): "
                            "the matrix has too few strong couplings for pairwise aggregation")
    c.tune("amg_absorb", 2)
    info = c.solve(method=capi.SOLVER_AMG, rtol=1e-10, maxit=38, raise_on_noconv=False)
    h = c.amg_hierarchy(capi.AMG_OF_SOLVE)
    print(f"C3: rows {h['rows']}, entries {h['nnz']}, operator complexity {sum(h['nnz']) / h['nnz'][0]:.3f}, set-up {h['setup_ms']:.1f} ms (the discarded build included), "
          f"solve {info.t_solve_ms:.1f} ms, {info.iters} iterations, relres {info.relres:.2e}")
    assert info.method_used == capi.SOLVER_AMG and info.converged == 1 and info.relres <= 1e-10 and info.iters <= 38
    u = c.solution()
    assert np.abs(u - u_exact(coords)).max() < 6.0 * h_mesh * h_mesh * np.pi**2
    assert np.all(u[bdofs.astype(bool)] == 0.0)
    assert len(h["rows"]) >= 5 and h["absorbed"] == 1 and h["rows"][0] == nd and h["rows"][-1] <= 1024
    # the smoothing system on the same context
    lam = 1e-4
    rp, ci = c.pattern_get()
    obs = br.observed_nodes(nodes.shape[0])
    rows = np.repeat(np.arange(nd), np.diff(rp))
    diag = np.flatnonzero(rows == ci)
    a11 = np.zeros(len(ci))
    a11[diag[obs]] = -1.0
    c.block_compute(a11, lam * r1, lam * r1, lam * r0, symmetric=True)
    b = br.smoothing_rhs(obs, lam, nd)
    x, binfo = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ar.RTOL, raise_on_noconv=False)
    hb = c.amg_hierarchy(capi.AMG_OF_BLOCK)
    R1, R0 = sp.csr_matrix((r1, ci, rp), shape=(nd, nd)), sp.csr_matrix((r0, ci, rp), shape=(nd, nd))
    ind = np.zeros(nd)
    ind[obs] = 1.0
    res = np.concatenate([b[:nd] - (-ind * x[:nd] + lam * (R1 @ x[nd:])), b[nd:] - lam * (R1 @ x[:nd] + R0 @ x[nd:])])
    rel = np.linalg.norm(res) / np.linalg.norm(b)
    print(f"C3 smoothing system: rows {hb['rows']}, absorbed {hb['absorbed']}, set-up {hb['setup_ms']:.1f} ms, solve {binfo.t_solve_ms:.1f} ms, {binfo.iters} iterations, "
          f"relres {binfo.relres:.2e}, recomputed {rel:.2e}")
    assert binfo.converged == 1 and binfo.method_used == capi.SOLVER_BLOCK_AMG and binfo.iters <= 200
    assert rel <= 10 * ar.RTOL
    c.close()
