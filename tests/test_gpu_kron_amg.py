"""FDAPDE_SOLVER_KRON_AMG (csrc/eng_kron_amg.hip, kernels_kron.h k_kamg_*): the multilevel preconditioner of the Kronecker-sum handle against SuperLU on
the explicit matrix, the numpy restatement of tests/kron_amg_ref.py (tests/test_kron_amg_cpu.py holds it under half of every budget handed over here), and
the 2 x 2 block handle's FDAPDE_SOLVER_BLOCK_AMG as a yardstick.  Every context runs under amg_coarse_rows = 256, so that 289-DOF systems get several levels."""
import os

import numpy as np
import pytest

import block_ref as br
import kron_amg_ref as ka
import kron_ref as kr

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
    capi, meshgen, workloads = env
    if isinstance(mesh, str):
        return workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", mesh))
    return getattr(meshgen, mesh[0])(mesh[1])


def _fresh(env, mesh="unit_square_16", order=1):
    capi = env[0]
    nodes, cells, bnd = _mesh(env, mesh)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(order)
    c.tune("amg_coarse_rows", ka.COARSE_ROWS)
    return c, nd, nodes


_spaces, _systems = {}, {}


def _space(env, mesh, order):
    """one context with assembled R1 = stiff(-laplacian) and R0 = mass per (mesh, order), shared by the tests (each computes its own handle)"""
    key = (mesh, order)
    if key not in _spaces:
        capi = env[0]
        c, nd, nodes = _fresh(env, mesh, order)
        c.set_operator(-capi.laplacian())
        c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
        c.init()
        rp, ci = c.pattern_get()
        _spaces[key] = dict(c=c, nd=nd, rp=rp, ci=ci, r1=c.matrix_values(capi.MAT_STIFF), r0=c.matrix_values(capi.MAT_MASS), obs=br.observed_nodes(nodes.shape[0]))
    return _spaces[key]


def _system(env, case, lu=True):
    """-> (context with the handle computed, A, b, n_dofs, q, LU solution or None, terms, space); the matrix and its factorisation once per case"""
    import scipy.sparse.linalg as spl

    sp_ = _space(env, case[1], case[2])
    if case not in _systems:
        terms, q, b = ka.system(case, sp_["rp"], sp_["ci"], sp_["r1"], sp_["r0"], sp_["obs"])
        A = kr.explicit(terms, sp_["rp"], sp_["ci"], sp_["nd"])
        _systems[case] = (terms, q, b, A, spl.splu(A.tocsc()).solve(b) if lu else None)
    terms, q, b, A, x_lu = _systems[case]
    sp_["c"].kron_compute(terms)   # (the context is shared: its handle may hold another test's matrix)
    return sp_["c"], A, b, sp_["nd"], q, x_lu, terms, sp_


def _rel(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


def _residual_ld(A, b, x):
    """|b - A x| / |b| with the products and sums in np.longdouble"""
    y, _ = kr.matvec_ld(A, x)
    r = np.asarray(b, dtype=np.longdouble) - y
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(np.asarray(b, dtype=np.longdouble) ** 2)))


def _check(env, case, lu=True):
    capi = env[0]
    c, A, b, nd, q, x_lu, terms, sp_ = _system(env, case, lu)
    budget = ka.budget(case)
    x, info = c.kron_solve(b, method=capi.SOLVER_KRON_AMG, rtol=ka.RTOL, maxit=budget, raise_on_noconv=False)
    h = c.kron_amg_hierarchy()
    rows_ref = ka.Hierarchy(sp_["rp"], sp_["ci"], terms, nd).rows if lu else []   # (the ladders' restatements: tests/test_kron_amg_cpu.py)
    res = _residual_ld(A, b, x)
    err = _rel(x, x_lu) if lu else float("nan")
    print(f"{ka.case_id(case)}: q n = {q * nd}, rows per level {h['rows']} (restatement {rows_ref}), absorbed {h['absorbed']}, iterations {info.iters} "
          f"(budget {budget}), relres {info.relres:.3e}, recomputed {res:.3e}, error against LU {err:.2e}")
    assert info.converged == 1 and info.method_used == capi.SOLVER_KRON_AMG == 10 and info.persistent == 0
    assert 0 < info.iters <= budget
    assert info.relres <= ka.RTOL
    assert res <= ka.RTOL
    if lu:
        assert err <= 1e-6
    assert h["rows"][0] == q * nd and all(r % q == 0 for r in h["rows"])
    if len(rows_ref) >= 3:
        assert len(h["rows"]) >= 3
    return info.iters


# ---- 1. the space-time and the parabolic systems --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ka.SPACETIME_CASES + ka.PARABOLIC_CASES, ids=[ka.case_id(c) for c in ka.SPACETIME_CASES + ka.PARABOLIC_CASES])
def test_spacetime_and_parabolic_against_lu(env, case):
    """budget 80 (P1) / 160 (2-D P2), the restatement stays under half: converged, relres <= rtol, the true residual recomputed in np.longdouble <= rtol, the
    solution within 1e-6 of SuperLU, at least three levels where the restatement has them"""
    _check(env, case)


# ---- 2. the team widths ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ka.WIDTH_CASES, ids=[ka.case_id(c) for c in ka.WIDTH_CASES])
def test_widths_that_can_go_wrong(env, case):
    """289 rows (a partly empty last workgroup at every width): q = 1 (a team of two, one idle lane), 2, 3, 5, 33 (a team of 64, 31 idle lanes), 10, 16, 64, and
    a dense T (no band to skip)"""
    assert _space(env, case[1], case[2])["nd"] == 289
    _check(env, case)


# ---- 3. the ladders -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ladder", ka.LADDERS, ids=[c[0][1][0] for c in ka.LADDERS])
def test_ladder(env, ladder):
    """outer iterations over a ladder of meshes: every count <= 40, the largest mesh's <= 1.5 x the smallest's + 2"""
    counts = [_check(env, case, lu=False) for case in ladder]
    print(f"{ladder[0][1][0]}: iterations {counts}")
    assert max(counts) <= ka.LADDER_CAP
    assert counts[-1] <= 1.5 * counts[0] + 2


# ---- 4. the same bits -----------------------------------------------------------------------------------------------------------------------------------
def test_same_bits_twice_and_after_a_rebuild(env):
    capi = env[0]
    c, A, b, nd, q, x_lu, terms, _ = _system(env, ka.SPACETIME_CASES[1])
    x1, i1 = c.kron_solve(b, method=capi.SOLVER_KRON_AMG, rtol=ka.RTOL, maxit=ka.BUDGET_P1)
    x2, i2 = c.kron_solve(b, method=capi.SOLVER_KRON_AMG, rtol=ka.RTOL, maxit=ka.BUDGET_P1)
    assert np.array_equal(x1, x2) and i1.iters == i2.iters
    c.tune("kron_amg_term", 3)   # drops the hierarchy ...
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_amg_hierarchy()
    assert e.value.status == capi.ENOTINIT
    c.tune("kron_amg_term", -1)
    x3, i3 = c.kron_solve(b, method=capi.SOLVER_KRON_AMG, rtol=ka.RTOL, maxit=ka.BUDGET_P1)   # ... and this solve builds it again
    assert np.array_equal(x1, x3) and i1.iters == i3.iters
    B = np.column_stack([b, kr.spacetime_rhs(_space(env, "unit_square_16", 1)["obs"], 1e-4, nd, q // 2, seed=2)])
    X, info = c.kron_solve(B, method=capi.SOLVER_KRON_AMG, rtol=ka.RTOL, maxit=ka.BUDGET_P1)   # columns one after another, iters summed
    xb, ib = c.kron_solve(B[:, 1], method=capi.SOLVER_KRON_AMG, rtol=ka.RTOL, maxit=ka.BUDGET_P1)
    assert np.array_equal(X[:, 0], x1) and np.array_equal(X[:, 1], xb) and info.iters == i1.iters + ib.iters


# ---- 5. the block handle as yardstick -------------------------------------------------------------------------------------------------------------------
def _unit(r, c_):
    T = np.zeros((2, 2))
    T[r, c_] = 1.0
    return T


def test_q2_reproduces_the_block_handles_hierarchy(env):
    """q = 2, four unit-T terms on the four blocks of the smoothing system, kron_amg_term naming the (2,1) term: the strength values and the rules are those
    of FDAPDE_SOLVER_BLOCK_AMG, so the rows per level and the aggregates of every level are equal array for array; both solutions within 1e-6 of SuperLU"""
    import scipy.sparse.linalg as spl

    capi = env[0]
    sp_ = _space(env, ("unit_square", 32), 1)   # (2 n = 2 178: aggregates on more than one level)
    c, nd, rp, ci = sp_["c"], sp_["nd"], sp_["rp"], sp_["ci"]
    blocks = br.smoothing_blocks(rp, ci, sp_["r1"], sp_["r0"], sp_["obs"], 1e-4, nd)
    b = br.smoothing_rhs(sp_["obs"], 1e-4, nd)
    x_lu = spl.splu(br.bmat(rp, ci, blocks, nd).tocsc()).solve(b)
    c.block_compute(*blocks, symmetric=True)
    c.kron_compute([(_unit(k // 2, k % 2), blocks[k]) for k in range(4)], symmetric=True)
    c.tune("kron_amg_term", 2)
    try:
        xk, ik = c.kron_solve(b, method=capi.SOLVER_KRON_AMG, rtol=ka.RTOL, maxit=ka.BUDGET_P1)
        xb, ib = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ka.RTOL, maxit=ka.BUDGET_P1)
        hk, hb = c.kron_amg_hierarchy(), c.amg_hierarchy(capi.AMG_OF_BLOCK)
        print(f"rows per level {hk['rows']} (block handle {hb['rows']}), iterations {ik.iters} (block handle {ib.iters})")
        assert hk["rows"] == hb["rows"] and hk["nnz"] == hb["nnz"] and hk["absorbed"] == hb["absorbed"] and len(hk["rows"]) >= 3
        for level in range(len(hk["rows"]) - 1):
            assert np.array_equal(c.kron_amg_aggregates(level), c.amg_aggregates(capi.AMG_OF_BLOCK, level))
        assert _rel(xk, x_lu) <= 1e-6 and _rel(xb, x_lu) <= 1e-6
    finally:
        c.tune("kron_amg_term", -1)


# ---- 6. / 7. the set-up knobs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob,value", [("amg_setup_check", 1), ("amg_absorb", 1), ("amg_absorb", 0)])
def test_under_the_set_up_knobs(env, knob, value):
    """amg_setup_check 1: every level step (aggregates, coarse pattern, strength values and the n_S spatial values per coarse entry) equals the host loops bit
    for bit, or the solve fails; amg_absorb 1 and 0: the case converges under both, and the hierarchy says which it was built under"""
    capi = env[0]
    case = ka.PARABOLIC_CASES[0]
    c, nd, _ = _fresh(env)
    _system(env, case)
    terms, q, b, A, x_lu = _systems[case]
    c.tune(knob, value)
    c.kron_compute(terms)
    x, info = c.kron_solve(b, method=capi.SOLVER_KRON_AMG, rtol=ka.RTOL, maxit=ka.BUDGET_P1)
    h = c.kron_amg_hierarchy()
    print(f"{knob} {value}: rows per level {h['rows']}, absorbed {h['absorbed']}, iterations {info.iters}")
    assert info.converged == 1 and info.iters <= ka.BUDGET_P1 and _rel(x, x_lu) <= 1e-6 and _residual_ld(A, b, x) <= ka.RTOL
    if knob == "amg_absorb":
        assert h["absorbed"] == value
    c.close()


# ---- 8. lifetime and errors -----------------------------------------------------------------------------------------------------------------------------
def _no_hierarchy(capi, c):
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_amg_hierarchy()
    return e.value.status == capi.ENOTINIT


def test_lifetime_of_the_hierarchy(env):
    capi = env[0]
    case = ka.PARABOLIC_CASES[0]
    _system(env, case)
    terms, q, b, A, x_lu = _systems[case]
    c, nd, _ = _fresh(env)
    c.kron_compute(terms)
    assert _no_hierarchy(capi, c)   # (built by the first solve that names the method)
    c.kron_solve(b, method=capi.SOLVER_GMRES)
    assert _no_hierarchy(capi, c)
    c.kron_solve(b, method=capi.SOLVER_KRON_AMG)
    assert len(c.kron_amg_hierarchy()["rows"]) >= 3
    with pytest.raises(capi.FdapdeError) as e:   # (the last level has no next one)
        c.kron_amg_aggregates(len(c.kron_amg_hierarchy()["rows"]) - 1)
    assert e.value.status == capi.EINVAL
    k = c.clone()   # the clone carries neither the handle nor its hierarchy
    assert _no_hierarchy(capi, k)
    k.close()
    c.tune("amg_absorb", 1)   # a change of amg_absorb drops the live hierarchies
    assert _no_hierarchy(capi, c)
    c.tune("amg_absorb", 2)
    c.kron_solve(b, method=capi.SOLVER_KRON_AMG)
    c.kron_amg_hierarchy()
    c.kron_compute(terms)
    assert _no_hierarchy(capi, c)
    c.kron_solve(b, method=capi.SOLVER_KRON_AMG)
    c.kron_amg_hierarchy()
    c.dofs_build(1)
    assert _no_hierarchy(capi, c)
    c.close()


def test_refusals(env):
    capi = env[0]
    case = ka.PARABOLIC_CASES[0]
    _system(env, case)
    terms, q, b, A, x_lu = _systems[case]
    sp_ = _space(env, case[1], case[2])
    c, nd, _ = _fresh(env)
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    # the other four solve entry points
    with pytest.raises(capi.FdapdeError) as e:
        c.solve(method=capi.SOLVER_KRON_AMG)
    assert e.value.status == capi.EUNSUPPORTED
    with pytest.raises(capi.FdapdeError) as e:
        c.solve_parabolic(np.linspace(0.0, 0.1, 3), np.zeros(nd), method=capi.SOLVER_KRON_AMG)
    assert e.value.status == capi.EUNSUPPORTED
    c.lin_compute(capi.MAT_STIFF)
    with pytest.raises(capi.FdapdeError) as e:
        c.lin_solve(np.ones(nd), method=capi.SOLVER_KRON_AMG)
    assert e.value.status == capi.EUNSUPPORTED
    blocks = br.smoothing_blocks(sp_["rp"], sp_["ci"], sp_["r1"], sp_["r0"], sp_["obs"], 1e-4, nd)
    c.block_compute(*blocks, symmetric=True)
    with pytest.raises(capi.FdapdeError) as e:
        c.block_solve(np.ones(2 * nd), method=capi.SOLVER_KRON_AMG)
    assert e.value.status == capi.EUNSUPPORTED
    # no D^-1 within the budget
    c.tune("kron_dinv_mb", 0)
    c.kron_compute(terms)
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(b, method=capi.SOLVER_KRON_AMG)
    assert e.value.status == capi.EUNSUPPORTED and "kron_dinv_mb" in str(e.value)
    assert str(e.value) == (f"[status {capi.EUNSUPPORTED}] FDAPDE_SOLVER_KRON_AMG: the inverted diagonal blocks (8 q^2 n bytes) exceed the budget `kron_dinv_mb`: "
                            "no block-Jacobi smoother")
    c.tune("kron_dinv_mb", 2048)
    c.kron_compute(terms)
    # a term the handle was not given
    c.tune("kron_amg_term", len(terms))
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(b, method=capi.SOLVER_KRON_AMG)
    assert e.value.status == capi.EINVAL
    with pytest.raises(capi.FdapdeError) as e:
        c.tune("kron_amg_term", 8)
    assert e.value.status == capi.EINVAL
    c.tune("kron_amg_term", -1)
    x, info = c.kron_solve(b, method=capi.SOLVER_KRON_AMG)
    assert info.converged == 1 and _rel(x, x_lu) <= 1e-6
    # one singular diagonal block (tests/test_gpu_kron.py's): no smoother
    S = sp_["r0"] + 0.1 * sp_["r1"]
    i = 7
    S[sp_["rp"][i] + np.searchsorted(sp_["ci"][sp_["rp"][i]:sp_["rp"][i + 1]], i)] = 0.0
    c.kron_compute([(np.random.default_rng(3).standard_normal((3, 3)) + 4.0 * np.eye(3), S)])
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(np.ones(3 * nd), method=capi.SOLVER_KRON_AMG)
    assert e.value.status == capi.EUNSUPPORTED and "diagonal block is singular" in str(e.value)
    assert str(e.value) == (f"[status {capi.EUNSUPPORTED}] FDAPDE_SOLVER_KRON_AMG: a DOF's diagonal block is singular (a pivot <= 1e-14 max|entry|): "
                            "no block-Jacobi smoother")
    c.close()


def test_the_gmres_stage_keeps_its_bits(env):
    """a GMRES solve before and after a KRON_AMG solve of the same handle: identical bits and counts"""
    capi = env[0]
    c, A, b, nd, q, x_lu, terms, _ = _system(env, ka.SPACETIME_CASES[1])
    x0, i0 = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
    c.kron_solve(b, method=capi.SOLVER_KRON_AMG, rtol=ka.RTOL, maxit=ka.BUDGET_P1)
    x1, i1 = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
    y0 = c.kron_spmv(b)
    assert np.array_equal(x0, x1) and i0.iters == i1.iters and i1.method_used == capi.SOLVER_GMRES
    assert np.array_equal(y0, c.kron_spmv(b))
