"""The texts of the three multilevel solvers' set-up (the build passes of csrc/eng_amg.hip, eng_block_amg.hip, eng_kron_amg.hip and the skeleton they share in
csrc/amg_setup.h) and of FDAPDE_SOLVER_AMG's endings without convergence: for each, the status, the whole message and the method the record names.
unit_square_16 P1, 289 DOFs, with `amg_coarse_rows`, `dense_rows` and `kron_dinv_mb` tuned down so that several levels and the limits are reached at that size
(tests/test_gpu_handle_driver.py pins the solve-time refusals and the endings of the two handles).

Not reached at a few thousand rows, hence not here: FDAPDE_SOLVER_AMG's "coarsening stalled above the dense limit" (its limit is the constant 8192 rows:
tests/test_gpu_amg_absorb.py reaches it at full size and holds the whole text there) and the two "the coarsest level is too large for the dense inverse" (a
hierarchy ends on a level within min(dense_rows, 8192) rows or within `amg_coarse_rows`: no input reaches them).  The block pass's "a DOF's diagonal block is
singular" is its handle's refusal word for word, and the handle gives it first (tests/test_gpu_handle_driver.py, tests/test_gpu_block_amg.py hold it)."""
import os

import numpy as np
import pytest

import block_ref as br

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND = 289
STALL = "coarsening stalled above the dense limit (a level kept more than 0.8 of its rows): the %s has too few strong couplings for pairwise aggregation"
CUT = "a coarse level has a singular diagonal block and the level above it is too large for the dense inverse"


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, workloads

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, workloads


def _fresh(env, coarse_rows=64):
    capi, workloads = env
    c = capi.Context(0)
    c.mesh_upload(*workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16")))
    assert c.dofs_build(1) == ND
    c.tune("amg_coarse_rows", coarse_rows)
    return c


@pytest.fixture(scope="module")
def space(env):
    """pattern, R1 = stiff(-laplacian) (pure Neumann: singular, its null space the constants), R0 = mass, the slots of the diagonal"""
    capi, _ = env
    c = _fresh(env)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    rp, ci = c.pattern_get()
    diag = np.array([rp[i] + np.searchsorted(ci[rp[i]:rp[i + 1]], i) for i in range(ND)])
    sp_ = dict(rp=rp, ci=ci, r1=c.matrix_values(capi.MAT_STIFF), r0=c.matrix_values(capi.MAT_MASS), diag=diag, obs=br.observed_nodes(ND))
    c.close()
    return sp_


def _refused(capi, c, call, status, text, method):
    with pytest.raises(capi.FdapdeError) as e:
        call()
    assert e.value.status == status
    assert str(e.value) == f"[status {status}] {text}"
    assert c.info().method_used == method


def _diagonal_only(sp_):
    """1 on the diagonal, 0 on every other entry of the pattern: no coupling to aggregate along"""
    v = np.zeros(len(sp_["ci"]))
    v[sp_["diag"]] = 1.0
    return v


def _levels(c, capi, which):
    return c.amg_hierarchy(which)["rows"]


# ---- FDAPDE_SOLVER_AMG: the build pass and level_prepare ---------------------------------------------------------------------------------------------------
def test_scalar_coarsest_level_singular(env):
    """-Lap without Dirichlet data: every Galerkin level keeps the constants in its null space, the coarsest has no inverse"""
    capi, _ = env
    c = _fresh(env)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    _refused(capi, c, lambda: c.solve(method=capi.SOLVER_AMG), capi.ENOCONV,
             "FDAPDE_SOLVER_AMG: the coarsest level is singular to working precision (a pure Neumann problem has no unique solution)", capi.SOLVER_AMG)
    c.close()


def test_scalar_no_free_rows(env):
    """every DOF a Dirichlet DOF: level 0 is above `amg_coarse_rows` and has no row to aggregate"""
    capi, _ = env
    c = _fresh(env)
    c.dofs_set_boundary(np.ones(ND, dtype=np.uint8))
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.set_dirichlet(np.zeros(ND))
    c.init()
    _refused(capi, c, lambda: c.solve(method=capi.SOLVER_AMG), capi.EUNSUPPORTED, "FDAPDE_SOLVER_AMG: a level above the dense limit has no free rows to aggregate",
             capi.SOLVER_AMG)
    c.close()


def test_scalar_zero_diagonal_entry(env, space):
    capi, _ = env
    c = _fresh(env)
    v = space["r0"] + 0.1 * space["r1"]
    v[space["diag"][7]] = 0.0
    c.lin_compute(values=v, symmetric=True)
    _refused(capi, c, lambda: c.lin_solve(np.ones(ND), method=capi.SOLVER_AMG), capi.EUNSUPPORTED,
             "FDAPDE_SOLVER_AMG: a level has a zero diagonal entry (its damped Jacobi smoother needs one)", capi.SOLVER_AMG)
    c.close()


# ---- FDAPDE_SOLVER_AMG: the endings without convergence ----------------------------------------------------------------------------------------------------
def test_scalar_endings_without_convergence(env, space):
    capi, _ = env
    c = _fresh(env)
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    _refused(capi, c, lambda: c.solve(method=capi.SOLVER_AMG, rtol=1e-15, maxit=1), capi.ENOCONV, "FDAPDE_SOLVER_AMG: maxit reached", capi.SOLVER_AMG)
    assert len(_levels(c, capi, capi.AMG_OF_SOLVE)) > 1 and c.info().converged == 0
    c.lin_compute(values=space["r0"] + 0.1 * space["r1"], symmetric=True)
    B = np.random.default_rng(2).standard_normal((ND, 3))
    for cols in (8, 1):   # a batch of two and a last column alone; every column alone
        c.tune("amg_cols", cols)
        _refused(capi, c, lambda: c.lin_solve(B, method=capi.SOLVER_AMG, rtol=1e-15, maxit=1), capi.ENOCONV, "FDAPDE_SOLVER_AMG: maxit reached in at least one column",
                 capi.SOLVER_AMG)
        assert c.info().converged == 0
    c.close()


# ---- FDAPDE_SOLVER_BLOCK_AMG ------------------------------------------------------------------------------------------------------------------------------
def _block(env, sp_, blocks, dense_rows=None):
    c = _fresh(env)
    if dense_rows is not None:
        c.tune("dense_rows", dense_rows)
    c.block_compute(*blocks)
    return c


def test_block_stall(env, space):
    """the strength block (2,1) couples no two DOFs and 2 n = 578 rows are above `dense_rows`: with or without absorption (the default tries both) no level step
    shrinks level 0"""
    capi, _ = env
    S = space["r0"] + 0.1 * space["r1"]
    for absorb in (2, 0, 1):
        c = _block(env, space, (S, _diagonal_only(space), _diagonal_only(space), S), dense_rows=2 * ND - 1)
        c.tune("amg_absorb", absorb)
        _refused(capi, c, lambda: c.block_solve(np.ones(2 * ND), method=capi.SOLVER_BLOCK_AMG), capi.EUNSUPPORTED, "FDAPDE_SOLVER_BLOCK_AMG: " + STALL % "strength block",
                 capi.SOLVER_BLOCK_AMG)
        c.close()


def _aggregate_of(c, capi, which, i):
    agg = c.amg_aggregates(which, 0)
    return np.flatnonzero(agg == agg[i])


def _entries_within(sp_, members):
    """the slots of the pattern's entries (i, j) with i and j both in `members`: what the Galerkin product sums into their aggregate's diagonal entry"""
    rp, ci = sp_["rp"], sp_["ci"]
    return np.array([k for i in members for k in range(rp[i], rp[i + 1]) if ci[k] in members])


def test_block_coarse_singular_diagonal_block(env, space):
    """[S, 0; S, S] with S = R0 + 0.1 R1, then a11 lowered on the diagonal of one DOF by the sum of a11 over its aggregate: level 1's diagonal block of that
    aggregate is [~0, 0; s, s] -- singular -- while level 0's blocks stay regular, and the aggregates (read from a first build: they come from the off-diagonal
    entries of the strength block (2,1) alone) do not move.  With 2 n above `dense_rows` the hierarchy cannot end on level 0: refused; within it the hierarchy ends
    there and the solve answers through level 0's inverse"""
    capi, _ = env
    S = space["r0"] + 0.1 * space["r1"]
    b = np.random.default_rng(4).standard_normal(2 * ND)
    c = _block(env, space, (S, None, S, S))
    c.block_solve(b, method=capi.SOLVER_BLOCK_AMG)
    assert len(_levels(c, capi, capi.AMG_OF_BLOCK)) >= 3
    members = _aggregate_of(c, capi, capi.AMG_OF_BLOCK, 7)
    c.close()
    a11 = S.copy()
    a11[space["diag"][7]] -= S[_entries_within(space, set(members.tolist()))].sum()
    assert abs(a11[space["diag"][7]]) > 0.1 * S[space["diag"][7]]   # (level 0's block of that DOF is far from singular)
    c = _block(env, space, (a11, None, S, S), dense_rows=2 * ND - 1)
    _refused(capi, c, lambda: c.block_solve(b, method=capi.SOLVER_BLOCK_AMG), capi.EUNSUPPORTED, "FDAPDE_SOLVER_BLOCK_AMG: " + CUT, capi.SOLVER_BLOCK_AMG)
    c.tune("dense_rows", 8192)
    c.block_compute(a11, None, S, S)
    x, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG)
    assert info.converged == 1 and info.method_used == capi.SOLVER_BLOCK_AMG and _levels(c, capi, capi.AMG_OF_BLOCK) == [2 * ND]
    c.close()


def test_block_coarsest_level_singular(env, space):
    """[R1, 0; 0, R1], the Neumann stiffness matrix twice: regular diagonal blocks on every level, no inverse on the last"""
    capi, _ = env
    c = _block(env, space, (space["r1"], None, None, space["r1"]))
    _refused(capi, c, lambda: c.block_solve(np.ones(2 * ND), method=capi.SOLVER_BLOCK_AMG), capi.ENOCONV,
             "FDAPDE_SOLVER_BLOCK_AMG: the coarsest level is singular to working precision", capi.SOLVER_BLOCK_AMG)
    c.close()


# ---- FDAPDE_SOLVER_KRON_AMG -------------------------------------------------------------------------------------------------------------------------------
def test_kron_stall(env, space):
    """a spatial factor that couples no two DOFs, q n = 578 rows above `dense_rows`"""
    capi, _ = env
    c = _fresh(env)
    c.tune("dense_rows", 2 * ND - 1)
    c.kron_compute([(np.array([[4.0, 1.0], [0.5, 3.0]]), _diagonal_only(space))])
    _refused(capi, c, lambda: c.kron_solve(np.ones(2 * ND), method=capi.SOLVER_KRON_AMG), capi.EUNSUPPORTED, "FDAPDE_SOLVER_KRON_AMG: " + STALL % "strength matrix",
             capi.SOLVER_KRON_AMG)
    c.close()


def test_kron_budget_of_all_levels(env, space):
    """q = 20 under `kron_dinv_mb` = 1: level 0's D^-1 (8 q^2 n = 924 800 bytes) is within the MiB and the handle has its Krylov stage; with the levels below it
    (n_1 >= n / 4 rows, another 231 200 bytes at least) the smoothers are not"""
    capi, _ = env
    q = 20
    c = _fresh(env, coarse_rows=256)
    c.tune("kron_dinv_mb", 1)
    rng = np.random.default_rng(q)
    c.kron_compute([(rng.standard_normal((q, q)) + 8.0 * np.eye(q), space["r0"] + 0.1 * space["r1"])])
    b = rng.standard_normal(q * ND)
    _refused(capi, c, lambda: c.kron_solve(b, method=capi.SOLVER_KRON_AMG), capi.EUNSUPPORTED,
             "FDAPDE_SOLVER_KRON_AMG: the inverted diagonal blocks of all levels (8 q^2 n_l bytes each) exceed the budget `kron_dinv_mb`", capi.SOLVER_KRON_AMG)
    x, info = c.kron_solve(b, method=capi.SOLVER_GMRES)
    assert info.converged == 1 and info.method_used == capi.SOLVER_GMRES
    c.close()


def test_kron_coarse_singular_diagonal_block(env, space):
    """diag(1, 0) (x) S1 + diag(0, 1) (x) S: a DOF's block is diag(S1[i, i], S[i, i]) on every level.  S1 = S with the diagonal of one DOF lowered by the sum of S
    over its aggregate (read from a first build; the strength matrix has no diagonal): level 1's block of that aggregate is diag(~0, s) -- singular --, level
    0's stay regular.  As the block form: refused where q n is above `dense_rows`, answered through level 0's inverse where it is not"""
    capi, _ = env
    S = space["r0"] + 0.1 * space["r1"]
    T1, T2 = np.diag([1.0, 0.0]), np.diag([0.0, 1.0])
    b = np.random.default_rng(5).standard_normal(2 * ND)
    c = _fresh(env)
    c.kron_compute([(T1, S), (T2, S)])
    c.kron_solve(b, method=capi.SOLVER_KRON_AMG)
    assert len(c.kron_amg_hierarchy()["rows"]) >= 3
    agg = c.kron_amg_aggregates(0)
    members = np.flatnonzero(agg == agg[7])
    c.close()
    S1 = S.copy()
    S1[space["diag"][7]] -= S[_entries_within(space, set(members.tolist()))].sum()
    assert abs(S1[space["diag"][7]]) > 0.1 * S[space["diag"][7]]
    c = _fresh(env)
    c.tune("dense_rows", 2 * ND - 1)
    c.kron_compute([(T1, S1), (T2, S)])
    _refused(capi, c, lambda: c.kron_solve(b, method=capi.SOLVER_KRON_AMG), capi.EUNSUPPORTED, "FDAPDE_SOLVER_KRON_AMG: " + CUT, capi.SOLVER_KRON_AMG)
    c.tune("dense_rows", 8192)
    c.kron_compute([(T1, S1), (T2, S)])
    x, info = c.kron_solve(b, method=capi.SOLVER_KRON_AMG)
    assert info.converged == 1 and info.method_used == capi.SOLVER_KRON_AMG and c.kron_amg_hierarchy()["rows"] == [2 * ND]
    c.close()


def test_kron_coarsest_level_singular(env, space):
    """I_2 (x) R1: regular diagonal blocks on every level, no inverse on the last"""
    capi, _ = env
    c = _fresh(env)
    c.kron_compute([(np.eye(2), space["r1"])])
    _refused(capi, c, lambda: c.kron_solve(np.ones(2 * ND), method=capi.SOLVER_KRON_AMG), capi.ENOCONV,
             "FDAPDE_SOLVER_KRON_AMG: the coarsest level is singular to working precision", capi.SOLVER_KRON_AMG)
    c.close()
