"""The solve driver the 2 x 2 block handle and the Kronecker-sum handle share (csrc/eng_handle.h): every refusal of fdapde_block_solve and fdapde_kron_solve
with its status and its full text -- written out here as the handles worded them before they shared a driver --, the dense stage with more columns than one
slice of the staging buffer holds, and one call with the method open that crosses from the Krylov stage to the dense inverse.  unit_square_16 P1, 289 DOFs."""
import os

import numpy as np
import pytest

import block_ref as br

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND = 289


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, workloads

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, workloads


@pytest.fixture(scope="module")
def space(env):
    """pattern, R1 = stiff(-laplacian), R0 = mass and the observed nodes of the fixture, computed once"""
    capi, _ = env
    c = _fresh(env, dofs=True)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    rp, ci = c.pattern_get()
    sp_ = dict(rp=rp, ci=ci, r1=c.matrix_values(capi.MAT_STIFF), r0=c.matrix_values(capi.MAT_MASS), obs=br.observed_nodes(ND))
    c.close()
    return sp_


def _fresh(env, dofs=True):
    capi, workloads = env
    c = capi.Context(0)
    c.mesh_upload(*workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16")))
    if dofs:
        assert c.dofs_build(1) == ND
        c.tune("amg_coarse_rows", 256)   # (as test_gpu_block_amg.py: a 289-DOF system gets several levels)
    return c


def _diag_slot(sp_, i=7):
    rp, ci = sp_["rp"], sp_["ci"]
    return rp[i] + np.searchsorted(ci[rp[i]:rp[i + 1]], i)


def _block(env, sp_, singular=False):
    """the smoothing system's handle (test_gpu_block.py); singular: a11 = a12 = 0 on the diagonal of one DOF, as test_singular_diagonal_block"""
    c = _fresh(env)
    blocks = [v.copy() for v in br.smoothing_blocks(sp_["rp"], sp_["ci"], sp_["r1"], sp_["r0"], sp_["obs"], 1e-2, ND)]
    if singular:
        blocks[0][_diag_slot(sp_)] = 0.0
        blocks[1][_diag_slot(sp_)] = 0.0
    c.block_compute(*blocks)
    return c, br.smoothing_rhs(sp_["obs"], 1e-2, ND)


def _kron(env, sp_, q=3, singular=False, tune=()):
    """one term T (x) S, S = R0 + 0.1 R1; singular: S[i, i] = 0 at one DOF, as test_kron_one_singular_diagonal_block"""
    c = _fresh(env)
    for key, value in tune:
        c.tune(key, value)
    rng = np.random.default_rng(q)
    S = sp_["r0"] + 0.1 * sp_["r1"]
    if singular:
        S[_diag_slot(sp_)] = 0.0
    c.kron_compute([(rng.standard_normal((q, q)) + 4.0 * np.eye(q), S)])
    return c, rng.standard_normal(q * ND)


def _psi(sp_):
    import scipy.sparse as sp

    obs = np.asarray(sp_["obs"])
    return sp.csr_matrix((np.ones(len(obs)), (np.arange(len(obs)), obs)), shape=(len(obs), ND))


def _refused(capi, call, status, text):
    with pytest.raises(capi.FdapdeError) as e:
        call()
    assert e.value.status == status
    assert str(e.value) == f"[status {status}] {text}"


SINGULAR_DENSE = "FDAPDE_SOLVER_DENSE: the %s matrix is singular to working precision (no usable pivot, or max |I - A X| beyond 1e-6)"
TOO_LARGE = "a DOF's diagonal block is singular: no block-Jacobi form for the Krylov stage, and the system is too large for the dense inverse"


# ---- (a) the refusals -----------------------------------------------------------------------------------------------------------------------------
def test_block_refusals_before_a_handle(env):
    capi, _ = env
    b = np.ones(2 * ND)
    c = _fresh(env, dofs=False)
    _refused(capi, lambda: c.block_solve(b), capi.ENOTINIT, "call fdapde_dofs_build first")
    c.close()
    c = _fresh(env)
    _refused(capi, lambda: c.block_solve(b), capi.ENOTINIT, "call fdapde_block_compute first")
    c.comm_init_callback(2, 0, lambda a: None)
    _refused(capi, lambda: c.block_solve(b), capi.EUNSUPPORTED, "the 2 x 2 block handle takes one-GPU contexts, not a rank of a multi-GPU job")
    c.close()


def test_kron_refusals_before_a_handle(env):
    capi, _ = env
    b = np.ones(2 * ND)
    c = _fresh(env, dofs=False)
    _refused(capi, lambda: c.kron_solve(b), capi.ENOTINIT, "call fdapde_dofs_build first")
    c.close()
    c = _fresh(env)
    _refused(capi, lambda: c.kron_solve(b), capi.ENOTINIT, "call fdapde_kron_compute first")
    c.comm_init_callback(2, 0, lambda a: None)
    _refused(capi, lambda: c.kron_solve(b), capi.EUNSUPPORTED, "the Kronecker-sum handle takes one-GPU contexts, not a rank of a multi-GPU job")
    c.close()


def test_block_refusals_of_a_regular_matrix(env, space):
    capi, _ = env
    c, b = _block(env, space)
    marker = c.block_solve(b, method=capi.SOLVER_DENSE)[1]   # the record of the last solve: a refusal that does not write it leaves it
    assert marker.method_used == capi.SOLVER_DENSE
    for method in (capi.SOLVER_CG, capi.SOLVER_BICGSTAB, capi.SOLVER_CG_SR, capi.SOLVER_CG_FUSED, capi.SOLVER_PMG, capi.SOLVER_AMG):
        _refused(capi, lambda: c.block_solve(b, method=method), capi.EUNSUPPORTED,
                 "fdapde_block_solve runs FDAPDE_SOLVER_GMRES, FDAPDE_SOLVER_DENSE, FDAPDE_SOLVER_BLOCK_AMG or the open method")
    c.tune("dense_rows", 2 * ND - 1)
    _refused(capi, lambda: c.block_solve(b, method=capi.SOLVER_DENSE), capi.EUNSUPPORTED, "FDAPDE_SOLVER_DENSE takes block systems of up to `dense_rows` (at most 8192) rows")
    for method in (capi.SOLVER_CG, capi.SOLVER_AMG):   # (the method's refusal comes before the size's)
        _refused(capi, lambda: c.block_solve(b, method=method), capi.EUNSUPPORTED,
                 "fdapde_block_solve runs FDAPDE_SOLVER_GMRES, FDAPDE_SOLVER_DENSE, FDAPDE_SOLVER_BLOCK_AMG or the open method")
    c.tune("dense_rows", 8192)
    assert c.info().method_used == capi.SOLVER_DENSE and c.info().t_solve_ms == marker.t_solve_ms
    _refused(capi, lambda: c.block_solve(b, method=capi.SOLVER_GMRES, maxit=20), capi.ENOCONV, "maxit reached in at least one column")
    assert c.info().method_used == capi.SOLVER_GMRES and c.info().converged == 0 and c.info().iters == 20
    _refused(capi, lambda: c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, maxit=1), capi.ENOCONV, "FDAPDE_SOLVER_BLOCK_AMG: maxit reached in at least one column")
    assert c.info().method_used == capi.SOLVER_BLOCK_AMG and c.info().converged == 0 and c.info().iters == 1
    c.block_set_obs(_psi(space))
    _refused(capi, lambda: c.block_solve(b, method=capi.SOLVER_BLOCK_AMG), capi.EUNSUPPORTED,
             "FDAPDE_SOLVER_BLOCK_AMG: a factored data term (fdapde_block_set_obs) is live; the hierarchy is built from pattern entries only unless the knob block_amg_obs is 1")
    assert c.info().iters == 1   # (the record of the call before)
    c.tune("block_amg_obs", 1)
    x, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG)   # the block handle's side of the table: with the knob the term is carried
    assert info.method_used == capi.SOLVER_BLOCK_AMG and info.converged == 1
    c.close()


def test_block_refusals_of_a_singular_diagonal_block(env, space):
    capi, _ = env
    c, b = _block(env, space, singular=True)
    marker = c.block_solve(b)[1]
    assert marker.method_used == capi.SOLVER_DENSE and marker.converged == 1   # the open method answers through the dense inverse
    _refused(capi, lambda: c.block_solve(b, method=capi.SOLVER_GMRES), capi.EUNSUPPORTED,
             "a DOF's diagonal block is singular (|det| <= 1e-14 max|entry|^2): no block-Jacobi form for the Krylov stage")
    _refused(capi, lambda: c.block_solve(b, method=capi.SOLVER_BLOCK_AMG), capi.EUNSUPPORTED,
             "FDAPDE_SOLVER_BLOCK_AMG: a DOF's diagonal block is singular (|det| <= 1e-14 max|entry|^2): no block-Jacobi smoother")
    c.tune("dense_rows", 2 * ND - 1)
    for method in (capi.SOLVER_AUTO, capi.SOLVER_GMRES):   # above the dense limit this text wins for GMRES by name too: its check comes first
        _refused(capi, lambda: c.block_solve(b, method=method), capi.EUNSUPPORTED, TOO_LARGE)
    info = c.info()   # info untouched by all four
    assert info.method_used == capi.SOLVER_DENSE and info.converged == 1 and info.t_solve_ms == marker.t_solve_ms
    c.close()


def test_block_dense_stage_on_a_singular_matrix(env, space):
    """both block rows the same: no inverse -- DENSE by name answers FDAPDE_ENOCONV and the record names the method"""
    capi, _ = env
    c = _fresh(env)
    v = space["r0"] + 0.1 * space["r1"]
    c.block_compute(v, v, v, v)
    b = np.random.default_rng(0).standard_normal(2 * ND)
    _refused(capi, lambda: c.block_solve(b, method=capi.SOLVER_DENSE), capi.ENOCONV, SINGULAR_DENSE % "block")
    assert c.info().method_used == capi.SOLVER_DENSE and c.info().converged == 0 and c.info().iters == 0
    c.close()


def test_kron_refusals_of_a_regular_matrix(env, space):
    capi, _ = env
    c, b = _kron(env, space)
    marker = c.kron_solve(b, method=capi.SOLVER_DENSE)[1]
    for method in (capi.SOLVER_CG, capi.SOLVER_BICGSTAB, capi.SOLVER_CG_SR, capi.SOLVER_CG_FUSED, capi.SOLVER_PMG, capi.SOLVER_AMG, capi.SOLVER_BLOCK_AMG):
        _refused(capi, lambda: c.kron_solve(b, method=method), capi.EUNSUPPORTED,
                 "fdapde_kron_solve runs FDAPDE_SOLVER_GMRES, FDAPDE_SOLVER_DENSE, FDAPDE_SOLVER_KRON_AMG or the open method")
    c.tune("dense_rows", 3 * ND - 1)
    _refused(capi, lambda: c.kron_solve(b, method=capi.SOLVER_DENSE), capi.EUNSUPPORTED, "FDAPDE_SOLVER_DENSE takes Kronecker systems of up to `dense_rows` (at most 8192) rows")
    c.tune("dense_rows", 8192)
    c.tune("kron_amg_term", 1)   # the handle has one term
    _refused(capi, lambda: c.kron_solve(b, method=capi.SOLVER_KRON_AMG), capi.EINVAL, "FDAPDE_SOLVER_KRON_AMG: the knob `kron_amg_term` names a term the handle was not given")
    c.tune("kron_amg_term", -1)
    assert c.info().method_used == capi.SOLVER_DENSE and c.info().t_solve_ms == marker.t_solve_ms
    _refused(capi, lambda: c.kron_solve(b, method=capi.SOLVER_GMRES, maxit=2), capi.ENOCONV, "maxit reached in at least one column")
    assert c.info().method_used == capi.SOLVER_GMRES and c.info().converged == 0 and c.info().iters == 2
    _refused(capi, lambda: c.kron_solve(b, method=capi.SOLVER_KRON_AMG, rtol=1e-15, maxit=1), capi.ENOCONV, "FDAPDE_SOLVER_KRON_AMG: maxit reached in at least one column")
    assert c.info().method_used == capi.SOLVER_KRON_AMG and c.info().converged == 0 and c.info().iters == 1
    c.kron_set_obs(_psi(space))
    _refused(capi, lambda: c.kron_solve(b, method=capi.SOLVER_KRON_AMG), capi.EUNSUPPORTED,
             "FDAPDE_SOLVER_KRON_AMG: a factored data term (fdapde_kron_set_obs) is live; the hierarchy is built from pattern entries only")
    assert c.info().iters == 1   # (the record of the call before)
    c.close()


def test_kron_refusals_of_a_singular_diagonal_block(env, space):
    capi, _ = env
    c, b = _kron(env, space, singular=True)
    marker = c.kron_solve(b)[1]
    assert marker.method_used == capi.SOLVER_DENSE and marker.converged == 1
    _refused(capi, lambda: c.kron_solve(b, method=capi.SOLVER_KRON_AMG), capi.EUNSUPPORTED,
             "FDAPDE_SOLVER_KRON_AMG: a DOF's diagonal block is singular (a pivot <= 1e-14 max|entry|): no block-Jacobi smoother")
    c.tune("dense_rows", 3 * ND - 1)
    _refused(capi, lambda: c.kron_solve(b), capi.EUNSUPPORTED, TOO_LARGE)
    assert c.info().method_used == capi.SOLVER_DENSE and c.info().t_solve_ms == marker.t_solve_ms   # info untouched so far
    for dense_rows in (3 * ND - 1, 8192):   # GMRES by name: FDAPDE_ENOCONV whatever the size, and the record names the method first
        c.tune("dense_rows", dense_rows)
        _refused(capi, lambda: c.kron_solve(b, method=capi.SOLVER_GMRES), capi.ENOCONV,
                 "a DOF's diagonal block is singular (a pivot <= 1e-14 max|entry|): no block-Jacobi form for the Krylov stage")
        info = c.info()
        assert info.method_used == capi.SOLVER_GMRES and info.converged == 0 and info.iters == 0 and info.relres == 0.0 and info.t_solve_ms == 0.0
    c.close()


def test_kron_refusals_over_the_dinv_budget(env, space):
    """kron_dinv_mb = 0: D^-1 is not built"""
    capi, _ = env
    c, b = _kron(env, space, tune=(("kron_dinv_mb", 0),))
    _refused(capi, lambda: c.kron_solve(b, method=capi.SOLVER_GMRES), capi.EUNSUPPORTED,
             "the inverted diagonal blocks (8 q^2 n bytes) exceed the budget `kron_dinv_mb`: no Krylov stage for this Kronecker handle")
    _refused(capi, lambda: c.kron_solve(b, method=capi.SOLVER_KRON_AMG), capi.EUNSUPPORTED,
             "FDAPDE_SOLVER_KRON_AMG: the inverted diagonal blocks (8 q^2 n bytes) exceed the budget `kron_dinv_mb`: no block-Jacobi smoother")
    x, info = c.kron_solve(b)   # the open method within the dense limit: the inverse, at once
    assert info.method_used == capi.SOLVER_DENSE and info.converged == 1
    c.tune("dense_rows", 3 * ND - 1)
    _refused(capi, lambda: c.kron_solve(b), capi.EUNSUPPORTED, "the inverted diagonal blocks exceed the budget `kron_dinv_mb`, and the system is too large for the dense inverse")
    c.close()


def test_kron_dense_stage_on_a_singular_matrix(env, space):
    """T singular: no inverse -- DENSE by name answers FDAPDE_ENOCONV and the record names the method"""
    capi, _ = env
    c = _fresh(env)
    c.kron_compute([(np.ones((2, 2)), space["r0"] + 0.1 * space["r1"])])
    b = np.random.default_rng(0).standard_normal(2 * ND)
    _refused(capi, lambda: c.kron_solve(b, method=capi.SOLVER_DENSE), capi.ENOCONV, SINGULAR_DENSE % "Kronecker")
    assert c.info().method_used == capi.SOLVER_DENSE and c.info().converged == 0 and c.info().iters == 0
    c.close()


# ---- the endings without convergence that name a breakdown ---------------------------------------------------------------------------------------------
GMRES_BROKE = "GMRES stagnated or broke down in at least one column"


def _stagnating(sp_):
    """S = R1, the Neumann stiffness matrix: singular, its null space the constants, every diagonal entry d_i > 0.  With D = diag(d) the Krylov stage solves
    D^-1 A z = D^-1 b, and for b = d^2 (entrywise) the right-hand side D^-1 b = d is orthogonal to the range D^-1 {y : sum y = 0} of the operator: no iterate
    lowers the residual, three cycles of 50 pass without progress, and the stage ends with its breakdown word set -- 150 iterations of the 2 000 allowed"""
    S = sp_["r1"].copy()
    d = S[[_diag_slot(sp_, i) for i in range(ND)]]
    assert d.min() > 0
    return S, np.concatenate([d * d, d * d])


def _broke(capi, c, solve, b, text, method, **kw):
    _refused(capi, lambda: solve(b, method=method, **kw), capi.ENOCONV, text)
    info = c.info()
    assert info.method_used == method and info.converged == 0
    return info


def test_block_endings_that_name_a_breakdown(env, space):
    capi, _ = env
    S, b = _stagnating(space)
    c = _fresh(env)
    c.block_compute(S, None, None, S)
    info = _broke(capi, c, c.block_solve, b, GMRES_BROKE, capi.SOLVER_GMRES)
    assert 0 < info.iters < 2000
    c.close()
    c, b = _block(env, space)   # a right-hand side with a non-finite entry: |b|^2 is not finite, the multilevel stage's column is broken before it starts
    bad = b.copy()
    bad[5] = np.inf
    text = "FDAPDE_SOLVER_BLOCK_AMG: the flexible GMRES broke down in at least one column"
    assert _broke(capi, c, c.block_solve, bad, text, capi.SOLVER_BLOCK_AMG).iters == 0
    _broke(capi, c, c.block_solve, np.column_stack([b, bad]), text, capi.SOLVER_BLOCK_AMG)   # ... and as one of a batch of two columns
    X, info = c.block_solve(np.column_stack([b, bad]), method=capi.SOLVER_BLOCK_AMG, raise_on_noconv=False)
    x, _ = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG)
    assert info.converged == 0 and np.array_equal(X[:, 0], x)   # (the column beside it is solved as alone)
    c.close()


def test_kron_endings_that_name_a_breakdown(env, space):
    capi, _ = env
    S, b = _stagnating(space)
    c = _fresh(env)
    c.kron_compute([(np.eye(2), S)])
    info = _broke(capi, c, c.kron_solve, b, GMRES_BROKE, capi.SOLVER_GMRES)
    assert 0 < info.iters < 2000
    c.close()
    c, b = _kron(env, space)
    b[5] = np.inf
    assert _broke(capi, c, c.kron_solve, b, "FDAPDE_SOLVER_KRON_AMG: the flexible GMRES broke down in at least one column", capi.SOLVER_KRON_AMG).iters == 0
    c.close()


# ---- (b) the dense stage in slices ----------------------------------------------------------------------------------------------------------------
def test_block_dense_stage_in_slices(env, space):
    """14 columns of 2 n = 578 words against a staging buffer of max(4 nnz, 2 n) words: more than one slice; every column as its one-column solve"""
    capi, _ = env
    c, _ = _block(env, space)
    per = max(4 * len(space["ci"]), 2 * ND) // (2 * ND)
    assert 1 <= per < 14
    B = np.random.default_rng(14).standard_normal((2 * ND, 14))
    X, info = c.block_solve(B, method=capi.SOLVER_DENSE)
    assert info.method_used == capi.SOLVER_DENSE and info.converged == 1
    for j in range(14):
        xj, ij = c.block_solve(B[:, j], method=capi.SOLVER_DENSE)
        assert ij.method_used == capi.SOLVER_DENSE and np.array_equal(xj, X[:, j])
    inplace = np.asfortranarray(B.copy())
    c.block_solve_inplace(inplace, method=capi.SOLVER_DENSE)
    assert np.array_equal(inplace, X)
    c.close()


def test_kron_dense_stage_in_slices(env, space):
    """q = 2 with four terms on four spatial factors: 14 columns of 578 words against max(4 nnz, 2 n) words"""
    capi, _ = env
    c = _fresh(env)
    rng = np.random.default_rng(41)
    S = [space["r0"] + 0.1 * space["r1"]] + [0.05 * rng.standard_normal(len(space["ci"])) for _ in range(3)]
    c.kron_compute([(rng.standard_normal((2, 2)) + (4.0 * np.eye(2) if k == 0 else 0.0), S[k]) for k in range(4)])
    per = max(4 * len(space["ci"]), 2 * ND) // (2 * ND)
    assert 1 <= per < 14
    B = rng.standard_normal((2 * ND, 14))
    X, info = c.kron_solve(B, method=capi.SOLVER_DENSE)
    assert info.method_used == capi.SOLVER_DENSE and info.converged == 1
    for j in range(14):
        xj, ij = c.kron_solve(B[:, j], method=capi.SOLVER_DENSE)
        assert ij.method_used == capi.SOLVER_DENSE and np.array_equal(xj, X[:, j])
    inplace = np.asfortranarray(B.copy())
    c.kron_solve_inplace(inplace, method=capi.SOLVER_DENSE)
    assert np.array_equal(inplace, X)
    c.close()


# ---- (c) the open method from the Krylov stage to the dense inverse ---------------------------------------------------------------------------
def _crossing(capi, c, solve, b):
    """the parts of the rent-or-buy rule that no clock decides, as test_open_method_hands_over_to_the_dense_inverse reads them off info.method_used: never
    the inverse within the first `dense_after` (2) columns of a matrix -- one column per call, so the count must be 0, then 1 --; with dense_after = 0 the next
    call builds the inverse, and it stays for calls of two columns under the default again"""
    seen = []
    for _ in range(2):
        x0, info = solve(b)
        seen.append(info.method_used)
    c.tune("dense_after", 0)
    x1, info = solve(b)
    seen.append(info.method_used)
    c.tune("dense_after", 2)
    for _ in range(2):
        x2, info = solve(np.column_stack([b, b]))
        seen.append(info.method_used)
        assert np.array_equal(x2[:, 0], x1) and np.array_equal(x2[:, 1], x1)
    assert seen == [capi.SOLVER_GMRES, capi.SOLVER_GMRES, capi.SOLVER_DENSE, capi.SOLVER_DENSE, capi.SOLVER_DENSE]
    assert np.linalg.norm(x0 - x1) <= 1e-6 * np.linalg.norm(x1)


def test_block_open_method_crosses_to_the_dense_inverse(env, space):
    capi, _ = env
    c, b = _block(env, space)
    _crossing(capi, c, c.block_solve, b)
    c.close()


def test_kron_open_method_crosses_to_the_dense_inverse(env, space):
    capi, _ = env
    c, b = _kron(env, space)
    _crossing(capi, c, c.kron_solve, b)
    c.close()
