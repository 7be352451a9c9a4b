"""Kronecker-sum operators on the FEM pattern (csrc/kernels_kron.h, eng_kron.hip): fdapde_kron_compute / _solve / _spmv against scipy -- sp.kron of the
factors (what the reference's Kronecker(A, B) evaluates to: fdaPDE/linear_algebra/kronecker_product.h:56-80), SuperLU standing in for Eigen::SparseLU, the
2 x 2 block handle as a second yardstick.  The reference side is tests/kron_ref.py; tests/test_kron_cpu.py checks, without a device, that the reference
GMRES stays under half of the iteration budget handed over here."""
import ctypes as C
import os

import numpy as np
import pytest

import block_ref as br
import kron_ref as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
FIXTURES = [("unit_square_16", 1), ("c_shaped", 2), ("unit_sphere", 1)]


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, workloads

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, workloads


_spaces = {}


def _space(env, name, order):
    """one context with assembled R1 = stiff(-laplacian) and R0 = mass per (fixture, order), shared by the tests (each computes its own handle)"""
    key = (name, order)
    if key not in _spaces:
        capi, workloads = env
        nodes, cells, bnd = workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", name))
        c = capi.Context(0)
        c.mesh_upload(nodes, cells, bnd)
        nd = c.dofs_build(order)
        c.set_operator(-capi.laplacian())
        c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
        c.init()
        rp, ci = c.pattern_get()
        _spaces[key] = dict(c=c, nd=nd, rp=rp, ci=ci, r1=c.matrix_values(capi.MAT_STIFF), r0=c.matrix_values(capi.MAT_MASS), obs=br.observed_nodes(nodes.shape[0]))
    return _spaces[key]


def sp_obs(env, name, order):
    return _space(env, name, order)["obs"]


def _fresh(env, name="unit_square_16", order=1):
    capi, workloads = env
    c = capi.Context(0)
    c.mesh_upload(*workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", name)))
    nd = c.dofs_build(order)
    return c, nd


def _product_bound(A, x, n_s, max_len, q):
    """row by row: y in extended precision and 2 k eps (|A| |x|)_i, k = n_S (max row length + q) + 2 additions feeding one output"""
    y_ref, mag = kr.matvec_ld(A, x)
    k = n_s * (max_len + q) + 2
    return y_ref, 2 * k * np.longdouble(EPS) * mag


# ---- 1. the product against the explicit matrix ---------------------------------------------------------------------------------------------------
def _random_terms(rng, q, n_terms, nnz, banded):
    """n_terms terms; with three or more, the last shares the spatial factor (the same array) of the first"""
    S = [rng.standard_normal(nnz) for _ in range(n_terms)]
    if n_terms >= 3:
        S[-1] = S[0]
    terms = []
    for k in range(n_terms):
        T = rng.standard_normal((q, q))
        if banded:
            T = np.triu(np.tril(T, 1), -1)   # tridiagonal, exact zeros outside
        terms.append((T, S[k]))
    return terms, n_terms - (1 if n_terms >= 3 else 0)


@pytest.mark.parametrize("name,order", FIXTURES)
@pytest.mark.parametrize("banded", [False, True])
@pytest.mark.parametrize("n_terms", [1, 3, 4])
@pytest.mark.parametrize("q", [1, 2, 3, 5, 10, 16, 33, 64])
def test_kron_product_against_the_explicit_matrix(env, name, order, q, n_terms, banded):
    """every q, K in {1, 3, 4} (with three or more terms two share an S pointer), dense random and tridiagonal T, on every fixture: per row
    |y - y_ref| <= 2 k eps (|A| |x|) against the product of the explicit matrix in np.longdouble, and the same bits from a second call.  The heaviest
    references are the dense T at q = 64 (q^2 nnz = 32 M entries on unit_sphere, 41 M on c_shaped P2: about 7 s of scipy each)"""
    sp_ = _space(env, name, order)
    c, nd, rp, ci = sp_["c"], sp_["nd"], sp_["rp"], sp_["ci"]
    max_len = int(np.diff(rp).max())
    if name == "unit_square_16":
        assert nd == 289   # (an odd row count: the last workgroup of every team width is partly empty)
    rng = np.random.default_rng(1000 * q + 10 * n_terms + int(banded))
    x = rng.standard_normal(q * nd)
    terms, n_s = _random_terms(rng, q, n_terms, len(ci), banded)
    c.kron_compute(terms)
    A = kr.explicit(terms, rp, ci, nd)
    y = c.kron_spmv(x)
    y_ref, bound = _product_bound(A, x, n_s, max_len, q)
    err = np.abs(y.astype(np.longdouble) - y_ref)
    worst = float(np.max(err / np.maximum(bound, np.longdouble(1e-300))))
    print(f"{name} P{order} q {q} K {n_terms} ({n_s} factors) {'tridiagonal' if banded else 'dense'} T: worst |y - y_ref| / bound = {worst:.4f}")
    assert np.all(err <= bound)
    assert np.array_equal(c.kron_spmv(x), y)


def test_kron_product_zero_rows_of_t_and_q1_edge(env):
    """a T with an all-zero row (nothing to sum there: exact zeros come back) and q = 1, which runs as a team of two with one idle lane: A = t S"""
    sp_ = _space(env, "unit_square_16", 1)
    c, nd, rp, ci = sp_["c"], sp_["nd"], sp_["rp"], sp_["ci"]
    rng = np.random.default_rng(7)
    T = rng.standard_normal((4, 4))
    T[2, :] = 0.0
    S = rng.standard_normal(len(ci))
    c.kron_compute([(T, S)])
    x = rng.standard_normal(4 * nd)
    y = c.kron_spmv(x)
    assert np.all(y[2 * nd:3 * nd] == 0.0) and np.count_nonzero(y[:nd]) == nd
    c.kron_compute([(np.array([[2.0]]), S)])
    x1 = rng.standard_normal(nd)
    y1 = c.kron_spmv(x1)
    y_ref, mag = kr.matvec_ld(br.on_pattern(rp, ci, 2.0 * S, nd), x1)
    assert np.all(np.abs(y1 - y_ref) <= 2 * (int(np.diff(rp).max()) + 3) * EPS * mag)


# ---- 2. the 2 x 2 handle as yardstick -------------------------------------------------------------------------------------------------------------
def _unit(r, c_):
    T = np.zeros((2, 2))
    T[r, c_] = 1.0
    return T


@pytest.mark.parametrize("name,order", FIXTURES)
def test_kron_q2_agrees_with_the_block_handle_product(env, name, order):
    sp_ = _space(env, name, order)
    c, nd, rp, ci = sp_["c"], sp_["nd"], sp_["rp"], sp_["ci"]
    rng = np.random.default_rng(21)
    blocks = [rng.standard_normal(len(ci)) for _ in range(4)]
    x = rng.standard_normal(2 * nd)
    c.block_compute(*blocks)
    c.kron_compute([(_unit(q // 2, q % 2), blocks[q]) for q in range(4)])
    yb, yk = c.block_spmv(x), c.kron_spmv(x)
    A = br.bmat(rp, ci, blocks, nd)
    y_ref, bound = _product_bound(A, x, 4, int(np.diff(rp).max()), 2)
    assert np.all(np.abs(yk - y_ref) <= bound) and np.all(np.abs(yb - y_ref) <= bound)
    print(f"{name} P{order}: worst |kron - block| / bound = {float(np.max(np.abs(yk.astype(np.longdouble) - yb) / np.maximum(bound, np.longdouble(1e-300)))):.4f}")
    assert np.all(np.abs(yk.astype(np.longdouble) - yb) <= bound)   # ... and with each other within the same bound


def test_kron_q2_solve_agrees_with_the_block_handle(env):
    """KRYLOV_CASES[0] through both handles with GMRES by name: scaled residuals <= 10 RTOL each, the solutions within 1e-6 of each other"""
    capi, _ = env
    name, order, lam, advection = br.KRYLOV_CASES[0]
    assert not advection
    sp_ = _space(env, name, order)
    c, nd, rp, ci = sp_["c"], sp_["nd"], sp_["rp"], sp_["ci"]
    blocks = br.smoothing_blocks(rp, ci, sp_["r1"], sp_["r0"], sp_["obs"], lam, nd)
    A = br.bmat(rp, ci, blocks, nd)
    b = br.smoothing_rhs(sp_["obs"], lam, nd)
    c.block_compute(*blocks, symmetric=True)
    c.kron_compute([(_unit(q // 2, q % 2), blocks[q]) for q in range(4)], symmetric=True)
    xb, ib = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=br.RTOL, maxit=br.MAXIT_CAP)
    xk, ik = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
    Dinv = kr.block_jacobi_q(A, nd, 2)
    rb, rk = kr.scaled_residual_ld(A, Dinv, b, xb), kr.scaled_residual_ld(A, Dinv, b, xk)
    print(f"block handle: {ib.iters} iterations, residual {rb:.2e}; Kronecker handle: {ik.iters} iterations, residual {rk:.2e}; "
          f"difference {np.linalg.norm(xk - xb) / np.linalg.norm(xb):.2e}")
    assert ib.converged == 1 and ik.converged == 1 and ik.method_used == capi.SOLVER_GMRES
    assert rb <= 10 * br.RTOL and rk <= 10 * kr.RTOL
    assert np.linalg.norm(xk - xb) <= 1e-6 * np.linalg.norm(xb)


# ---- 3. the diagonal inverse ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", kr.PIVOTING_QS)
def test_kron_diagonal_blocks_that_need_pivoting(env, q):
    """kron_ref.pivoting_terms: the leading entry of D_i is exactly zero at every unobserved DOF.  GMRES by name succeeds (so no block was flagged), the
    scaled residual recomputed in np.longdouble with numpy's own inverses of the D_i is <= 10 RTOL, and the solution agrees with SuperLU to 1e-6"""
    import scipy.sparse.linalg as spl

    capi, _ = env
    sp_ = _space(env, "unit_square_16", 1)
    c, nd, rp, ci = sp_["c"], sp_["nd"], sp_["rp"], sp_["ci"]
    rng = np.random.default_rng(300 + q)
    terms = kr.pivoting_terms(rp, ci, sp_["obs"], q, seed=q)
    A = kr.explicit(terms, rp, ci, nd)
    if q > 1:
        D = kr.diag_blocks(A, nd, q)
        unobserved = np.setdiff1d(np.arange(nd), sp_["obs"])
        assert np.all(D[unobserved, 0, 0] == 0.0) and len(unobserved) > 100
    b = rng.standard_normal(q * nd)
    c.kron_compute(terms)
    x, info = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
    res = kr.scaled_residual_ld(A, kr.block_jacobi_q(A, nd, q), b, x)
    x_lu = spl.splu(A.tocsc()).solve(b)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    print(f"q {q}: {info.iters} iterations, relres {info.relres:.2e}, recomputed {res:.2e}, error against LU {err:.2e}")
    assert info.converged == 1 and info.method_used == capi.SOLVER_GMRES and info.relres <= kr.RTOL
    assert res <= 10 * kr.RTOL
    assert err <= 1e-6


@pytest.mark.parametrize("q", [3, 33])
def test_kron_one_singular_diagonal_block(env, q):
    """S[i, i] = 0 in the only factor at ONE DOF: D_i = 0 -- GMRES by name answers FDAPDE_ENOCONV with the block handle's message, the open method goes
    to the dense stage where q n <= dense_rows (q = 3) and is refused where it is not (q = 33)"""
    import scipy.sparse.linalg as spl

    capi, _ = env
    sp_ = _space(env, "unit_square_16", 1)
    nd, rp, ci = sp_["nd"], sp_["rp"], sp_["ci"]
    c, _ = _fresh(env)
    rng = np.random.default_rng(q)
    S = sp_["r0"] + 0.1 * sp_["r1"]
    i = 7
    S[rp[i] + np.searchsorted(ci[rp[i]:rp[i + 1]], i)] = 0.0
    T = rng.standard_normal((q, q)) + 4.0 * np.eye(q)
    c.kron_compute([(T, S)])
    b = rng.standard_normal(q * nd)
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(b, method=capi.SOLVER_GMRES)
    assert e.value.status == capi.ENOCONV and "diagonal block is singular" in str(e.value)
    if q * nd <= 8192:
        x, info = c.kron_solve(b)
        assert info.method_used == capi.SOLVER_DENSE
        x_lu = spl.splu(kr.explicit([(T, S)], rp, ci, nd).tocsc()).solve(b)
        assert np.linalg.norm(x - x_lu) <= 1e-7 * np.linalg.norm(x_lu)
    else:
        with pytest.raises(capi.FdapdeError) as e:
            c.kron_solve(b)
        assert e.value.status == capi.EUNSUPPORTED
    c.close()


# ---- 4. the space-time smoothing system -----------------------------------------------------------------------------------------------------------
_systems = {}


def _spacetime(env, name, order, m, lam):
    """-> (context with the handle computed, A, b, n_dofs, q, D^-1, LU solution); one factorisation per case, shared by the tests"""
    import scipy.sparse.linalg as spl

    key = (name, order, m, lam)
    sp_ = _space(env, name, order)
    c, nd, rp, ci = sp_["c"], sp_["nd"], sp_["rp"], sp_["ci"]
    terms = kr.spacetime_terms(rp, ci, sp_["r1"], sp_["r0"], sp_["obs"], lam, lam, m)
    if key not in _systems:
        A = kr.explicit(terms, rp, ci, nd)
        b = kr.spacetime_rhs(sp_["obs"], lam, nd, m)
        _systems[key] = (A, b, kr.block_jacobi_q(A, nd, 2 * m), spl.splu(A.tocsc()).solve(b))
    c.kron_compute(terms, symmetric=True)   # (the context is shared: its handle may hold another test's matrix)
    A, b, Dinv, x_lu = _systems[key]
    return c, A, b, nd, 2 * m, Dinv, x_lu


@pytest.mark.parametrize("name,order,m,lam", kr.SOLVE_CASES)
def test_kron_gmres_by_name_on_the_spacetime_system(env, name, order, m, lam):
    """FDAPDE_SOLVER_GMRES, rtol 1e-10, at most 1 000 iterations (a cap: tests/test_kron_cpu.py holds the reference under half of it): converged, the scaled
    residual recomputed in np.longdouble <= 10 RTOL, the error against SuperLU <= 1e-6; in place equals out of place bit for bit"""
    capi, _ = env
    c, A, b, nd, q, Dinv, x_lu = _spacetime(env, name, order, m, lam)
    assert q * nd == {("unit_square_16", 5): 2890, ("unit_sphere", 4): 4696, ("c_shaped", 3): 5670}[(name, m)]
    x, info = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
    res = kr.scaled_residual_ld(A, Dinv, b, x)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    print(f"{name} P{order} m {m} lambda {lam:g}: iterations {info.iters}, relres {info.relres:.2e}, recomputed {res:.2e}, error against LU {err:.2e}")
    assert info.converged == 1 and info.method_used == capi.SOLVER_GMRES
    assert 0 < info.iters <= kr.MAXIT_CAP and 0 < info.relres <= kr.RTOL
    assert res <= 10 * kr.RTOL
    assert err <= 1e-6
    inplace = np.asfortranarray(b.reshape(-1, 1).copy())
    c.kron_solve_inplace(inplace, method=capi.SOLVER_GMRES, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
    assert np.array_equal(inplace[:, 0], x)


@pytest.mark.parametrize("name,order,m,lam", kr.SOLVE_CASES)
def test_kron_dense_by_name_on_the_spacetime_system(env, name, order, m, lam):
    """FDAPDE_SOLVER_DENSE: the bar tests/test_gpu_block.py applies to the block handle's dense stage -- residual <= 1e-9 |b|, solution <= 1e-7 |ref|"""
    capi, _ = env
    c, A, b, nd, q, Dinv, x_lu = _spacetime(env, name, order, m, lam)
    x, info = c.kron_solve(b, method=capi.SOLVER_DENSE)
    print(f"{name} P{order} m {m} lambda {lam:g}: residual {np.linalg.norm(A @ x - b) / np.linalg.norm(b):.2e}, error {np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu):.2e}")
    assert info.method_used == capi.SOLVER_DENSE and info.converged == 1 and np.isfinite(info.relres) and info.iters in (0, 1)
    assert np.linalg.norm(A @ x - b) <= 1e-9 * np.linalg.norm(b)
    assert np.linalg.norm(x - x_lu) <= 1e-7 * np.linalg.norm(x_lu)
    inplace = np.asfortranarray(b.reshape(-1, 1).copy())
    c.kron_solve_inplace(inplace, method=capi.SOLVER_DENSE)
    assert np.array_equal(inplace[:, 0], x)


@pytest.mark.parametrize("name,order,m,lam", kr.SOLVE_CASES)
def test_kron_open_method_with_three_columns(env, name, order, m, lam):
    """AUTO with three columns: a fresh matrix's first call is served by GMRES (never the inverse within the first `dense_after` = 2 calls' columns ... the
    rule counts columns: 3 > 2, but no Krylov time has been spent yet), every column meets the GMRES bars, and equals its one-column solve bit for bit"""
    capi, _ = env
    c, A, b, nd, q, Dinv, x_lu = _spacetime(env, name, order, m, lam)
    B = np.column_stack([b, kr.spacetime_rhs(sp_obs(env, name, order), lam, nd, m, seed=2), kr.spacetime_rhs(sp_obs(env, name, order), lam, nd, m, seed=3)])
    X, info = c.kron_solve(B, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
    assert info.method_used == capi.SOLVER_GMRES and info.converged == 1 and 0 < info.relres <= kr.RTOL
    import scipy.sparse.linalg as spl

    lu = spl.splu(A.tocsc())
    iters = 0
    for j in range(3):
        assert kr.scaled_residual_ld(A, Dinv, B[:, j], X[:, j]) <= 10 * kr.RTOL
        ref = lu.solve(B[:, j])
        assert np.linalg.norm(X[:, j] - ref) <= 1e-6 * np.linalg.norm(ref)
        xj, ij = c.kron_solve(B[:, j], method=capi.SOLVER_GMRES, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
        assert np.array_equal(xj, X[:, j])
        iters += ij.iters
    assert info.iters == iters   # summed over the columns


def test_kron_open_method_hands_over_to_the_dense_inverse(env):
    """rent or buy on q n rows, the parts of the rule that no clock decides: never the inverse within the first `dense_after` (2) columns of a matrix; with
    `dense_after` = 0 the inverse at once, and it stays"""
    capi, _ = env
    c, A, b, nd, q, Dinv, x_lu = _spacetime(env, *kr.SOLVE_CASES[1])
    seen = []
    for _ in range(2):
        x, info = c.kron_solve(b)
        seen.append(info.method_used)
        assert info.converged == 1 and np.linalg.norm(x - x_lu) <= 1e-6 * np.linalg.norm(x_lu)
    c.tune("dense_after", 0)
    try:
        for _ in range(2):
            x, info = c.kron_solve(b)
            seen.append(info.method_used)
            assert info.converged == 1 and np.linalg.norm(x - x_lu) <= 1e-6 * np.linalg.norm(x_lu)
    finally:
        c.tune("dense_after", 2)
    x, info = c.kron_solve(b)
    seen.append(info.method_used)
    print("stages:", seen)
    assert seen == [capi.SOLVER_GMRES, capi.SOLVER_GMRES, capi.SOLVER_DENSE, capi.SOLVER_DENSE, capi.SOLVER_DENSE]


def test_kron_exhausted_budget_leaves_the_last_iterate(env):
    capi, _ = env
    c, A, b, nd, q, Dinv, x_lu = _spacetime(env, *kr.SOLVE_CASES[0])
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(b, method=capi.SOLVER_GMRES, maxit=20)
    assert e.value.status == capi.ENOCONV
    x, info = c.kron_solve(b, method=capi.SOLVER_GMRES, maxit=20, raise_on_noconv=False)
    res = kr.scaled_residual_ld(A, Dinv, b, x)
    assert info.converged == 0 and info.iters == 20 and info.method_used == capi.SOLVER_GMRES
    assert 1e-10 < res < 1.0 and abs(res - info.relres) <= 1e-6 * res


# ---- 5. errors and lifetime -----------------------------------------------------------------------------------------------------------------------
def test_kron_arguments_and_call_order(env):
    capi, _ = env
    c, nd = _fresh(env)
    nnz = c.sizes()["nnz"]
    v = np.random.default_rng(0).standard_normal(nnz)
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(np.ones(2 * nd))
    assert e.value.status == capi.ENOTINIT
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_spmv(np.ones(2 * nd))
    assert e.value.status == capi.ENOTINIT
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_bench_spmv(1)
    assert e.value.status == capi.ENOTINIT
    dp = C.POINTER(C.c_double)
    t65 = np.asfortranarray(np.eye(65))
    one_t, one_s = (dp * 1)(t65.ctypes.data_as(dp)), (dp * 1)(v.ctypes.data_as(dp))
    assert c.lib.fdapde_kron_compute(c._ctx, 0, 1, one_t, one_s, 0) == capi.EINVAL    # q = 0
    assert c.lib.fdapde_kron_compute(c._ctx, 65, 1, one_t, one_s, 0) == capi.EINVAL   # q = 65
    assert c.lib.fdapde_kron_compute(c._ctx, 2, 0, one_t, one_s, 0) == capi.EINVAL    # n_terms = 0
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_compute([(np.eye(2), v)] * 9)                                         # n_terms = 9
    assert e.value.status == capi.EINVAL
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_compute([(np.eye(65), v)])
    assert e.value.status == capi.EINVAL
    for terms in ([(np.eye(2), v), (np.eye(2), None)], [(np.eye(2), v), (None, v)]):   # a NULL factor
        with pytest.raises(capi.FdapdeError) as e:
            c.kron_compute(terms)
        assert e.value.status == capi.EINVAL
    assert c.lib.fdapde_kron_compute(c._ctx, 2, 1, None, one_s, 0) == capi.EINVAL
    with pytest.raises(capi.FdapdeError) as e:   # none of the refused calls left a handle behind
        c.kron_spmv(np.ones(2 * nd))
    assert e.value.status == capi.ENOTINIT
    c.kron_compute([(np.eye(2) * 3.0, v)])
    for method in (capi.SOLVER_CG, capi.SOLVER_BICGSTAB, capi.SOLVER_CG_SR, capi.SOLVER_CG_FUSED, capi.SOLVER_PMG, capi.SOLVER_AMG, capi.SOLVER_BLOCK_AMG):
        with pytest.raises(capi.FdapdeError) as e:
            c.kron_solve(np.ones(2 * nd), method=method)
        assert e.value.status == capi.EUNSUPPORTED
    k = c.clone()   # the clone does not carry the handle, as it does not carry the block handle
    with pytest.raises(capi.FdapdeError) as e:
        k.kron_solve(np.ones(2 * nd))
    assert e.value.status == capi.ENOTINIT
    k.close()
    c.dofs_build(1)   # a new space drops the handle
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_spmv(np.ones(2 * nd))
    assert e.value.status == capi.ENOTINIT
    c.close()


def test_kron_dinv_budget(env):
    """q = 64 on 289 DOFs: D^-1 takes 9.5 MB; with kron_dinv_mb = 1 it is not built -- GMRES by name is refused with a message, the product still runs, DENSE
    by name is refused above the dense limit; back at the default budget GMRES runs"""
    capi, _ = env
    sp_ = _space(env, "unit_square_16", 1)
    c, nd = _fresh(env)
    rng = np.random.default_rng(9)
    q = 64
    T = 0.1 * rng.standard_normal((q, q)) + 2.0 * np.eye(q)
    terms = [(T, sp_["r0"]), (0.01 * np.eye(q), sp_["r1"])]
    b = rng.standard_normal(q * nd)
    c.tune("kron_dinv_mb", 1)
    c.kron_compute(terms)
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(b, method=capi.SOLVER_GMRES)
    assert e.value.status == capi.EUNSUPPORTED and "kron_dinv_mb" in str(e.value)
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(b)
    assert e.value.status == capi.EUNSUPPORTED
    A = kr.explicit(terms, sp_["rp"], sp_["ci"], nd)
    y_ref, bound = _product_bound(A, b, 2, int(np.diff(sp_["rp"]).max()), q)
    assert np.all(np.abs(c.kron_spmv(b) - y_ref) <= bound)
    ms, by = c.kron_bench_spmv(2)
    assert ms > 0 and by == 8 * 2 * len(sp_["ci"]) + 4 * len(sp_["ci"]) + 4 * (nd + 1) + 16 * q * nd
    c.tune("kron_dinv_mb", 2048)
    c.kron_compute(terms)
    x, info = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
    assert info.converged == 1 and kr.scaled_residual_ld(A, kr.block_jacobi_q(A, nd, q), b, x) <= 10 * kr.RTOL
    ms, by = c.kron_bench_spmv(2)
    assert by == 8 * 2 * len(sp_["ci"]) + 4 * len(sp_["ci"]) + 4 * (nd + 1) + 16 * q * nd + 8 * q * q * nd
    c.close()


def test_kron_fused_and_separate_preconditioner_give_the_same_bits(env):
    """knob kron_fuse: D^-1 in the operator kernel's epilogue or as a launch of its own -- the same sums in the same order"""
    capi, _ = env
    c, A, b, nd, q, Dinv, x_lu = _spacetime(env, *kr.SOLVE_CASES[1])
    x1, i1 = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
    c.tune("kron_fuse", 0)
    try:
        x0, i0 = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=kr.RTOL, maxit=kr.MAXIT_CAP)
    finally:
        c.tune("kron_fuse", 1)
    assert np.array_equal(x0, x1) and i0.iters == i1.iters


def test_kron_second_compute_replaces_the_first(env):
    sp_ = _space(env, "unit_square_16", 1)
    c, nd, rp, ci = sp_["c"], sp_["nd"], sp_["rp"], sp_["ci"]
    rng = np.random.default_rng(12)
    S = rng.standard_normal(len(ci))
    x5, x2 = rng.standard_normal(5 * nd), rng.standard_normal(2 * nd)
    c.kron_compute([(rng.standard_normal((5, 5)), S)])
    y5 = c.kron_spmv(x5)
    T2 = rng.standard_normal((2, 2))
    c.kron_compute([(T2, S), (np.eye(2), sp_["r0"])])
    y2 = c.kron_spmv(x2)
    y_ref, bound = _product_bound(kr.explicit([(T2, S), (np.eye(2), sp_["r0"])], rp, ci, nd), x2, 2, int(np.diff(rp).max()), 2)
    assert y2.shape == (2 * nd,) and y5.shape == (5 * nd,) and np.all(np.abs(y2 - y_ref) <= bound)


def test_kron_other_solves_of_the_context_keep_their_bits(env):
    """the n x n handle, the 2 x 2 block handle and fdapde_solve before and after Kronecker calls"""
    capi, _ = env
    c, nd = _fresh(env)
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    rng = np.random.default_rng(2)
    rhs = rng.standard_normal((nd, 3))
    rp, ci = c.pattern_get()
    obs = br.observed_nodes(289)
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    blocks = br.smoothing_blocks(rp, ci, r1, r0, obs, 1e-4, nd)
    bb = br.smoothing_rhs(obs, 1e-4, nd)
    c.block_compute(*blocks, symmetric=True)

    def others():
        c.lin_compute(capi.MAT_STIFF)
        X, _ = c.lin_solve(rhs, rtol=1e-12)
        c.solve(rtol=1e-12)
        xg, _ = c.block_solve(bb, method=capi.SOLVER_GMRES)
        xd, _ = c.block_solve(bb, method=capi.SOLVER_DENSE)
        return X, c.solution(), xg, xd, c.block_spmv(bb)

    before = others()
    m = 3
    terms = kr.spacetime_terms(rp, ci, r1, r0, obs, 1e-4, 1e-4, m)
    b = kr.spacetime_rhs(obs, 1e-4, nd, m)
    c.kron_compute(terms, symmetric=True)
    xk, _ = c.kron_solve(b, method=capi.SOLVER_GMRES)
    c.kron_solve(b, method=capi.SOLVER_DENSE)
    c.kron_spmv(b)
    after = others()
    for u, w in zip(before, after):
        assert np.array_equal(u, w)
    xk2, _ = c.kron_solve(b, method=capi.SOLVER_GMRES)   # ... and the Kronecker handle kept its own through theirs
    assert np.array_equal(xk, xk2)
    c.close()


def test_kron_multi_device_context_is_refused(env):
    capi, _ = env
    c = capi.Context(devices=[0, 0])
    v = np.ones(8)
    dp = v.ctypes.data_as(C.POINTER(C.c_double))
    pp = (C.POINTER(C.c_double) * 1)(dp)
    assert c.lib.fdapde_kron_compute(c._ctx, 2, 1, pp, pp, 0) == capi.EUNSUPPORTED
    assert c.lib.fdapde_kron_solve(c._ctx, None, dp, 1, dp, None) == capi.EUNSUPPORTED
    assert c.lib.fdapde_kron_spmv(c._ctx, dp, dp) == capi.EUNSUPPORTED
    assert c.lib.fdapde_kron_bench_spmv(c._ctx, 1, None, None) == capi.EUNSUPPORTED
    c.close()
