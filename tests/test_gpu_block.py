"""2 x 2 block systems on the FEM pattern (csrc/kernels_block.h, eng_block.hip): fdapde_block_compute / _solve / _spmv and fdapde_gram_pointwise against
scipy -- sp.bmat of the four blocks, SuperLU (standing in for Eigen::SparseLU on a SparseBlockMatrix<double,2,2>: fdaPDE/linear_algebra/
sparse_block_matrix.h:29-128, utils/symbols.h:133-160), numpy for the Psi products.  The reference side is tests/block_ref.py; tests/test_block_cpu.py
checks, without a device, that the reference GMRES stays under half of the iteration budget handed over here."""
import ctypes as C
import os

import numpy as np
import pytest

import block_ref as br
import segment_ref as sg
import surface_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, workloads

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, workloads


def _mesh(workloads, name):
    from oracle import oracle as o

    if name == "network":
        o.build()
        return sg.load_network_fixture(ROOT)
    if name == "surface":
        o.build()
        m = sr.load_surface_fixture(ROOT)
        return np.ascontiguousarray(m.nodes), np.ascontiguousarray(m.cells, dtype=np.int32), np.ascontiguousarray(m.boundary)
    if name == "one_triangle":
        return np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), np.array([[0, 1, 2]], dtype=np.int32), np.ones(3, dtype=np.uint8)
    return workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", name))


def _space(env, name, order):
    capi, workloads = env
    nodes, cells, bnd = _mesh(workloads, name)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(order)
    return c, nd, nodes, cells


# ---- 1. operator parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", [("network", 1), ("unit_square_16", 1), ("c_shaped", 2), ("unit_sphere", 1), ("unit_sphere", 2), ("surface", 1),
                                        ("one_triangle", 1)])
def test_block_product_against_scipy(env, name, order):
    """y = A x for random values on the pattern in all four blocks, then with each block in turn absent: per row |y - y_ref| <= (2 len + 1) eps (|A| |x|)
    -- the bound of a sum of 2 len products in any order, for the two sums compared -- and the same bits from a second call"""
    c, nd, _, _ = _space(env, name, order)
    rp, ci = c.pattern_get()
    nnz = len(ci)
    rng = np.random.default_rng(11)
    full = [rng.standard_normal(nnz) for _ in range(4)]
    x = rng.standard_normal(2 * nd)
    length = np.diff(rp)
    if name == "unit_sphere":
        assert length.max() > 8, "rows longer than one pass of a team of 8 lanes"
    bound_len = np.concatenate([length, length])
    for absent in (None, 0, 1, 2, 3):
        blocks = [None if q == absent else full[q] for q in range(4)]
        c.block_compute(*blocks)
        A = br.bmat(rp, ci, blocks, nd)
        y = c.block_spmv(x)
        y_ref = A @ x
        scale = abs(A) @ np.abs(x)
        worst = np.max(np.abs(y - y_ref) / np.maximum((2 * bound_len + 1) * EPS * scale, 1e-300))
        print(f"{name} P{order} absent block {absent}: worst |y - y_ref| / bound = {worst:.3f}")
        assert np.all(np.abs(y - y_ref) <= (2 * bound_len + 1) * EPS * scale)
        assert np.array_equal(c.block_spmv(x), y)
    c.close()


# ---- 2. Psi^T W Psi -------------------------------------------------------------------------------------------------------------------------------
def _gram_reference(rp, ci, nd, dofs, cells, vals, w):
    """per pattern entry: the sum in extended precision, the sum of the absolute terms, the number of locations contributing"""
    import scipy.sparse as sp

    slot_of = sp.csr_matrix((np.arange(len(ci)) + 1, ci, rp), shape=(nd, nd))
    ok = cells >= 0
    d = dofs[cells[ok]]
    v = vals[ok].astype(np.longdouble)
    wl = (np.ones(ok.sum()) if w is None else w[ok]).astype(np.longdouble)
    terms = wl[:, None, None] * v[:, :, None] * v[:, None, :]
    rows, cols = np.repeat(d[:, :, None], d.shape[1], axis=2).reshape(-1), np.repeat(d[:, None, :], d.shape[1], axis=1).reshape(-1)
    slots = np.asarray(slot_of[rows, cols]).reshape(-1) - 1
    assert slots.min() >= 0
    total, mag, k = np.zeros(len(ci), dtype=np.longdouble), np.zeros(len(ci), dtype=np.longdouble), np.zeros(len(ci))
    np.add.at(total, slots, terms.reshape(-1))
    np.add.at(mag, slots, np.abs(terms.reshape(-1)))
    np.add.at(k, slots, 1.0)
    return total, mag, k


def _check_gram(c, nd, cells, vals, weights):
    rp, ci = c.pattern_get()
    dofs, _, _ = c.dofs_get()
    got = c.gram_pointwise(cells, vals, weights)
    total, mag, k = _gram_reference(rp, ci, nd, dofs, cells, vals, weights)
    err = np.abs(got.astype(np.longdouble) - total)
    bound = k * EPS * mag
    print(f"gram: {int((cells >= 0).sum())} of {len(cells)} locations inside, up to {int(k.max())} per entry, worst error / bound = "
          f"{float(np.max(err / np.maximum(bound, np.longdouble(1e-300)))):.3f}")
    assert np.all(err <= bound)
    assert np.all(got[k == 0] == 0.0)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("weighted", [False, True])
def test_gram_matrix_on_c_shaped(env, order, weighted):
    """the fixture's locations plus 2 000 random points of its bounding box (some outside: rows with cell id -1): |error| <= k eps sum |terms| per entry
    (k terms, each a rounded product, added in some order; the reference sum is taken in extended precision)"""
    capi, workloads = env
    c, nd, nodes, _ = _space(env, "c_shaped", order)
    locs = workloads._read_fixture_csv(os.path.join(ROOT, "tests", "golden", "mesh", "c_shaped", "locs.csv"), float)
    rng = np.random.default_rng(3)
    pts = np.concatenate([locs, rng.uniform(nodes.min(axis=0), nodes.max(axis=0), size=(2000, 2))])
    cells, vals = c.eval_pointwise_raw(pts)
    assert (cells < 0).any() and (cells >= 0).sum() > 1000
    _check_gram(c, nd, cells, vals, rng.uniform(0.5, 2.0, len(pts)) if weighted else None)
    c.close()


@pytest.mark.parametrize("weighted", [False, True])
def test_gram_matrix_on_the_surface_through_project(env, weighted):
    c, nd, nodes, cells_m = _space(env, "surface", 1)
    rng = np.random.default_rng(4)
    pts = nodes[cells_m].mean(axis=1) + 0.01 * rng.standard_normal((len(cells_m), 3))
    cells, vals, _, _ = c.project_raw(pts)
    assert (cells >= 0).all()
    _check_gram(c, nd, cells, vals, rng.uniform(0.5, 2.0, len(pts)) if weighted else None)
    c.close()


# ---- 3. / 4. the smoothing system -----------------------------------------------------------------------------------------------------------------
_systems = {}


def _smoothing(env, name, order, lam, advection):
    """-> (context with the block handle computed, A, b, n_dofs, LU solution); one context and one factorisation per case, shared by the tests"""
    import scipy.sparse.linalg as spl

    key = (name, order, lam, advection)
    if key not in _systems:
        capi, _ = env
        c, nd, nodes, _ = _space(env, name, order)
        op = -capi.laplacian()
        if advection:
            op = op + capi.advection([4.0, -2.0] if nodes.shape[1] == 2 else [4.0, -2.0, 1.0])
        c.set_operator(op)
        c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
        c.init()
        rp, ci = c.pattern_get()
        r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
        obs = br.observed_nodes(nodes.shape[0])
        blocks = br.smoothing_blocks(rp, ci, r1, r0, obs, lam, nd)
        A = br.bmat(rp, ci, blocks, nd)
        b = br.smoothing_rhs(obs, lam, nd)
        c.block_compute(*blocks, symmetric=True)
        _systems[key] = (c, A, b, nd, spl.splu(A.tocsc()).solve(b))
    return _systems[key]


@pytest.mark.parametrize("name,order,lam,advection", br.KRYLOV_CASES)
def test_gmres_by_name_on_the_smoothing_system(env, name, order, lam, advection):
    """FDAPDE_SOLVER_GMRES, rtol 1e-10, at most 1 000 iterations (a cap: the reference needs 52 - 185, tests/test_block_cpu.py): converged, relres <= rtol, the
    scaled residual recomputed by numpy <= 10 rtol, and the error against LU within 10 times that of scipy's GMRES(50) with the same preconditioner and
    stop rule (two correct GMRES runs stop at different last iterates)"""
    capi, _ = env
    c, A, b, nd, x_lu = _smoothing(env, name, order, lam, advection)
    if advection:
        assert abs(A - A.T).max() <= 1e-15 * abs(A).max()
    Dinv = br.block_jacobi(A, nd)
    x_ref, it_ref, info_ref = br.reference_gmres(A, Dinv, b)
    assert info_ref == 0
    e_ref = np.linalg.norm(x_ref - x_lu) / np.linalg.norm(x_lu)
    x, info = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=br.RTOL, maxit=br.MAXIT_CAP)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    res = br.scaled_residual(A, Dinv, b, x)
    print(f"{name} P{order} lambda {lam:g} advection {advection}: iterations {info.iters} (scipy {it_ref}), relres {info.relres:.2e}, recomputed {res:.2e}, "
          f"error against LU {err:.2e} (scipy {e_ref:.2e})")
    assert info.converged == 1 and info.method_used == capi.SOLVER_GMRES
    assert info.relres <= br.RTOL
    assert res <= 10 * br.RTOL
    assert err <= 10 * e_ref


@pytest.mark.parametrize("name,order,lam,advection", br.KRYLOV_CASES)
def test_dense_by_name_on_the_smoothing_system(env, name, order, lam, advection):
    """FDAPDE_SOLVER_DENSE: the bounds tests/test_gpu_dense.py uses for indefinite matrices -- residual <= 1e-9 |b|, solution <= 1e-7 |ref|"""
    capi, _ = env
    c, A, b, nd, x_lu = _smoothing(env, name, order, lam, advection)
    x, info = c.block_solve(b, method=capi.SOLVER_DENSE)
    print(f"{name} P{order} lambda {lam:g}: residual {np.linalg.norm(A @ x - b) / np.linalg.norm(b):.2e}, error {np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu):.2e}")
    assert info.method_used == capi.SOLVER_DENSE and info.converged == 1
    assert np.linalg.norm(A @ x - b) <= 1e-9 * np.linalg.norm(b)
    assert np.linalg.norm(x - x_lu) <= 1e-7 * np.linalg.norm(x_lu)


def test_dense_columns_together_one_by_one_and_in_place(env):
    capi, _ = env
    c, A, b, nd, _ = _smoothing(env, "unit_square_16", 1, 1e-4, False)
    rng = np.random.default_rng(5)
    B = rng.standard_normal((2 * nd, 64))
    X, info = c.block_solve(B, method=capi.SOLVER_DENSE)
    assert info.method_used == capi.SOLVER_DENSE
    for j in range(64):
        xj, _ = c.block_solve(B[:, j], method=capi.SOLVER_DENSE)
        assert np.linalg.norm(X[:, j] - xj) <= 1e-12 * np.linalg.norm(xj)
    inplace = np.asfortranarray(B.copy())
    c.block_solve_inplace(inplace, method=capi.SOLVER_DENSE)
    assert np.array_equal(inplace, X)
    one = np.asfortranarray(B[:, :1].copy())   # ... and through the Krylov stage
    c.block_solve_inplace(one, method=capi.SOLVER_GMRES)
    xk, _ = c.block_solve(B[:, 0], method=capi.SOLVER_GMRES)
    assert np.array_equal(one[:, 0], xk)


def test_open_method_hands_over_to_the_dense_inverse(env):
    """rent or buy, as fdapde_lin_solve: never within the first `dense_after` (2) columns, then the inverse once the Krylov columns have cost half of it"""
    capi, _ = env
    c, A, b, nd, x_lu = _smoothing(env, "unit_square_16", 1, 1e-2, False)
    blocks_again = br.smoothing_blocks(*c.pattern_get(), c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS), br.observed_nodes(289), 1e-2, nd)
    c.block_compute(*blocks_again, symmetric=True)   # (a new matrix starts over: the column count and the inverse belong to it)
    seen = []
    for _ in range(8):
        x, info = c.block_solve(b)
        seen.append(info.method_used)
        assert info.converged == 1 and np.linalg.norm(x - x_lu) <= 1e-6 * np.linalg.norm(x_lu)
    print("stages:", seen)
    assert seen[0] == capi.SOLVER_GMRES and seen[1] == capi.SOLVER_GMRES
    assert seen[-1] == capi.SOLVER_DENSE


def test_above_the_dense_limit(env):
    """unit_sphere P2: 2 n = 8 386 > 8 192 -- DENSE by name is refused, the open method solves it with GMRES"""
    capi, _ = env
    c, A, b, nd, x_lu = _smoothing(env, "unit_sphere", 2, 1e-4, False)
    assert 2 * nd == 8386
    with pytest.raises(capi.FdapdeError) as e:
        c.block_solve(b, method=capi.SOLVER_DENSE)
    assert e.value.status == capi.EUNSUPPORTED
    x, info = c.block_solve(b)
    assert info.method_used == capi.SOLVER_GMRES and info.converged == 1 and info.relres <= 1e-10
    assert np.linalg.norm(x - x_lu) <= 1e-6 * np.linalg.norm(x_lu)


# ---- 5. edges -------------------------------------------------------------------------------------------------------------------------------------
def test_call_order_and_arguments(env):
    capi, _ = env
    c, nd, _, _ = _space(env, "unit_square_16", 1)
    nnz = c.sizes()["nnz"]
    v = np.random.default_rng(0).standard_normal(nnz)
    with pytest.raises(capi.FdapdeError) as e:
        c.block_solve(np.ones(2 * nd))
    assert e.value.status == capi.ENOTINIT
    with pytest.raises(capi.FdapdeError) as e:
        c.block_spmv(np.ones(2 * nd))
    assert e.value.status == capi.ENOTINIT
    for blocks in ((None, None, v, v), (v, v, None, None)):
        with pytest.raises(capi.FdapdeError) as e:
            c.block_compute(*blocks)
        assert e.value.status == capi.EINVAL
    c.block_compute(v, None, None, v)
    for method in (capi.SOLVER_CG, capi.SOLVER_BICGSTAB, capi.SOLVER_CG_SR, capi.SOLVER_CG_FUSED, capi.SOLVER_PMG, capi.SOLVER_AMG):
        with pytest.raises(capi.FdapdeError) as e:
            c.block_solve(np.ones(2 * nd), method=method)
        assert e.value.status == capi.EUNSUPPORTED
    k = c.clone()   # the clone does not carry the block handle
    with pytest.raises(capi.FdapdeError) as e:
        k.block_solve(np.ones(2 * nd))
    assert e.value.status == capi.ENOTINIT
    k.close()
    c.close()


def test_singular_diagonal_block(env):
    """a11 = a12 = 0 on the diagonal of one DOF: no block-Jacobi form -- GMRES by name is refused, the open method answers through the dense inverse"""
    import scipy.sparse.linalg as spl

    capi, _ = env
    c, A, b, nd, _ = _smoothing(env, "unit_square_16", 1, 1e-4, False)
    rp, ci = c.pattern_get()
    blocks = [v.copy() for v in br.smoothing_blocks(rp, ci, c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS), br.observed_nodes(289), 1e-4, nd)]
    i = 7
    d = rp[i] + np.searchsorted(ci[rp[i]:rp[i + 1]], i)
    blocks[0][d] = 0.0
    blocks[1][d] = 0.0
    k = capi.Context(0)
    from fdapde_core_amd import workloads

    k.mesh_upload(*workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16")))
    k.dofs_build(1)
    k.block_compute(*blocks)
    with pytest.raises(capi.FdapdeError) as e:
        k.block_solve(b, method=capi.SOLVER_GMRES)
    assert e.value.status == capi.EUNSUPPORTED
    x, info = k.block_solve(b)
    assert info.method_used == capi.SOLVER_DENSE
    x_lu = spl.splu(br.bmat(rp, ci, blocks, nd).tocsc()).solve(b)
    assert np.linalg.norm(x - x_lu) <= 1e-7 * np.linalg.norm(x_lu)
    k.close()


def test_exhausted_budget_leaves_the_last_iterate(env):
    capi, _ = env
    c, A, b, nd, x_lu = _smoothing(env, "unit_square_16", 1, 1e-2, False)
    with pytest.raises(capi.FdapdeError) as e:
        c.block_solve(b, method=capi.SOLVER_GMRES, maxit=20)
    assert e.value.status == capi.ENOCONV
    x, info = c.block_solve(b, method=capi.SOLVER_GMRES, maxit=20, raise_on_noconv=False)
    Dinv = br.block_jacobi(A, nd)
    res = br.scaled_residual(A, Dinv, b, x)
    assert info.converged == 0 and info.iters == 20 and info.method_used == capi.SOLVER_GMRES
    assert 1e-10 < res < 1.0 and abs(res - info.relres) <= 1e-6 * res   # the iterate of 20 steps: better than zero, and the one relres speaks of


def test_other_solves_of_the_context_keep_their_bits(env):
    """the n x n handle and fdapde_solve before and after block calls"""
    capi, _ = env
    c, nd, _, _ = _space(env, "unit_square_16", 1)
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    rng = np.random.default_rng(2)
    rhs = rng.standard_normal((nd, 3))

    def others():
        c.lin_compute(capi.MAT_STIFF)
        X, _ = c.lin_solve(rhs, rtol=1e-12)
        c.solve(rtol=1e-12)
        return X, c.solution()

    X0, u0 = others()
    rp, ci = c.pattern_get()
    blocks = br.smoothing_blocks(rp, ci, c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS), br.observed_nodes(289), 1e-4, nd)
    c.block_compute(*blocks, symmetric=True)
    b = br.smoothing_rhs(br.observed_nodes(289), 1e-4, nd)
    c.block_solve(b, method=capi.SOLVER_GMRES)
    c.block_solve(b, method=capi.SOLVER_DENSE)
    c.block_spmv(b)
    X1, u1 = others()
    assert np.array_equal(X0, X1) and np.array_equal(u0, u1)
    xb, _ = c.block_solve(b, method=capi.SOLVER_GMRES)   # ... and both handles live side by side
    assert np.linalg.norm(br.bmat(rp, ci, blocks, nd) @ xb - b) <= 1e-6 * np.linalg.norm(b)
    c.close()


def test_multi_device_context_is_refused(env):
    capi, _ = env
    c = capi.Context(devices=[0, 0])
    v = np.ones(8)
    dp = v.ctypes.data_as(C.POINTER(C.c_double))
    cells = np.zeros(2, dtype=np.int32)
    assert c.lib.fdapde_block_compute(c._ctx, dp, dp, dp, dp, 0) == capi.EUNSUPPORTED
    assert c.lib.fdapde_block_solve(c._ctx, None, dp, 1, dp, None) == capi.EUNSUPPORTED
    assert c.lib.fdapde_block_spmv(c._ctx, dp, dp) == capi.EUNSUPPORTED
    assert c.lib.fdapde_gram_pointwise(c._ctx, C.c_int64(2), cells.ctypes.data_as(C.POINTER(C.c_int32)), dp, None, dp) == capi.EUNSUPPORTED
    c.close()
