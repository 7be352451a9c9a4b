"""The Kronecker-sum handle without a device: the reference side of tests/test_gpu_kron.py is checked here, and the entry points are there.
  * the solve cases of the GPU test (tests/kron_ref.py SOLVE_CASES), rebuilt from the ORACLE's matrices: scipy's GMRES(50) with the q x q point-block
    Jacobi preconditioner converges to rtol 1e-10 in at most HALF of the budget the GPU test hands over (1 000 iterations) -- the budget is a cap with a
    factor 2 to spare, not a measurement of the code under test -- and agrees with SuperLU;
  * explicit() against a dense numpy Kronecker product, and the time matrices' properties;
  * the library exports the entry points, and a host-only context answers FDAPDE_ENODEVICE."""
import os

import numpy as np
import pytest

import block_ref as br
import kron_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_system(o, mesh_loader, name, order, m, lam):
    mesh = mesh_loader(name)
    dofs, _, nd, _ = o.enumerate_dofs(mesh, order)
    R1 = o.assemble_operator(mesh, order, dofs, nd, -o.laplacian())
    R0 = o.assemble_operator(mesh, order, dofs, nd, o.reaction(1.0))
    assert np.array_equal(R1.rowptr, R0.rowptr) and np.array_equal(R1.colidx, R0.colidx)
    obs = br.observed_nodes(mesh.n_nodes)
    terms = kr.spacetime_terms(R1.rowptr, R1.colidx, R1.values, R0.values, obs, lam, lam, m)
    return kr.explicit(terms, R1.rowptr, R1.colidx, nd), kr.spacetime_rhs(obs, lam, nd, m), nd


@pytest.mark.parametrize("name,order,m,lam", kr.SOLVE_CASES)
def test_reference_gmres_stays_under_half_of_the_cap(oracle, mesh_loader, name, order, m, lam):
    import scipy.sparse.linalg as spl

    A, b, nd = oracle_system(oracle, mesh_loader, name, order, m, lam)
    q = 2 * m
    assert A.shape == (q * nd, q * nd)
    assert abs(A - A.T).max() <= 1e-15 * abs(A).max(), "the space-time smoothing system is symmetric"
    Dinv = kr.block_jacobi_q(A, nd, q)
    x, iters, info = kr.reference_gmres(A, Dinv, b)
    x_lu = spl.splu(A.tocsc()).solve(b)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    res = kr.scaled_residual_ld(A, Dinv, b, x)
    print(f"{name} P{order} m {m} lambda {lam:g}: q n = {q * nd}, GMRES(50) iterations {iters}, error against LU {err:.2e}, scaled residual {res:.2e}, "
          f"cond(D_i) up to {np.linalg.cond(kr.diag_blocks(A, nd, q)).max():.1e}")
    assert info == 0
    assert 2 * iters <= kr.MAXIT_CAP
    assert res <= 10 * kr.RTOL
    assert err <= 1e-6


def test_explicit_against_a_dense_kronecker_product():
    rng = np.random.default_rng(0)
    n, q = 6, 3
    dense = rng.standard_normal((n, n)) * (rng.uniform(size=(n, n)) < 0.5)
    np.fill_diagonal(dense, 1.0)
    import scipy.sparse as sp

    S = sp.csr_matrix(dense)
    S.sort_indices()
    T = [rng.standard_normal((q, q)) for _ in range(2)]
    T[1][0, 2] = 0.0
    v2 = rng.standard_normal(S.nnz)
    A = kr.explicit([(T[0], S.data), (T[1], v2)], S.indptr, S.indices, n)
    ref = np.kron(T[0], dense) + np.kron(T[1], br.on_pattern(S.indptr, S.indices, v2, n).toarray())
    assert np.abs(A.toarray() - ref).max() <= 1e-15 * np.abs(ref).max()
    assert np.isclose(A[1 * n + 2, 2 * n + 2], T[0][1, 2] * dense[2, 2] + T[1][1, 2] * br.on_pattern(S.indptr, S.indices, v2, n)[2, 2], rtol=1e-14)   # index r n + i
    D = kr.diag_blocks(A, n, q)
    assert np.allclose(D[4], T[0] * dense[4, 4] + T[1] * br.on_pattern(S.indptr, S.indices, v2, n)[4, 4])
    Dinv = kr.block_jacobi_q(A, n, q)
    P = (Dinv @ A).toarray()
    for i in range(n):
        assert np.allclose(P[i::n, i::n], np.eye(q), atol=1e-10)


@pytest.mark.parametrize("m", [2, 3, 5, 8])
def test_time_matrices(m):
    M, P = kr.time_mass(m), kr.time_penalty(m)
    for T in (M, P):
        assert np.array_equal(T, T.T) and np.all(np.triu(T, 2) == 0.0)
    assert np.linalg.eigvalsh(M).min() > 0
    assert np.linalg.eigvalsh(P).min() > -1e-12 and np.abs(P @ np.ones(m)).max() <= 1e-12
    assert abs(M.sum() - 1.0) <= 1e-14   # the integral of 1 over [0, 1]


def test_kron_entry_points_exist_and_need_a_device():
    from fdapde_loader import load_package

    capi = load_package().capi
    lib = capi.load()
    for name in ("fdapde_kron_compute", "fdapde_kron_solve", "fdapde_kron_spmv", "fdapde_kron_bench_spmv"):
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    from fdapde_core_amd import workloads

    nodes, cells, bnd = workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16"))
    c = capi.Context(device=None)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    v = np.ones(c.sizes()["nnz"])
    for call in (lambda: c.kron_compute([(np.eye(3), v)]), lambda: c.kron_solve(np.ones(3 * nd)), lambda: c.kron_spmv(np.ones(3 * nd)),
                 lambda: c.kron_bench_spmv(1)):
        with pytest.raises(capi.FdapdeError) as e:
            call()
        assert e.value.status == capi.ENODEVICE
    c.close()


@pytest.mark.parametrize("q", kr.PIVOTING_QS)
def test_reference_gmres_on_the_pivoting_cases(oracle, mesh_loader, q):
    """the diagonal-inverse cases of the GPU test: the leading entry of D_i is exactly zero at every unobserved DOF, and the reference converges at once"""
    import scipy.sparse.linalg as spl

    mesh = mesh_loader("unit_square_16")
    dofs, _, nd, _ = oracle.enumerate_dofs(mesh, 1)
    R1 = oracle.assemble_operator(mesh, 1, dofs, nd, -oracle.laplacian())
    obs = br.observed_nodes(mesh.n_nodes)
    A = kr.explicit(kr.pivoting_terms(R1.rowptr, R1.colidx, obs, q, seed=q), R1.rowptr, R1.colidx, nd)
    D = kr.diag_blocks(A, nd, q)
    if q > 1:
        unobserved = np.setdiff1d(np.arange(nd), obs)
        assert len(unobserved) > 100 and np.all(D[unobserved, 0, 0] == 0.0) and np.all(D[obs, 0, 0] == -1.0)
    b = np.random.default_rng(300 + q).standard_normal(q * nd)
    Dinv = kr.block_jacobi_q(A, nd, q)
    x, iters, info = kr.reference_gmres(A, Dinv, b)
    x_lu = spl.splu(A.tocsc()).solve(b)
    print(f"q {q}: GMRES(50) iterations {iters}, cond(D_i) up to {np.linalg.cond(D).max():.1e}")
    assert info == 0 and 2 * iters <= kr.MAXIT_CAP
    assert kr.scaled_residual_ld(A, Dinv, b, x) <= 10 * kr.RTOL
    assert np.linalg.norm(x - x_lu) <= 1e-6 * np.linalg.norm(x_lu)
