"""The factored data term of the Kronecker-sum handle without a device: the reference side of tests/test_gpu_kron_obs.py is checked here.
  * the Krylov cases of the GPU test (tests/kron_obs_ref.py SOLVE_CASES), rebuilt from the ORACLE's matrices: scipy's GMRES(50) with the q x q point-block
    Jacobi preconditioner of the FULL matrix converges to rtol 1e-10 in at most HALF of the budget the GPU test hands over (1 000 iterations) -- the budget
    is a cap with a factor 2 to spare, not a measurement of the code under test -- and agrees with SuperLU (the bars of tests/test_kron_cpu.py);
  * the explicit term against a dense numpy Kronecker product, Phi = NULL against an explicit [I_p 0], the hat functions;
  * the library exports both entry points, and a host-only context answers FDAPDE_ENODEVICE."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import kron_obs_ref as ko
import kron_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,order,m,p,lam,lam_t,design,miss", ko.SOLVE_CASES)
def test_reference_gmres_stays_under_half_of_the_cap(oracle, mesh_loader, name, order, m, p, lam, lam_t, design, miss):
    import scipy.sparse.linalg as spl

    A, b, nd, Psi, Phi, W, _ = ko.oracle_case(oracle, mesh_loader, name, order, m, p, lam, lam_t, design, miss)
    q = 2 * m
    assert A.shape == (q * nd, q * nd) and Phi.shape == (p, q) and W.shape == (p, Psi.shape[0])
    assert abs(A - A.T).max() <= 1e-13 * abs(A).max(), "the space-time smoothing system is symmetric"
    if miss > 0:
        assert 0.15 < 1.0 - W.mean() < 0.45, "about `miss` of the observations are missing"
    if name == "c_shaped":
        assert (np.diff(Psi.indptr) == 0).any(), "locations outside the mesh give empty rows"
    if name == "unit_sphere":
        assert np.diff(Psi.indptr).max() == 113
    Dinv = kr.block_jacobi_q(A, nd, q)
    x, iters, info = kr.reference_gmres(A, Dinv, b)
    x_lu = spl.splu(A.tocsc()).solve(b)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    res = kr.scaled_residual_ld(A, Dinv, b, x)
    print(f"{name} P{order} m {m} p {p} lambda {lam:g} lambda_T {lam_t:g} {design} miss {miss}: q n = {q * nd}, Psi {Psi.shape[0]} x {nd} with rows up to "
          f"{np.diff(Psi.indptr).max()}, GMRES(50) iterations {iters}, error against LU {err:.2e}, scaled residual {res:.2e}")
    assert info == 0
    assert 2 * iters <= ko.MAXIT_CAP
    assert res <= 10 * ko.RTOL
    assert err <= 1e-6


def test_explicit_term_against_a_dense_kronecker_product():
    rng = np.random.default_rng(0)
    n, q, p, n_obs = 6, 3, 2, 4
    psi = rng.standard_normal((n_obs, n)) * (rng.uniform(size=(n_obs, n)) < 0.5)
    psi[2] = 0.0   # an empty row
    Phi = rng.standard_normal((p, q))
    W = rng.uniform(size=(p, n_obs)) * (rng.uniform(size=(p, n_obs)) < 0.7)
    B = np.kron(Phi, psi)
    ref = 0.37 * B.T @ np.diag(W.reshape(-1)) @ B
    got = ko.term(Phi, sp.csr_matrix(psi), W, 0.37).toarray()
    assert np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max()
    # entry (r n + i, s n + j) = scale sum_tau Phi[tau, r] Phi[tau, s] sum_k w[tau, k] Psi[k, i] Psi[k, j]
    r, i, s, j = 1, 4, 2, 0
    entry = 0.37 * sum(Phi[t, r] * Phi[t, s] * sum(W[t, k] * psi[k, i] * psi[k, j] for k in range(n_obs)) for t in range(p))
    assert np.isclose(got[r * n + i, s * n + j], entry, rtol=1e-12, atol=1e-15)
    # the diagonal block of DOF i is Phi^T diag(g_i) Phi, g_i[tau] = scale sum_k w[tau, k] Psi[k, i]^2
    g = 0.37 * np.array([sum(W[t, k] * psi[k, 3] ** 2 for k in range(n_obs)) for t in range(p)])
    assert np.allclose(got[3::n, 3::n], Phi.T @ np.diag(g) @ Phi, rtol=1e-12, atol=1e-15)
    # the product reference applies the factors: the same vector
    x = rng.standard_normal(q * n)
    y, mag = ko.product_reference(sp.csr_matrix((q * n, q * n)), n, Phi, sp.csr_matrix(psi), W, 0.37, x)
    assert np.allclose(y.astype(float), ref @ x, rtol=1e-12, atol=1e-14) and np.all(mag.astype(float) >= np.abs(ref @ x) * (1 - 1e-12))


def test_pattern_product_without_the_explicit_matrix():
    """pattern_product_ld (what the GPU test uses at q = 64) against kron_ref.matvec_ld on the explicit matrix: the same y, and |A| |x| to rounding"""
    rng = np.random.default_rng(3)
    n, q = 7, 4
    dense = rng.standard_normal((n, n)) * (rng.uniform(size=(n, n)) < 0.5)
    np.fill_diagonal(dense, 1.0)
    S = sp.csr_matrix(dense)
    S.sort_indices()
    v2 = rng.standard_normal(S.nnz)
    terms = [(rng.standard_normal((q, q)), S.data), (rng.standard_normal((q, q)), v2), (rng.standard_normal((q, q)), S.data)]
    x = rng.standard_normal(q * n)
    y, mag = ko.pattern_product_ld(terms, S.indptr, S.indices, n, x)
    y_ref, mag_ref = kr.matvec_ld(kr.explicit(terms, S.indptr, S.indices, n), x)
    assert np.all(np.abs(y - y_ref) <= 1e-15 * mag_ref) and np.all(np.abs(mag - mag_ref) <= 1e-14 * mag_ref)


def test_null_phi_is_the_leading_identity():
    rng = np.random.default_rng(1)
    n, q, p = 5, 4, 3
    Psi = sp.random(7, n, density=0.5, random_state=2, format="csr")
    W = rng.uniform(size=(p, 7))
    Phi = ko.identity_phi(p, q)
    assert np.array_equal(Phi, np.hstack([np.eye(p), np.zeros((p, q - p))]))
    T = ko.term(Phi, Psi, W, -1.0).toarray()
    for r in range(q):
        for s in range(q):
            blk = T[r * n:(r + 1) * n, s * n:(s + 1) * n]
            if r == s and r < p:
                assert np.allclose(blk, -(Psi.T @ sp.diags(W[r]) @ Psi).toarray(), rtol=1e-13, atol=1e-15)
            else:
                assert not blk.any()


@pytest.mark.parametrize("m", [1, 2, 5])
def test_hat_functions(m):
    t = np.sort(np.random.default_rng(m).uniform(0, 1, 9))
    H = ko.hats(m, t)
    assert H.shape == (9, m) and np.allclose(H.sum(axis=1), 1.0) and (H >= 0).all() and ((H > 0).sum(axis=1) <= 2).all()
    if m > 1:
        assert np.allclose(H @ np.linspace(0, 1, m), t)   # P1 reproduces linear functions
        assert np.array_equal(ko.hats(m, np.linspace(0, 1, m)), np.eye(m))


def test_kron_obs_entry_points_exist_and_need_a_device():
    from fdapde_loader import load_package

    capi = load_package().capi
    lib = capi.load()
    for name in ("fdapde_kron_set_obs", "fdapde_kron_obs_info"):
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    from fdapde_core_amd import workloads

    nodes, cells, bnd = workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16"))
    c = capi.Context(device=None)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    Psi = sp.identity(nd, format="csr")
    for call in (lambda: c.kron_set_obs(Psi, Phi=np.eye(2, 3)), lambda: c.kron_set_obs(None), lambda: c.kron_obs_info()):
        with pytest.raises(capi.FdapdeError) as e:
            call()
        assert e.value.status == capi.ENODEVICE
    c.close()
