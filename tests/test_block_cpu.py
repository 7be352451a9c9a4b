"""The 2 x 2 block handle without a device: the reference side of tests/test_gpu_block.py is checked here, and the entry points are there.
  * the Krylov cases of the GPU test (tests/block_ref.py KRYLOV_CASES), rebuilt from the ORACLE's matrices: scipy's GMRES(50) with the 2 x 2 block-Jacobi
    preconditioner converges to rtol 1e-10 in at most HALF of the budget the GPU test hands over (1 000 iterations) -- the budget is a cap with a factor 2
    to spare, not a measurement of the code under test -- and agrees with SuperLU;
  * the library exports the entry points, and a host-only context answers FDAPDE_ENODEVICE."""
import os

import numpy as np
import pytest

import block_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_system(o, mesh_loader, name, order, lam, advection):
    m = mesh_loader(name)
    dofs, _, nd, _ = o.enumerate_dofs(m, order)
    op = -o.laplacian()
    if advection:
        op = op + o.advection([4.0, -2.0] if m.N == 2 else [4.0, -2.0, 1.0])
    R1 = o.assemble_operator(m, order, dofs, nd, op)
    R0 = o.assemble_operator(m, order, dofs, nd, o.reaction(1.0))
    assert np.array_equal(R1.rowptr, R0.rowptr) and np.array_equal(R1.colidx, R0.colidx)
    obs = br.observed_nodes(m.n_nodes)
    blocks = br.smoothing_blocks(R1.rowptr, R1.colidx, R1.values, R0.values, obs, lam, nd)
    return br.bmat(R1.rowptr, R1.colidx, blocks, nd), br.smoothing_rhs(obs, lam, nd), nd


@pytest.mark.parametrize("name,order,lam,advection", br.KRYLOV_CASES)
def test_reference_gmres_stays_under_half_of_the_cap(oracle, mesh_loader, name, order, lam, advection):
    import scipy.sparse.linalg as spl

    A, b, nd = oracle_system(oracle, mesh_loader, name, order, lam, advection)
    assert abs(A - A.T).max() <= 1e-15 * abs(A).max(), "the smoothing system is symmetric, with or without advection in R1"
    Dinv = br.block_jacobi(A, nd)
    x, iters, info = br.reference_gmres(A, Dinv, b)
    x_lu = spl.splu(A.tocsc()).solve(b)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    print(f"{name} P{order} lambda {lam:g} advection {advection}: 2n = {2 * nd}, GMRES(50) iterations {iters}, error against LU {err:.2e}, "
          f"scaled residual {br.scaled_residual(A, Dinv, b, x):.2e}")
    assert info == 0
    assert 2 * iters <= br.MAXIT_CAP
    assert br.scaled_residual(A, Dinv, b, x) <= 10 * br.RTOL
    assert err <= 1e-6


def test_block_entry_points_exist_and_need_a_device():
    from fdapde_loader import load_package

    capi = load_package().capi
    lib = capi.load()
    for name in ("fdapde_block_compute", "fdapde_block_solve", "fdapde_block_spmv", "fdapde_gram_pointwise"):
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    from fdapde_core_amd import workloads

    nodes, cells, bnd = workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16"))
    c = capi.Context(device=None)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    s = c.sizes()
    v = np.ones(s["nnz"])
    for call in (lambda: c.block_compute(v, v, v, v), lambda: c.block_solve(np.ones(2 * nd)), lambda: c.block_spmv(np.ones(2 * nd)),
                 lambda: c.gram_pointwise(np.zeros(4, dtype=np.int32), np.ones((4, s["n_basis"])))):
        with pytest.raises(capi.FdapdeError) as e:
            call()
        assert e.value.status == capi.ENODEVICE
    c.close()
