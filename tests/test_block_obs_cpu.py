"""The factored data term of the 2 x 2 block handle without a device: the reference side of tests/test_gpu_block_obs.py is checked here, and the entry points
are there.
  * the seven Krylov cases of the GPU test (tests/block_obs_ref.py KRYLOV_CASES: areal Psi over tiles of the bounding box, or quasi_circle's golden incidence
    matrix), rebuilt from the ORACLE's matrices with scale Psi^T Psi added explicitly: scipy's GMRES(50) with the 2 x 2 block-Jacobi preconditioner converges to
    rtol 1e-10 in at most HALF of the budget the GPU test hands over (1 000 iterations) -- a cap with a factor 2 to spare, not a measurement of the code under
    test -- and agrees with SuperLU to 1e-6;
  * Psi^T Psi of those cases is off the FEM pattern (what fdapde_block_compute cannot take);
  * the library exports both entry points, and a host-only context answers FDAPDE_ENODEVICE."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import block_obs_ref as bo
import block_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,order,lam,regions", bo.KRYLOV_CASES)
def test_reference_gmres_stays_under_half_of_the_cap(oracle, mesh_loader, name, order, lam, regions):
    import scipy.sparse.linalg as spl

    A, b, nd, Psi, (rp, ci, _) = bo.oracle_case(oracle, mesh_loader, name, order, lam, regions)
    assert abs(A - A.T).max() <= 1e-15 * abs(A).max()
    pattern = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(nd, nd))
    gram = (Psi.T @ Psi).tocsr()
    off = gram.nnz - gram.multiply(pattern).nnz
    assert off > 0, "Psi^T Psi has entries off the FEM pattern"
    Dinv = br.block_jacobi(A, nd)
    x, iters, info = br.reference_gmres(A, Dinv, b)
    x_lu = spl.splu(A.tocsc()).solve(b)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    print(f"{name} P{order} lambda {lam:g}: {Psi.shape[0]} regions, 2n = {2 * nd}, longest Psi row {np.diff(Psi.indptr).max()}, pattern nnz {len(ci)}, "
          f"nnz of Psi^T Psi {gram.nnz} ({off} off the pattern), GMRES(50) iterations {iters}, error against LU {err:.2e}")
    assert info == 0
    assert 2 * iters <= bo.MAXIT_CAP
    assert err <= 1e-6


def test_obs_entry_points_exist_and_need_a_device():
    from fdapde_loader import load_package

    capi = load_package().capi
    lib = capi.load()
    for name in ("fdapde_block_set_obs", "fdapde_block_obs_info"):
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    from fdapde_core_amd import workloads

    nodes, cells, bnd = workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16"))
    c = capi.Context(device=None)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    for call in (lambda: c.block_set_obs(sp.identity(nd, format="csr")), lambda: c.block_obs_info()):
        with pytest.raises(capi.FdapdeError) as e:
            call()
        assert e.value.status == capi.ENODEVICE
    c.close()
