"""FDAPDE_SOLVER_BLOCK_AMG without a device: the reference side of tests/test_gpu_block_amg.py is checked here.
  * every capped case of the GPU test, rebuilt from the ORACLE's matrices: the numpy restatement of the scheme (tests/block_amg_ref.py) converges to rtol
    1e-10 in at most HALF of the budget the GPU test hands over -- a budget is a cap with a factor 2 to spare, not a measurement of the code under test --
    and ends within 1e-6 of SuperLU;
  * the ladder rule of the GPU test (every count <= 40, the largest mesh's <= 1.5 x the smallest's + 2) holds for the restatement on the same inputs;
  * the library exports nothing new that needs a device-less answer: a host-only context answers the new id like the other block methods."""
import os

import numpy as np
import pytest

import block_amg_ref as ar
import block_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _mesh(oracle, mesh_loader, mesh):
    if isinstance(mesh, str):
        return mesh_loader(mesh)
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import meshgen

    nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
    return oracle.Mesh(np.ascontiguousarray(nodes, dtype=float), np.ascontiguousarray(cells, dtype=np.int32), np.ascontiguousarray(bnd, dtype=np.uint8))


def restated(oracle, mesh_loader, case):
    """-> (iterations, converged, error against SuperLU, rows per level, relative residual), once per case"""
    import scipy.sparse.linalg as spl

    if case not in _cache:
        mesh, order, lam, advection = case
        m = _mesh(oracle, mesh_loader, mesh)
        dofs, _, nd, _ = oracle.enumerate_dofs(m, order)
        op = -oracle.laplacian()
        if advection:
            op = op + oracle.advection([4.0, -2.0] if m.N == 2 else [4.0, -2.0, 1.0])
        R1 = oracle.assemble_operator(m, order, dofs, nd, op)
        R0 = oracle.assemble_operator(m, order, dofs, nd, oracle.reaction(1.0))
        assert np.array_equal(R1.rowptr, R0.rowptr) and np.array_equal(R1.colidx, R0.colidx)
        obs = br.observed_nodes(m.n_nodes)
        blocks = br.smoothing_blocks(R1.rowptr, R1.colidx, R1.values, R0.values, obs, lam, nd)
        A = br.bmat(R1.rowptr, R1.colidx, blocks, nd)
        b = br.smoothing_rhs(obs, lam, nd)
        x, it, ok, rows = ar.solve(R1.rowptr, R1.colidx, blocks, nd, b)
        x_lu = spl.splu(A.tocsc()).solve(b)
        _cache[case] = (it, ok, np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu), rows, np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    return _cache[case]


CAPPED = [(c, ar.BUDGET_P1) for c in ar.LU_CASES] + [(c, ar.BUDGET_P2_2D) for c in ar.P2_2D_CASES] + [(c, ar.BUDGET_P2_3D) for c in ar.P2_3D_CASES]


@pytest.mark.parametrize("case,budget", CAPPED, ids=[ar.case_id(c) for c, _ in CAPPED])
def test_restatement_stays_under_half_of_the_budget(oracle, mesh_loader, case, budget):
    it, ok, err, rows, res = restated(oracle, mesh_loader, case)
    print(f"{ar.case_id(case)}: rows per level {rows}, iterations {it} (budget {budget}), |b - A x| / |b| = {res:.2e}, error against LU {err:.2e}")
    assert ok and res <= ar.RTOL
    assert 2 * it <= budget
    assert err <= 1e-6
    if case == (("unit_square", 32), 1, 1e-4, False):
        assert len(rows) >= 3, "the smallest system with an inner GCR step"


@pytest.mark.parametrize("meshes,lam", ar.LADDERS, ids=[f"{m[0][0]}-{lam:g}" for m, lam in ar.LADDERS])
def test_restatement_satisfies_the_ladder_rule(oracle, mesh_loader, meshes, lam):
    counts = []
    for mesh in meshes:
        it, ok, err, rows, _ = restated(oracle, mesh_loader, (mesh, 1, lam, False))
        assert ok and err <= 1e-6
        counts.append(it)
    print(f"{meshes[0][0]} lambda {lam:g}: iterations {counts}")
    assert max(counts) <= ar.LADDER_CAP
    assert counts[-1] <= 1.5 * counts[0] + 2


def test_a_system_under_the_coarse_limit_is_one_exact_level(oracle, mesh_loader):
    import scipy.sparse.linalg as spl

    m = mesh_loader("unit_square_16")
    dofs, _, nd, _ = oracle.enumerate_dofs(m, 1)
    R1 = oracle.assemble_operator(m, 1, dofs, nd, -oracle.laplacian())
    R0 = oracle.assemble_operator(m, 1, dofs, nd, oracle.reaction(1.0))
    obs = br.observed_nodes(m.n_nodes)
    blocks = br.smoothing_blocks(R1.rowptr, R1.colidx, R1.values, R0.values, obs, 1e-4, nd)
    b = br.smoothing_rhs(obs, 1e-4, nd)
    x, it, ok, rows = ar.solve(R1.rowptr, R1.colidx, blocks, nd, b, coarse_rows=1024)
    x_lu = spl.splu(br.bmat(R1.rowptr, R1.colidx, blocks, nd).tocsc()).solve(b)
    assert rows == [2 * nd] and ok and it <= 2
    assert np.linalg.norm(x - x_lu) <= 1e-7 * np.linalg.norm(x_lu)


def test_new_method_needs_no_new_entry_point_and_needs_a_device():
    from fdapde_loader import load_package

    capi = load_package().capi
    assert capi.SOLVER_BLOCK_AMG == 9
    assert not [s for s in capi.SYMBOLS if "block_amg" in s], "the method goes through fdapde_block_solve: no new export"
    from fdapde_core_amd import workloads

    nodes, cells, bnd = workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16"))
    c = capi.Context(device=None)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    with pytest.raises(capi.FdapdeError) as e:
        c.block_solve(np.ones(2 * nd), method=capi.SOLVER_BLOCK_AMG)
    assert e.value.status == capi.ENODEVICE
    c.close()
