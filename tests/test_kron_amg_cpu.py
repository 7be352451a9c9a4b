"""FDAPDE_SOLVER_KRON_AMG without a device: the reference side of tests/test_gpu_kron_amg.py is checked here.
  * every capped case of the GPU test, rebuilt from the ORACLE's matrices: the numpy restatement of the scheme (tests/kron_amg_ref.py) converges to rtol
    1e-10 in at most HALF of the budget the GPU test hands over -- a budget is a cap with a factor 2 to spare, not a measurement of the code under test --
    and ends within 1e-6 of SuperLU;
  * the ladder rule of the GPU test (every count <= 40, the largest mesh's <= 1.5 x the smallest's + 2) holds for the restatement on the same inputs;
  * a system under the coarse limit is one exact level;
  * the new id, the new exports, and what a host-only context answers."""
import os

import numpy as np
import pytest

import block_ref as br
import kron_amg_ref as ka
import kron_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache, _spaces = {}, {}


def _space(oracle, mesh_loader, mesh, order):
    """-> (rowptr, colidx, R1, R0, n_dofs, observed nodes), once per (mesh, order)"""
    key = (mesh, order)
    if key not in _spaces:
        if isinstance(mesh, str):
            m = mesh_loader(mesh)
        else:
            from fdapde_loader import load_package

            load_package()
            from fdapde_core_amd import meshgen

            nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
            m = oracle.Mesh(np.ascontiguousarray(nodes, dtype=float), np.ascontiguousarray(cells, dtype=np.int32), np.ascontiguousarray(bnd, dtype=np.uint8))
        dofs, _, nd, _ = oracle.enumerate_dofs(m, order)
        R1 = oracle.assemble_operator(m, order, dofs, nd, -oracle.laplacian())
        R0 = oracle.assemble_operator(m, order, dofs, nd, oracle.reaction(1.0))
        assert np.array_equal(R1.rowptr, R0.rowptr) and np.array_equal(R1.colidx, R0.colidx)
        _spaces[key] = (R1.rowptr, R1.colidx, R1.values, R0.values, nd, br.observed_nodes(m.n_nodes))
    return _spaces[key]


def restated(oracle, mesh_loader, case, term=-1):
    """-> (iterations, converged, error against SuperLU, rows per level, relative residual), once per case"""
    import scipy.sparse.linalg as spl

    if (case, term) not in _cache:
        rp, ci, R1, R0, nd, obs = _space(oracle, mesh_loader, case[1], case[2])
        terms, q, b = ka.system(case, rp, ci, R1, R0, obs)
        A = kr.explicit(terms, rp, ci, nd)
        x, it, ok, rows = ka.solve(rp, ci, terms, nd, b, term=term)
        x_lu = spl.splu(A.tocsc()).solve(b)
        _cache[(case, term)] = (it, ok, np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu), rows, np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    return _cache[(case, term)]


CAPPED = list(dict.fromkeys(ka.SPACETIME_CASES + ka.PARABOLIC_CASES + ka.WIDTH_CASES))


@pytest.mark.parametrize("case", CAPPED, ids=[ka.case_id(c) for c in CAPPED])
def test_restatement_stays_under_half_of_the_budget(oracle, mesh_loader, case):
    it, ok, err, rows, res = restated(oracle, mesh_loader, case)
    print(f"{ka.case_id(case)}: rows per level {rows}, iterations {it} (budget {ka.budget(case)}), |b - A x| / |b| = {res:.2e}, error against LU {err:.2e}")
    assert ok and res <= ka.RTOL
    assert 2 * it <= ka.budget(case)
    assert err <= 1e-6


def test_naming_the_stiffness_factor_is_no_worse_on_c_shaped_p2(oracle, mesh_loader):
    """knob kron_amg_term: term 3 of the space-time system is lambda M_t (x) R1"""
    case = ka.SPACETIME_CASES[3]
    assert case[1] == "c_shaped"
    it, ok, err, rows, res = restated(oracle, mesh_loader, case, term=3)
    print(f"{ka.case_id(case)} on the stiffness factor: rows per level {rows}, iterations {it}")
    assert ok and res <= ka.RTOL and err <= 1e-6 and 2 * it <= ka.budget(case)


@pytest.mark.parametrize("ladder", ka.LADDERS, ids=[c[0][1][0] for c in ka.LADDERS])
def test_restatement_satisfies_the_ladder_rule(oracle, mesh_loader, ladder):
    counts = []
    for case in ladder:
        it, ok, err, rows, _ = restated(oracle, mesh_loader, case)
        assert ok and err <= 1e-6
        counts.append(it)
    print(f"{ladder[0][1][0]}: iterations {counts}")
    assert max(counts) <= ka.LADDER_CAP
    assert counts[-1] <= 1.5 * counts[0] + 2


def test_a_system_under_the_coarse_limit_is_one_exact_level(oracle, mesh_loader):
    import scipy.sparse.linalg as spl

    rp, ci, R1, R0, nd, obs = _space(oracle, mesh_loader, "unit_square_16", 1)
    terms, q, b = ka.system(("parabolic", "unit_square_16", 1, 3, 0.01), rp, ci, R1, R0, obs)
    x, it, ok, rows = ka.solve(rp, ci, terms, nd, b, coarse_rows=1024)
    x_lu = spl.splu(kr.explicit(terms, rp, ci, nd).tocsc()).solve(b)
    assert rows == [3 * nd] and ok and it <= 2
    assert np.linalg.norm(x - x_lu) <= 1e-7 * np.linalg.norm(x_lu)


def test_new_method_its_entry_points_and_a_host_only_context():
    from fdapde_loader import load_package

    capi = load_package().capi
    assert capi.SOLVER_KRON_AMG == 10
    assert "fdapde_kron_amg_hierarchy" in capi.SYMBOLS and "fdapde_kron_amg_aggregates" in capi.SYMBOLS
    lib = capi.load()
    for s in capi.SYMBOLS:
        assert hasattr(lib, s), s
    from fdapde_core_amd import workloads

    nodes, cells, bnd = workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16"))
    c = capi.Context(device=None)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(np.ones(2 * nd), method=capi.SOLVER_KRON_AMG)
    assert e.value.status == capi.ENODEVICE
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_amg_hierarchy()
    assert e.value.status == capi.ENOTINIT
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_amg_aggregates(0)
    assert e.value.status == capi.ENOTINIT
    c.close()
