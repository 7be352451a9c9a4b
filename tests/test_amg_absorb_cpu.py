"""The absorption pass of the multilevel set-ups (knob `amg_absorb`) without a device: the reference side of tests/test_gpu_amg_absorb.py is checked here.
  * every capped case of the GPU test, rebuilt from the ORACLE's matrices: the numpy restatement (tests/amg_absorb_ref.py) converges to rtol 1e-10 in at most
    HALF of the cap the GPU test hands over -- a cap is a condition with a factor 2 to spare, not a measurement of the code under test --, ends within 1e-6
    of SuperLU, and every level keeps at most 0.35 of the rows above it;
  * the ladder rule of tests/test_gpu_amg.py (the largest mesh's count <= 1.5 x the smallest's + 2) holds for the restatement on the same inputs;
  * the rule itself, against a row-by-row loop: hosts are paired rows, only rows the matching left single have one, no single with a paired neighbour stays
    alone; without absorption the pass is block_amg_ref.pairwise;
  * the smallest refusal: the block system on unit_cube(16) stalls above 48 rows without absorption and coarsens to <= 32 rows with it;
  * the library exports the query, and a host-only context has no hierarchy to report."""
import numpy as np
import pytest

import amg_absorb_ref as ab
import block_amg_ref as ar
import block_ref as br

_cache = {}


def _mesh(oracle, mesh):
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import meshgen

    nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
    return oracle.Mesh(np.ascontiguousarray(nodes, dtype=float), np.ascontiguousarray(cells, dtype=np.int32), np.ascontiguousarray(bnd, dtype=np.uint8))


def _interior_system(oracle, mesh):
    """P1 -Lap with zero Dirichlet data: the interior block of the oracle's matrix and of its load vector"""
    m = _mesh(oracle, mesh)
    dofs, bnd, nd, _ = oracle.enumerate_dofs(m, 1)
    A = oracle.assemble_operator(m, 1, dofs, nd, -oracle.laplacian()).to_scipy().tocsr()
    qn = oracle.quadrature_nodes(m, 1)
    f = oracle.assemble_forcing(m, 1, dofs, nd, ab.ladder_forcing(qn.shape[0]))
    free = np.flatnonzero(np.asarray(bnd) == 0)
    return A[free][:, free].tocsr(), f[free]


def scalar_restated(oracle, mesh):
    """-> (iterations, converged, error against SuperLU, rows per level, singles per level), once per mesh"""
    import scipy.sparse.linalg as spl

    if mesh not in _cache:
        A, b = _interior_system(oracle, mesh)
        x, it, ok, H = ab.scalar_solve(A, b, True)
        x_lu = spl.splu(A.tocsc()).solve(b)
        _cache[mesh] = (it, ok, np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu), H.rows, H.singles)
    return _cache[mesh]


def _block_system(oracle):
    mesh, order, lam, _ = ab.BLOCK_CASE
    if "block" not in _cache:
        m = _mesh(oracle, mesh)
        dofs, _, nd, _ = oracle.enumerate_dofs(m, order)
        R1 = oracle.assemble_operator(m, order, dofs, nd, -oracle.laplacian())
        R0 = oracle.assemble_operator(m, order, dofs, nd, oracle.reaction(1.0))
        obs = br.observed_nodes(m.n_nodes)
        blocks = br.smoothing_blocks(R1.rowptr, R1.colidx, R1.values, R0.values, obs, lam, nd)
        _cache["block"] = (R1.rowptr, R1.colidx, blocks, nd, br.smoothing_rhs(obs, lam, nd))
    return _cache["block"]


SCALAR = [(m, ab.CAP_3D) for m in ab.LADDER_3D] + [(m, ab.CAP_2D) for m in ab.LADDER_2D]


@pytest.mark.parametrize("mesh,cap", SCALAR, ids=[f"{m[0]}({m[1]})" for m, _ in SCALAR])
def test_scalar_restatement_stays_under_half_of_the_cap(oracle, mesh, cap):
    it, ok, err, rows, singles = scalar_restated(oracle, mesh)
    print(f"{mesh[0]}({mesh[1]}): rows per level {rows}, kept {[round(k, 3) for k in ab.kept(rows)]}, singles before absorption {singles}, "
          f"iterations {it} (cap {cap}), error against LU {err:.2e}")
    assert ok and err <= 1e-6
    assert 2 * it <= cap
    assert len(rows) >= 2 and max(ab.kept(rows)) <= ab.KEEP


@pytest.mark.parametrize("ladder", [ab.LADDER_3D, ab.LADDER_2D], ids=["unit_cube", "unit_square"])
def test_scalar_restatement_satisfies_the_ladder_rule(oracle, ladder):
    counts = [scalar_restated(oracle, mesh)[0] for mesh in ladder]
    print(f"{ladder[0][0]}: iterations {counts}")
    assert counts[-1] <= 1.5 * counts[0] + 2


def test_block_restatement_is_refused_without_absorption_and_stays_under_half_of_the_cap_with_it(oracle):
    import scipy.sparse.linalg as spl

    rp, ci, blocks, nd, b = _block_system(oracle)
    with pytest.raises(ab.Stalled) as e:
        ab.BlockHierarchy(rp, ci, blocks, nd, False, ab.BLOCK_COARSE_ROWS, ab.BLOCK_DENSE_ROWS)
    print(f"without absorption: stalls at 2 n_l = {e.value.rows}")
    assert e.value.rows >= 64, "a margin over dense_rows 48: the device numbers the rows differently"
    x, it, ok, rows = ab.block_solve(rp, ci, blocks, nd, b, True, ab.BLOCK_COARSE_ROWS, ab.BLOCK_DENSE_ROWS)
    A = br.bmat(rp, ci, blocks, nd)
    x_lu = spl.splu(A.tocsc()).solve(b)
    err, res = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu), np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print(f"with absorption: rows per level {rows}, iterations {it} (cap {ab.CAP_BLOCK}), |b - A x| / |b| = {res:.2e}, error against LU {err:.2e}")
    assert ok and res <= ar.RTOL and err <= 1e-6
    assert 2 * it <= ab.CAP_BLOCK
    assert rows[-1] <= ab.BLOCK_COARSE_ROWS and max(ab.kept(rows)) <= ab.KEEP


def test_the_rule_row_by_row(oracle):
    """on the pair graph of unit_cube(8)'s interior (where the matching leaves singles): the vectorised rule against a loop over the rows"""
    A, _ = _interior_system(oracle, ("unit_cube", 8))
    A.sort_indices()
    n = A.shape[0]
    rp, ci, a = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data
    agg1, n1, _ = ab.pairwise(rp, ci, a, n, True)
    rp1, ci1, v1 = ar.galerkin(rp, ci, [a], agg1, n1, n)
    for rp_, ci_, a_, n_ in ((rp, ci, a, n), (rp1, ci1, v1[0], n1)):
        mate, sw, rows, h = ab.matching(rp_, ci_, a_, n_)
        host = ab.absorb(ci_, sw, rows, h, mate)
        for i in range(n_):
            best = (-1, 0.0, 0)
            for k in range(rp_[i], rp_[i + 1]):
                j, w = ci_[k], abs(sw[k])
                if mate[i] >= 0 or not w > 0.0 or j == i or mate[j] < 0:
                    continue
                if w > best[1] or (w == best[1] and (h[k] > best[2] or (h[k] == best[2] and j < best[0]))):
                    best = (j, w, h[k])
            assert host[i] == best[0], i
        assert np.all(mate[host[host >= 0]] >= 0), "hosts are paired rows: no chains"
        agg, nc, singles = ab.pairwise(rp_, ci_, a_, n_, True)
        plain, nc_plain = ar.pairwise(rp_, ci_, a_, n_)
        agg0, nc0, _ = ab.pairwise(rp_, ci_, a_, n_, False)
        assert np.array_equal(agg0, plain) and nc0 == nc_plain, "without absorption the pass is the one of block_amg_ref"
        assert nc == nc_plain - int((host >= 0).sum()) and agg.min() == 0 and agg.max() == nc - 1 and len(np.unique(agg)) == nc
        i = np.flatnonzero(host >= 0)
        assert np.array_equal(agg[i], agg[host[i]]) and np.array_equal(agg[host[i]], agg[mate[host[i]]])
        print(f"{n_} rows: {singles} left single, {len(i)} of them absorbed, {nc_plain} -> {nc} aggregates")
    assert singles > 0 and len(i) > 0, "the case exercises the pass"


def test_the_query_is_exported_and_a_host_only_context_has_no_hierarchy():
    from fdapde_loader import load_package

    capi = load_package().capi
    assert "fdapde_amg_hierarchy" in capi.SYMBOLS and hasattr(capi.load(), "fdapde_amg_hierarchy")
    assert capi.load().fdapde_abi_version() == 5, "the query is an addition: the ABI version stays"
    c = capi.Context(device=None)
    for which in (0, 1, 2):
        with pytest.raises(capi.FdapdeError) as e:
            c.amg_hierarchy(which)
        assert e.value.status == capi.ENOTINIT
    with pytest.raises(capi.FdapdeError) as e:
        c.amg_hierarchy(3)
    assert e.value.status == capi.EINVAL
    # ... and fdapde_amg_aggregates / fdapde_amg_damping / fdapde_amg_order likewise: no hierarchy of any kind is live, no fourth kind
    for symbol in ("fdapde_amg_aggregates", "fdapde_amg_damping", "fdapde_amg_order"):
        assert symbol in capi.SYMBOLS and hasattr(capi.load(), symbol)
    for which, status in ((2, capi.ENOTINIT), (0, capi.ENOTINIT), (1, capi.ENOTINIT), (3, capi.EINVAL)):
        for call in (lambda: c.amg_aggregates(which, 0), lambda: c.amg_damping(which), lambda: c.amg_order(which)):
            with pytest.raises(capi.FdapdeError) as e:
                call()
            assert e.value.status == status, which
    c.close()
