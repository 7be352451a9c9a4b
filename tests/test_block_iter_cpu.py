"""The reference side of tests/test_gpu_block_iterates.py without a device (tests/block_iter_ref.py).

Every case of the GPU test is rebuilt from the ORACLE's matrices, with aggregates from the restatement's passes in the caller's numbering
(block_amg_ref.pairwise / amg_absorb_ref: any valid aggregates serve -- the device hands its own out), and the float64 checkers of the two schemes are
measured against the extended-precision reference in the units of the GPU test's bounds:
  * r_cpu(k), the worst ratio per case and k, is written to profiles/block_iterates.txt;
  * the constants committed in block_iter_ref (c(k) = 4 r_cpu(k) rounded up to a power of two, one set per stage) must still fit, and none exceeds 2^12:
    a relative 1e-6 defect of the cycle moves an iterate by 1e6 .. 1e9 of the unit, three orders above such a bound.
The reference checks itself: at k large enough it agrees with SuperLU to 1e-9, its coarse block values are symmetric in the block sense where the blocks
are, and its cycle agrees with block_amg_ref's float64 cycle on the same aggregates."""
import os

import numpy as np
import pytest

import amg_absorb_ref as ab
import block_iter_ref as ir
import block_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "block_iterates.txt")
_systems, _rows = {}, {}


def _system(oracle, name):
    """-> (rowptr, colidx, blocks, n, smoothing right-hand side, observed nodes) of the system of AMG_CASES[name], from the oracle's matrices"""
    mesh, order, lam, advection = ir.AMG_CASES[name][:4]
    key = (mesh, order, lam, advection)
    if key not in _systems:
        from fdapde_loader import load_package

        load_package()
        from fdapde_core_amd import meshgen

        nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
        m = oracle.Mesh(np.ascontiguousarray(nodes, dtype=float), np.ascontiguousarray(cells, dtype=np.int32), np.ascontiguousarray(bnd, dtype=np.uint8))
        dofs, _, nd, _ = oracle.enumerate_dofs(m, order)
        op = -oracle.laplacian()
        if advection:
            op = op + oracle.advection([4.0, -2.0] if m.N == 2 else [4.0, -2.0, 1.0])
        R1 = oracle.assemble_operator(m, order, dofs, nd, op)
        R0 = oracle.assemble_operator(m, order, dofs, nd, oracle.reaction(1.0))
        assert np.array_equal(R1.rowptr, R0.rowptr) and np.array_equal(R1.colidx, R0.colidx)
        obs = br.observed_nodes(m.n_nodes)
        rp, ci = np.asarray(R1.rowptr, dtype=np.int64), np.asarray(R1.colidx, dtype=np.int64)
        blocks = br.smoothing_blocks(rp, ci, R1.values, R0.values, obs, lam, nd)
        _systems[key] = (rp, ci, blocks, nd, br.smoothing_rhs(obs, lam, nd), obs)
    return _systems[key]


def _aggregates(rp, ci, blocks, n, coarse_rows, absorbing):
    """the restatement's passes, level by level -> (maps row -> row of the next level, the float64 hierarchy they came from)"""
    H = ab.BlockHierarchy(rp, ci, blocks, n, absorbing, coarse_rows)
    return [np.asarray(P.tocsr()[::2].indices // 2, dtype=np.int64) for P in H.P], H


def _hierarchy(oracle, name):
    rp, ci, blocks, n, b, _ = _system(oracle, name)
    knobs = ir.AMG_CASES[name][4]
    aggs, H64 = _aggregates(rp, ci, blocks, n, knobs.get("amg_coarse_rows", ir.AMG_COARSE_ROWS), knobs.get("amg_absorb", 0) == 1)
    return rp, ci, blocks, n, b, aggs, H64


HEADER = ["# k-th iterates of the 2 x 2 block handle's two Krylov stages against the extended-precision reference (tests/block_iter_ref.py): worst ratios per case and k.",
          "# Units: block_amg max |x - x_ref| / (u max s) per field, gmres max_i |x - x_ref|_i / (u s_i); [relres]: |relres - rho_k| / (u || |A| s || / ||b||); u = 2^-53.",
          "# cpu lines: the float64 numpy checkers (also against relres' unit), rewritten by tests/test_block_iter_cpu.py; gpu lines: an MI355X, appended by",
          "# tests/test_gpu_block_iterates.py under FDAPDE_BLOCK_ITER_PROFILE."]
STAGES = ("cpu block_amg ", "cpu gmres ", "cpu gmres_obs ")


def _table(stage, cases, measure, constants):
    ir.constants_table(PROFILE, HEADER, STAGES, stage, cases, measure, constants)


def test_multilevel_constants_fit(oracle):
    def measure(name, K):
        rp, ci, blocks, n, b, aggs, _ = _hierarchy(oracle, name)
        restart = ir.AMG_CASES[name][4].get("gmres_m", 50)
        ref = ir.fgmres_iterates(ir.Hierarchy(rp, ci, blocks, n, aggs), b, K, restart)
        chk = ir.fgmres_float64(rp, ci, blocks, n, aggs, b, K, restart)
        _rows[name] = [len(a) for a in aggs] + [int(aggs[-1].max()) + 1]
        return {it.k: max(ir.field_ratios(c.x.astype(np.float64), it) + [ir.relres_ratio(c.rho, it)]) for it, c in zip(ref, chk)}

    _table("block_amg", [(name, case[5]) for name, case in ir.AMG_CASES.items()], measure, ir.C_AMG)
    print("rows per level:", {k: [2 * r for r in v] for k, v in _rows.items()})
    for name in "abcdef":
        assert len(_rows[name]) >= 3, "cases a .. f have an inner GCR level in the restatement's numbering as well"
    assert len(_rows["g"]) == 2


def test_gmres_constants_fit(oracle):
    def measure(name, K):
        system, knobs, rhs, _ = ir.GMRES_CASES[name]
        rp, ci, blocks, n, b, _ = _system(oracle, system)
        if rhs == "unit":
            b = ir.unit_rhs(n, ir.interior_dof(rp, n))
        restart = knobs.get("gmres_m", 50)
        ref = ir.gmres_iterates(rp, ci, blocks, n, b, K, restart)
        chk = ir.gmres_float64(rp, ci, blocks, n, b, K, restart)
        if rhs == "unit":
            assert all((it.s == 0).any() for it in ref), "dead entries at every k of the unit right-hand side"
        return {it.k: max(ir.entry_ratio(c.x.astype(np.float64), it), ir.relres_ratio(c.rho, it)) for it, c in zip(ref, chk)}

    _table("gmres", [(name, case[3]) for name, case in ir.GMRES_CASES.items()], measure, ir.C_GMRES)


def _obs_system(oracle, name):
    """-> (rowptr, colidx, blocks, n, right-hand side, Psi) of a case of GMRES_OBS_CASES: block_obs_ref's system on the oracle's matrices and Psi"""
    import block_obs_ref as bo
    import kron_obs_ref as ko
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import meshgen

    system, design, _ = ir.GMRES_OBS_CASES[name]
    mesh, order, lam, advection = ir.AMG_CASES[system][:4]
    assert not advection
    nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
    m = oracle.Mesh(np.ascontiguousarray(nodes, dtype=float), np.ascontiguousarray(cells, dtype=np.int32), np.ascontiguousarray(bnd, dtype=np.uint8))
    dofs, _, nd, _ = oracle.enumerate_dofs(m, order)
    R1 = oracle.assemble_operator(m, order, dofs, nd, -oracle.laplacian())
    R0 = oracle.assemble_operator(m, order, dofs, nd, oracle.reaction(1.0))
    Psi = ko.design_psi(oracle, m, None, order, dofs, nd, design)
    rp, ci = np.asarray(R1.rowptr, dtype=np.int64), np.asarray(R1.colidx, dtype=np.int64)
    return rp, ci, bo.smoothing_blocks(rp, ci, R1.values, R0.values, lam, nd), nd, bo.smoothing_rhs(Psi, lam, nd), Psi


def test_gmres_constants_with_a_term_fit(oracle):
    import block_obs_ref as bo
    import scipy.sparse.linalg as spl

    def measure(name, K):
        rp, ci, blocks, n, b, Psi = _obs_system(oracle, name)
        rows = np.diff(Psi.indptr)
        assert (rows.max() > 64) if name == "a-areal" else (rows.max() <= 3), "an areal row is longer than a team of 64; a pointwise row holds one cell's DOFs"
        obs = (Psi, None, -1.0)
        ref = ir.gmres_iterates(rp, ci, blocks, n, b, K, obs=obs)
        chk = ir.gmres_float64(rp, ci, blocks, n, b, K, obs=obs)
        return {it.k: max(ir.entry_ratio(c.x.astype(np.float64), it), ir.relres_ratio(c.rho, it)) for it, c in zip(ref, chk)}

    _table("gmres_obs", [(name, case[2]) for name, case in ir.GMRES_OBS_CASES.items()], measure, ir.C_GMRES_OBS)
    # the reference with a term checks itself: at k large enough it agrees with SuperLU on the explicit system
    rp, ci, blocks, n, b, Psi = _obs_system(oracle, "a-points")
    x_lu = spl.splu(bo.system(rp, ci, blocks, n, Psi).tocsc()).solve(b)
    its = ir.gmres_iterates(rp, ci, blocks, n, b, 300, restart=300, obs=(Psi, None, -1.0))
    err = float(np.abs(its[-1].x - x_lu).max() / np.abs(x_lu).max())
    print(f"GMRES reference with a pointwise term at k = 300: rho {its[-1].rho:.2e}, error against SuperLU {err:.2e}")
    assert err <= 1e-9


@pytest.mark.parametrize("name", ["a", "f", "g"])
def test_reference_converges_to_lu(oracle, name):
    import scipy.sparse.linalg as spl

    rp, ci, blocks, n, b, aggs, _ = _hierarchy(oracle, name)
    x_lu = spl.splu(br.bmat(rp, ci, blocks, n).tocsc()).solve(b)
    its = ir.fgmres_iterates(ir.Hierarchy(rp, ci, blocks, n, aggs), b, 40)
    err = float(np.abs(its[-1].x - x_lu).max() / np.abs(x_lu).max())
    print(f"{name}: multilevel reference at k = 40: rho {its[-1].rho:.2e}, error against SuperLU {err:.2e}")
    assert err <= 1e-9
    rhos = [it.rho for it in its]
    assert all(b_ <= a_ * (1 + 1e-12) for a_, b_ in zip(rhos, rhos[1:]) if a_ > 1e-15), "a minimal-residual iteration: the residual does not grow"


def test_gmres_reference_converges_to_lu(oracle):
    import scipy.sparse.linalg as spl

    rp, ci, blocks, n, b, _ = _system(oracle, "a")
    x_lu = spl.splu(br.bmat(rp, ci, blocks, n).tocsc()).solve(b)
    its = ir.gmres_iterates(rp, ci, blocks, n, b, 400, restart=400)
    err = float(np.abs(its[-1].x - x_lu).max() / np.abs(x_lu).max())
    print(f"GMRES reference at k = 400: rho {its[-1].rho:.2e}, error against SuperLU {err:.2e}")
    assert err <= 1e-9


def test_coarse_blocks_of_symmetric_blocks_are_symmetric(oracle):
    rp, ci, blocks, n, b, aggs, _ = _hierarchy(oracle, "b")
    H = ir.Hierarchy(rp, ci, blocks, n, aggs)
    assert len(H.A) >= 3
    for A in H.A:
        M = A.dense() if A.n <= 400 else None
        # entry (i, j) holds the transpose of entry (j, i): a11 and a22 symmetric, a12 of one the a21 of the other
        rows = np.repeat(np.arange(A.n), np.diff(A.rp))
        slot = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(rows, A.ci))}
        t = np.array([slot[(int(j), int(i))] for i, j in zip(rows, A.ci)])
        scale = np.abs(A.bv).max()
        assert np.abs(A.bv[:, 0] - A.bv[t, 0]).max() <= 1e-17 * scale and np.abs(A.bv[:, 3] - A.bv[t, 3]).max() <= 1e-17 * scale
        assert np.abs(A.bv[:, 1] - A.bv[t, 2]).max() <= 1e-17 * scale
        if M is not None:
            assert np.abs(M - M.T).max() <= 1e-17 * scale


def test_cycle_agrees_with_the_float64_restatement_on_the_same_aggregates(oracle):
    """block_amg_ref's cycle (scipy products, SuperLU last level, float64) on ITS aggregates against the reference built from them: within c u s per field"""
    rp, ci, blocks, n, b, aggs, H64 = _hierarchy(oracle, "b")
    H = ir.Hierarchy(rp, ci, blocks, n, aggs)
    assert [2 * r for r in H.rows] == H64.rows
    for A, A64 in zip(H.A, H64.A):   # (the float64 Galerkin sums against the extended ones: a few roundings of the largest entry)
        if A.n <= 400:
            assert np.abs(A.dense() - A64.toarray().astype(ir.LD)).max() <= 16 * ir.U * np.abs(A.bv).max()
    r = ir.interleave(b)
    z64 = H64.cycle(0, r)
    z = H.cycle(0, r.astype(ir.LD))
    # the scale of one application: what the cycle adds up is bounded by |z| + 0.7 |D^-1| (|r| + |A| |z|) entrywise; its maximum per field is the unit
    s = np.abs(z) + ir.OMEGA * np.abs(ir._dinv_apply(np.abs(H.dinv[0]), np.abs(r).astype(ir.LD) + H.A[0].amv(z)))
    ref = ir.Iterate(1, ir.stack(z), ir.stack(s), 0.0, 1.0)
    ratios = ir.field_ratios(ir.stack(z64), ref)
    print(f"cycle of case b, float64 restatement against the reference: {ratios[0]:.3g} / {ratios[1]:.3g} u max s per field")
    assert max(ratios) <= ir.C_AMG[1]
