"""The reference side of tests/test_gpu_kron_iterates.py without a device (tests/kron_iter_ref.py).

Every case of the GPU test is rebuilt from the ORACLE's matrices, with aggregates from the restatement's passes in the caller's numbering
(kron_amg_ref's strength values through amg_absorb_ref's passes: any valid aggregates serve -- the device hands its own out), and the float64 checkers of
the two schemes are measured against the extended-precision reference in the units of the GPU test's bounds:
  * r_cpu(k), the worst ratio per case and k, is written to profiles/kron_iterates.txt;
  * the constants committed in kron_iter_ref (c(k) = 4 r_cpu(k) rounded up to a power of two, one set per stage: multilevel, GMRES, GMRES with a factored
    term) must be the rule's values, and none exceeds 2^12.
Cases o and p (4 225 and 25 921 DOFs at q = 33) are measured with the others -- about 5 s and 20 s of host time --: their checkers are 2 to 9 times further
from the reference than case g's on the small mesh, so a bound borrowed from g would not be theirs.
The reference checks itself: at k large enough it agrees with SuperLU on the explicit matrix to 1e-9, its float64 cycle agrees with
kron_amg_ref.Hierarchy.cycle on the same aggregates, and at q = 2 it reproduces block_iter_ref's iterates on the same aggregates."""
import os

import numpy as np
import pytest

import amg_absorb_ref as ab
import block_amg_ref as ar
import block_iter_ref as ir
import block_ref as br
import kron_amg_ref as ka
import kron_iter_ref as ki
import kron_obs_ref as ko
import kron_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "kron_iterates.txt")
_spaces, _levels = {}, {}


def _space(oracle, mesh, order):
    """-> dict(rp, ci, r1, r0, n, obs: observed nodes, mesh, dofs) from the oracle, once per (mesh, order)"""
    key = (mesh, order)
    if key not in _spaces:
        from fdapde_loader import load_package

        load_package()
        from fdapde_core_amd import meshgen

        nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
        m = oracle.Mesh(np.ascontiguousarray(nodes, dtype=float), np.ascontiguousarray(cells, dtype=np.int32), np.ascontiguousarray(bnd, dtype=np.uint8))
        dofs, _, nd, _ = oracle.enumerate_dofs(m, order)
        R1 = oracle.assemble_operator(m, order, dofs, nd, -oracle.laplacian())
        R0 = oracle.assemble_operator(m, order, dofs, nd, oracle.reaction(1.0))
        assert np.array_equal(R1.rowptr, R0.rowptr) and np.array_equal(R1.colidx, R0.colidx)
        _spaces[key] = dict(rp=np.asarray(R1.rowptr, dtype=np.int64), ci=np.asarray(R1.colidx, dtype=np.int64), r1=R1.values, r0=R0.values, n=nd,
                            obs=br.observed_nodes(m.n_nodes), mesh=m, dofs=dofs)
    return _spaces[key]


def _system(oracle, name):
    """-> (rowptr, colidx, terms, n, q, b) of ki.SYSTEMS[name]"""
    case = ki.SYSTEMS[name]
    s = _space(oracle, case[1], case[2])
    terms, q, b = ki.system(case, s["rp"], s["ci"], s["r1"], s["r0"], s["obs"])
    return s["rp"], s["ci"], terms, s["n"], q, b


def restated_aggregates(rp, ci, terms, n, coarse_rows, absorbing):
    """the restatement's passes level by level (kron_amg_ref.Hierarchy's loop with amg_absorb_ref's passes) -> the maps DOF -> DOF of the next level"""
    Ts, Ss, where = ka.merge(terms)
    q = Ts[0].shape[0]
    s = ka.strength_values(Ts, Ss, where)
    aggs = []
    while q * n > coarse_rows:
        agg, n2, rp2, ci2, v2, _ = ab._two_passes(rp, ci, [s] + list(Ss), n, absorbing)
        if n2 > ar.STALL * n and q * n2 > coarse_rows:
            break
        aggs.append(np.asarray(agg, dtype=np.int64))
        rp, ci, s, Ss, n = rp2, ci2, v2[0], v2[1:], n2
    return aggs


def _hierarchy(oracle, name):
    system, knobs, _ = ki.AMG_CASES[name]
    rp, ci, terms, n, q, b = _system(oracle, system)
    aggs = restated_aggregates(rp, ci, terms, n, knobs["amg_coarse_rows"], knobs.get("amg_absorb", 0) == 1)
    return rp, ci, terms, n, q, b, aggs


HEADER = ["# k-th iterates of the Kronecker-sum handle's two Krylov stages against the extended-precision reference (tests/kron_iter_ref.py): worst ratios per case and k.",
          "# Units: kron_amg max |x - x_ref| / (u max s) per unknown (the n entries of one unknown are a field), gmres and gmres_obs max_i |x - x_ref|_i / (u s_i);",
          "# [relres]: |relres - rho_k| / (u || |A| s || / ||b||); u = 2^-53.",
          "# cpu lines: the float64 numpy checkers (also against relres' unit), rewritten by tests/test_kron_iter_cpu.py; gpu lines: an MI355X, appended by",
          "# tests/test_gpu_kron_iterates.py under FDAPDE_KRON_ITER_PROFILE."]
STAGES = ("cpu kron_amg ", "cpu gmres ", "cpu gmres_obs ")


def _table(stage, cases, measure, constants):
    worst = ir.constants_table(PROFILE, HEADER, STAGES, stage, cases, measure, constants)
    for k, c in constants.items():
        assert c == ki.constant_for(worst[k]) <= ki.C_MAX, "every constant is the rule's value for this measurement"


def test_multilevel_constants_fit(oracle):
    def measure(name, K):
        rp, ci, terms, n, q, b, aggs = _hierarchy(oracle, name)
        restart = ki.AMG_CASES[name][1].get("gmres_m", 50)
        worst = {}
        for col in ((b, ki.second_column(b)) if name == "n" else (b,)):
            ref = ki.fgmres_iterates(ki.Hierarchy(rp, ci, terms, n, aggs), col, K, restart)
            chk = ki.fgmres_float64(rp, ci, terms, n, aggs, col, K, restart)
            for it, c in zip(ref, chk):
                worst[it.k] = max([worst.get(it.k, 0.0), ir.relres_ratio(c.rho, it)] + ki.field_ratios(c.x.astype(np.float64), it, q))
        _levels[name] = [q * len(a) for a in aggs] + [q * (int(aggs[-1].max()) + 1 if aggs else n)]
        return worst

    _table("kron_amg", [(name, case[2]) for name, case in ki.AMG_CASES.items()], measure, ki.C_AMG)
    print("rows per level:", _levels)
    for name in ki.THREE_LEVELS:
        assert len(_levels[name]) >= 3, "an inner GCR level in the restatement's numbering as well"
    assert _levels["p"][1] // 33 > 4096, "level 1 of case p holds more rows than k_kamg_spmv_dots' 1 024 workgroups take in one trip"
    assert len(_levels["k"]) == 1 and len(_levels["l"]) == 2
    assert all(v[-1] <= ki.LAST_LEVEL_ROWS for v in _levels.values())


def test_the_lds_predicate_of_case_f_on_both_sides(oracle):
    for name, in_lds in (("f", True), ("f+", False)):
        rp, ci, terms, n, q, b = _system(oracle, name)
        n_s = len(ka.merge(terms)[1])
        assert q == 16 and (n_s * q * q <= ki.LDS_FACTOR_DOUBLES) == in_lds, (name, n_s)
    assert len(ka.merge(_system(oracle, "f")[2])[1]) * 256 == ki.LDS_FACTOR_DOUBLES, "at the limit itself"


def test_gmres_constants_fit(oracle):
    def measure(name, K):
        system, knobs, rhs, _ = ki.GMRES_CASES[name]
        rp, ci, terms, n, q, b = _system(oracle, system)
        if rhs == "unit":
            b = ki.unit_rhs(n, q, ir.interior_dof(rp, n))
        restart = knobs.get("gmres_m", 50)
        ref = ki.gmres_iterates(rp, ci, terms, n, b, K, restart)
        chk = ki.gmres_float64(rp, ci, terms, n, b, K, restart)
        if rhs == "unit":
            assert all((it.s == 0).any() for it in ref), "dead entries at every k of the unit right-hand side"
        return {it.k: max(ir.entry_ratio(c.x.astype(np.float64), it), ir.relres_ratio(c.rho, it)) for it, c in zip(ref, chk)}

    _table("gmres", [(name, case[3]) for name, case in ki.GMRES_CASES.items()], measure, ki.C_GMRES)


def _obs_case(oracle, name):
    case = ki.GMRES_OBS_CASES[name]
    s = _space(oracle, case[0], 1)
    Psi = ko.design_psi(oracle, s["mesh"], None, 1, s["dofs"], s["n"], case[4])
    if case[8] == "holes":
        Psi = ki.with_holes(Psi)
    terms, q, b, obs, _ = ki.obs_system(case, s["rp"], s["ci"], s["r1"], s["r0"], Psi)
    return s, terms, q, b, obs


def test_gmres_constants_with_a_term_fit(oracle):
    def measure(name, K):
        s, terms, q, b, obs = _obs_case(oracle, name)
        rows, cols = np.diff(obs["Psi"].indptr), np.bincount(obs["Psi"].indices, minlength=s["n"])
        if name.startswith("tiles"):
            assert rows.min() >= 100, "areal rows of hundreds of entries"
        else:
            assert rows.max() <= 3
        if name == "holes":
            assert (rows == 0).any() and (cols == 0).any()
        assert (obs["W"] == 0).any() and (obs["W"] == 1).any(), "missing observations: exact zeros among the weights"
        ref = ki.gmres_iterates(s["rp"], s["ci"], terms, s["n"], b, K, obs=obs)
        chk = ki.gmres_float64(s["rp"], s["ci"], terms, s["n"], b, K, obs=obs)
        return {it.k: max(ir.entry_ratio(c.x.astype(np.float64), it), ir.relres_ratio(c.rho, it)) for it, c in zip(ref, chk)}

    _table("gmres_obs", [(name, case[9]) for name, case in ki.GMRES_OBS_CASES.items()], measure, ki.C_GMRES_OBS)


@pytest.mark.parametrize("name", ["a", "d", "l"])
def test_reference_converges_to_lu(oracle, name):
    import scipy.sparse.linalg as spl

    rp, ci, terms, n, q, b, aggs = _hierarchy(oracle, name)
    x_lu = spl.splu(kr.explicit(terms, rp, ci, n).tocsc()).solve(b)
    its = ki.fgmres_iterates(ki.Hierarchy(rp, ci, terms, n, aggs), b, 40)
    err = float(np.abs(its[-1].x - x_lu).max() / np.abs(x_lu).max())
    print(f"{name}: multilevel reference at k = 40: rho {its[-1].rho:.2e}, error against SuperLU {err:.2e}")
    assert err <= 1e-9
    rhos = [it.rho for it in its]
    assert all(b_ <= a_ * (1 + 1e-12) for a_, b_ in zip(rhos, rhos[1:]) if a_ > 1e-15), "a minimal-residual iteration: the residual does not grow"


def test_gmres_reference_converges_to_lu(oracle):
    import scipy.sparse.linalg as spl

    rp, ci, terms, n, q, b = _system(oracle, "c")
    x_lu = spl.splu(kr.explicit(terms, rp, ci, n).tocsc()).solve(b)
    its = ki.gmres_iterates(rp, ci, terms, n, b, 300, restart=300)
    err = float(np.abs(its[-1].x - x_lu).max() / np.abs(x_lu).max())
    print(f"GMRES reference at k = 300: rho {its[-1].rho:.2e}, error against SuperLU {err:.2e}")
    assert err <= 1e-9


def test_gmres_reference_with_a_term_converges_to_lu(oracle):
    """the explicit system A + scale B^T W B of kron_obs_ref (scipy.sparse.kron) against the factored reference, with a dense Phi of p > q"""
    import scipy.sparse.linalg as spl

    s, terms, q, b, obs = _obs_case(oracle, "phi-dense")
    assert obs["Phi"].shape[0] > q
    x_lu = spl.splu(ko.system(terms, s["rp"], s["ci"], s["n"], obs["Phi"], obs["Psi"], obs["W"], obs["scale"]).tocsc()).solve(b)
    its = ki.gmres_iterates(s["rp"], s["ci"], terms, s["n"], b, 400, restart=400, obs=obs)
    err = float(np.abs(its[-1].x - x_lu).max() / np.abs(x_lu).max())
    print(f"GMRES reference with a term at k = 400: rho {its[-1].rho:.2e}, error against SuperLU {err:.2e}")
    assert err <= 1e-9


def test_cycle_agrees_with_the_float64_restatement_on_the_same_aggregates(oracle):
    """kron_amg_ref's cycle (scipy products, SuperLU last level, float64) on ITS aggregates against the reference built from them: within c u max s per unknown"""
    rp, ci, terms, n, q, b = _system(oracle, "d")
    H64 = ka.Hierarchy(rp, ci, terms, n, coarse_rows=256)
    H = ki.Hierarchy(rp, ci, terms, n, H64.aggs)
    assert len(H.A) >= 3 and [q * r for r in H.rows] == H64.rows
    for A, A64 in zip(H.A, H64.A):
        if A.n * q <= 700:
            assert np.abs(A.dense() - A64.toarray().astype(ki.LD)).max() <= 16 * ki.U * float(np.abs(A.dense()).max())
    r = ki.to_rows(b, n, q)
    z64 = H64.cycle(0, r)
    z = H.cycle(0, r.astype(ki.LD))
    # the scale of one application: what the cycle adds up is bounded by |z| + 0.7 |D^-1| (|r| + |A| |z|) entrywise; its maximum per unknown is the unit
    s = np.abs(z) + ki.OMEGA * ki.dinv_apply(np.abs(ki.blocks_inverse(H.A[0].diagonal_blocks())), np.abs(r).astype(ki.LD) + H.A[0].amv(z))
    ref = ki.Iterate(1, ki.to_kron(z, n, q), ki.to_kron(s, n, q), 0.0, 1.0)
    ratios = ki.field_ratios(ki.to_kron(z64, n, q), ref, q)
    print("cycle of case d, float64 restatement against the reference, u max s per unknown:", " ".join(f"{v:.3g}" for v in ratios))
    assert max(ratios) <= ki.C_AMG[1]


def test_q2_reproduces_the_block_reference_on_the_same_aggregates(oracle):
    """four unit-T terms on the four blocks of the smoothing system: the Kronecker reference and block_iter_ref's are the same scheme on the same numbers"""
    s = _space(oracle, ki.SQ16, 1)
    rp, ci, n = s["rp"], s["ci"], s["n"]
    blocks = br.smoothing_blocks(rp, ci, s["r1"], s["r0"], s["obs"], 1e-2, n)
    b = br.smoothing_rhs(s["obs"], 1e-2, n)
    aggs = [np.asarray(P.tocsr()[::2].indices // 2, dtype=np.int64) for P in ab.BlockHierarchy(rp, ci, blocks, n, False, 64).P]
    unit = lambda r, c: np.eye(2)[:, [r]] @ np.eye(2)[[c], :]
    terms = [(unit(k // 2, k % 2), blocks[k]) for k in range(4)]
    assert len(aggs) >= 2
    kron = ki.fgmres_iterates(ki.Hierarchy(rp, ci, terms, n, aggs), b, 8)
    block = ir.fgmres_iterates(ir.Hierarchy(rp, ci, blocks, n, aggs), b, 8)
    for a, c in zip(kron, block):
        ratios = ki.field_ratios(a.x, c, 2)
        print(f"k={a.k}: the Kronecker reference against the block reference: {max(ratios):.3g} u max s, rho {a.rho:.3e} / {c.rho:.3e}")
        assert max(ratios) <= 4.0 and abs(a.rho - c.rho) <= 4.0 * ki.U * c.res_scale
    kg, bg = ki.gmres_iterates(rp, ci, terms, n, b, 8), ir.gmres_iterates(rp, ci, blocks, n, b, 8)
    for a, c in zip(kg, bg):
        assert ir.entry_ratio(a.x, c) <= 4.0
