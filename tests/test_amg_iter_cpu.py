"""The reference side of tests/test_gpu_amg_iterates.py without a device (tests/amg_iter_ref.py).

Every case of the GPU test is rebuilt from the ORACLE's matrices, with aggregates from the restatement's passes in the caller's numbering (amg_absorb_ref: any
valid aggregates serve -- the device hands its own out) and the damping of the float64 estimator, and the float64 checker of the scheme is measured against
the extended-precision reference in the units of the GPU test's bounds:
  * r_cpu(k), the worst ratio per case and k, is written to profiles/amg_iterates.txt;
  * the constants committed in amg_iter_ref (c(k) = 4 r_cpu(k) rounded up to a power of two) must still fit, and none exceeds 2^12: a relative 1e-6 defect of
    the cycle moves an iterate by 1e6 or more of the unit;
  * the damping's bound likewise: the float64 estimator against the np.longdouble one, relative, times 4, rounded up to a power of two, at most 1e-9.
The reference checks itself: at k large enough it agrees with SuperLU to 1e-9, its cycle agrees with amg_absorb_ref.ScalarHierarchy's float64 cycle on the same
aggregates, and its coarse matrices are symmetric where A is."""
import os

import numpy as np
import pytest

import amg_absorb_ref as ab
import amg_iter_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "amg_iterates.txt")
_systems, _hier = {}, {}


def _system(oracle, name):
    """-> dict(rp, ci, a = K's values, rhs, lift or None, free, bnd, coords, sym) of the system of AMG_CASES[name], from the oracle's matrices"""
    if name not in _systems:
        from fdapde_loader import load_package

        load_package()
        from fdapde_core_amd import meshgen

        mesh, order, kind, path = ir.AMG_CASES[name][:4]
        nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
        m = oracle.Mesh(np.ascontiguousarray(nodes, dtype=float), np.ascontiguousarray(cells, dtype=np.int32), np.ascontiguousarray(bnd, dtype=np.uint8))
        dofs, bd, nd, _ = oracle.enumerate_dofs(m, order)
        coords = oracle.dofs_coords(m, order, dofs, nd)
        op = -oracle.laplacian() + oracle.reaction(2.0) if kind == "reaction" else -oracle.laplacian() + oracle.advection(ir.ADVECTION) + oracle.reaction(1.0)
        A = oracle.assemble_operator(m, order, dofs, nd, op)
        rp, ci = np.asarray(A.rowptr, dtype=np.int64), np.asarray(A.colidx, dtype=np.int64)
        bd = np.asarray(bd, dtype=bool)
        if path == "solve":
            f = oracle.assemble_forcing(m, order, dofs, nd, ir.forcing(oracle.quadrature_nodes(m, order)))
            g = ir.dirichlet_data(coords)
            a = ir.unit_rows(rp, ci, A.values, bd)
            rhs, lift = np.where(bd, g, f), np.where(bd, g, 0.0)
        else:
            a, bd = np.asarray(A.values, dtype=float), np.zeros(nd, dtype=bool)
            rhs, lift = ir.Csr(rp, ci, a, np.float64).mv(np.prod(np.cos(np.pi * coords), axis=1)), None
        _systems[name] = dict(rp=rp, ci=ci, a=a, rhs=rhs, lift=lift, bnd=bd, free=~bd, coords=coords, n=nd, sym=kind == "reaction")
    return _systems[name]


def _hierarchy(oracle, name):
    """the restatement's passes on the free block, level by level -> (system, maps row -> row of the next level, float64 damping, ScalarHierarchy)"""
    if name not in _hier:
        import scipy.sparse as sp

        s = _system(oracle, name)
        free = np.flatnonzero(s["free"])
        K = sp.csr_matrix((s["a"], s["ci"], s["rp"]), shape=(s["n"], s["n"]))
        knobs = ir.AMG_CASES[name][4]
        H64 = ab.ScalarHierarchy(K[free][:, free], knobs.get("amg_absorb", 0) == 1, coarse_rows=ir.AMG_COARSE_ROWS)
        aggs = [np.asarray(P.tocsr().indices, dtype=np.int64) for P in H64.P]
        if aggs:
            a0 = np.full(s["n"], -1, dtype=np.int64)
            a0[free] = aggs[0]
            aggs[0] = a0
        # the damping: the float64 estimator on the float64 Galerkin chain (what the device holds is such a number)
        shape = ir.Hierarchy(s["rp"], s["ci"], s["a"], aggs, [1.0] * len(aggs), s["sym"], dt=np.float64, like_device=True)
        oms = [float(w) for w in shape.estimated_damping()]
        _hier[name] = (s, aggs, oms, H64)
    return _hier[name]


HEADER = ["# k-th iterates of FDAPDE_SOLVER_AMG against the extended-precision reference (tests/amg_iter_ref.py): worst ratios per case and k.",
          "# Units: max |x - x_ref| / (u max s) over the free entries; [relres]: |relres - rho_k| / (u || |K| s || / ||r_lift||); u = 2^-53.  omega: the relative",
          "# difference of the damping from the np.longdouble estimator, worst level.",
          "# cpu lines: the float64 numpy checker, rewritten by tests/test_amg_iter_cpu.py; gpu lines: an MI355X, appended by tests/test_gpu_amg_iterates.py under",
          "# FDAPDE_AMG_ITER_PROFILE; wall lines: pytest's wall time of the two iterate files on the same machine."]
STAGES = ("cpu amg ", "cpu omega ")


def _write_profile(tag, lines):
    """replace the block of lines that starts with `tag`: the header, the CPU tables in a fixed order, then whatever else the file holds (the GPU's lines)"""
    old = open(PROFILE).read().splitlines() if os.path.exists(PROFILE) else []
    groups = {t: [ln for ln in old if ln.startswith(t)] for t in STAGES}
    groups[tag] = lines
    rest = [ln for ln in old if ln and not ln.startswith("#") and not ln.startswith(STAGES)]
    new = HEADER + [ln for t in STAGES for ln in groups[t]] + rest
    if new != old:   # (a run that measures what is committed leaves the file alone)
        with open(PROFILE, "w") as fh:
            fh.write("\n".join(new) + "\n")


def test_constants_fit(oracle):
    worst, lines, rows = {}, [], {}
    for name, case in ir.AMG_CASES.items():
        ks = case[5]
        s, aggs, oms, _ = _hierarchy(oracle, name)
        H = ir.Hierarchy(s["rp"], s["ci"], s["a"], aggs, oms, s["sym"])
        ref = ir.iterates(H, s["rhs"], max(ks), s["lift"])
        chk = ir.iterates_float64(s["rp"], s["ci"], s["a"], aggs, oms, s["sym"], s["rhs"], max(ks), s["lift"])
        rows[name] = (H.rows, ir.teams(H.rows, H.entries))
        ratios = {it.k: max(ir.iterate_ratio(c.x.astype(np.float64), it, s["free"]), ir.relres_ratio(c.rho, it)) for it, c in zip(ref, chk)}
        for k in ks:
            worst[k] = max(worst.get(k, 0.0), ratios[k])
        lines.append(f"cpu amg {name}: " + " ".join(f"{k}={ratios[k]:.3g}" for k in ks))
        if s["lift"] is not None and aggs:   # (the one-level form's elimination may pivot a unit row: its boundary entries are the data to rounding)
            assert all(np.array_equal(it.x[s["bnd"]], s["lift"][s["bnd"]].astype(ir.LD)) for it in ref), (name, "the boundary entries of every iterate are the data")
    lines.append("cpu amg c(k) = 4 r_cpu(k) rounded up to a power of two: " + " ".join(f"{k}={ir.constant_for(worst[k]):g}" for k in sorted(worst)))
    print("\n".join(lines))
    print("rows per level, team widths:", rows)
    _write_profile("cpu amg ", lines)
    assert sorted(worst) == sorted(ir.C_AMG)
    for k in sorted(worst):
        assert 4.0 * worst[k] <= ir.C_AMG[k], (k, worst[k], ir.C_AMG[k])   # (r_cpu still fits c / 4)
        assert ir.C_AMG[k] <= ir.C_MAX, "a case whose checker needs more is replaced by a better-conditioned one: the constant is not raised"
    # the paths the cases are there for, in the restatement's numbering as well
    for name in "ace":
        assert len(rows[name][0]) >= 3, (name, rows[name])
    assert len(rows["b"][0]) >= 5 and len(rows["f"][0]) == 1
    assert {t for _, tm in rows.values() for t in tm} == {4, 8, 16}


def test_damping_bound_fits(oracle):
    worst, lines = 0.0, []
    for name in ir.AMG_CASES:
        s, aggs, oms, _ = _hierarchy(oracle, name)
        if not aggs:
            continue
        H = ir.Hierarchy(s["rp"], s["ci"], s["a"], aggs, oms, s["sym"])
        ld = H.estimated_damping()
        rel = [abs(float((ir.LD(w) - e) / e)) for w, e in zip(oms, ld)]
        assert all(0.0 < float(e) < 1.5 for e in ld), "1.5 / lambda_max(D^-1 A) with lambda_max > 1"
        worst = max(worst, max(rel))
        lines.append(f"cpu omega {name}: " + " ".join(f"{r:.3g}" for r in rel))
    bound = float(2.0 ** np.ceil(np.log2(4.0 * worst)))
    lines.append(f"cpu omega bound = 4 worst rounded up to a power of two: {bound:.3g} = 2^{int(np.log2(bound))}")
    print("\n".join(lines))
    _write_profile("cpu omega ", lines)
    assert 4.0 * worst <= ir.OMEGA_RTOL <= ir.OMEGA_RTOL_MAX, (worst, ir.OMEGA_RTOL)


def test_damping_in_another_row_order_is_the_permuted_matrix_s(oracle):
    """`order`: the estimator off the start vector of a device that keeps level 0's rows in another order is the estimator of the permuted matrix in its own"""
    import scipy.sparse as sp

    s, aggs, oms, _ = _hierarchy(oracle, "a")
    H = ir.Hierarchy(s["rp"], s["ci"], s["a"], aggs, oms, s["sym"])
    order = np.random.default_rng(3).permutation(s["n"])
    B = sp.csr_matrix((s["a"], s["ci"], s["rp"]), shape=(s["n"], s["n"]))[order][:, order].tocsr()
    B.sort_indices()
    there = ir.damping(ir.Csr(B.indptr, B.indices, B.data, ir.LD), H.dinv[0][order])
    here, plain = ir.damping(H.A[0], H.dinv[0], order=order), ir.damping(H.A[0], H.dinv[0])
    # (np.longdouble sums of 625 terms in another order, 15 steps: far below 1e-15; the plain order is off by about a per cent)
    assert abs(float((here - there) / there)) <= 1e-15 and abs(float((plain - there) / there)) > 1e-6, (float(here), float(there), float(plain))


@pytest.mark.parametrize("name", ["a", "c", "d", "f"])
def test_reference_converges_to_lu(oracle, name):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl

    s, aggs, oms, _ = _hierarchy(oracle, name)
    x_lu = spl.splu(sp.csr_matrix((s["a"], s["ci"], s["rp"]), shape=(s["n"], s["n"])).tocsc()).solve(s["rhs"])
    K = 1 if name == "f" else 40
    its = ir.iterates(ir.Hierarchy(s["rp"], s["ci"], s["a"], aggs, oms, s["sym"]), s["rhs"], K, s["lift"])
    err = float(np.abs(its[-1].x - x_lu).max() / np.abs(x_lu).max())
    print(f"{name}: reference at k = {K}: rho {its[-1].rho:.2e}, error against SuperLU {err:.2e}")
    assert err <= 1e-9
    rhos = [it.rho for it in its]
    assert all(b_ <= a_ * (1 + 1e-12) for a_, b_ in zip(rhos, rhos[1:]) if a_ > 1e-15), "a minimal-residual iteration: the residual does not grow"


@pytest.mark.parametrize("name", ["b", "d"])
def test_coarse_matrices_of_a_symmetric_matrix_are_symmetric(oracle, name):
    s, aggs, oms, _ = _hierarchy(oracle, name)
    H = ir.Hierarchy(s["rp"], s["ci"], s["a"], aggs, oms, s["sym"])
    assert len(H.A) >= 3
    for A in H.A[1:]:
        rows = np.repeat(np.arange(A.n), np.diff(A.rp))
        slot = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(rows, A.ci))}
        t = np.array([slot[(int(j), int(i))] for i, j in zip(rows, A.ci)])
        assert np.abs(A.a - A.a[t]).max() <= 1e-17 * np.abs(A.a).max()


@pytest.mark.parametrize("name", ["a", "b"])
def test_cycle_agrees_with_the_float64_restatement_on_the_same_aggregates(oracle, name):
    """amg_absorb_ref.ScalarHierarchy's cycle (scipy products, SuperLU last level, float64, flexible-CG steps) on ITS aggregates and this damping against the
    reference built from them, on the free block: within c u max s"""
    s, aggs, oms, H64 = _hierarchy(oracle, name)
    H = ir.Hierarchy(s["rp"], s["ci"], s["a"], aggs, oms, s["sym"])
    assert H.rows[1:] == H64.rows[1:] and H64.rows[0] == int(s["free"].sum())
    for A, A64 in zip(H.A[1:], H64.A[1:]):   # (the float64 Galerkin sums against the extended ones: a few roundings of the largest entry)
        assert np.abs(A.dense() - A64.toarray().astype(ir.LD)).max() <= 16 * ir.U * np.abs(A.a).max()
    H64.omd = [w * (1.0 / A.diagonal()) for w, A in zip(oms, H64.A[:-1])]
    free = s["free"]
    r = np.where(free, s["rhs"], 0.0)
    z64 = H64.cycle(0, r[free])
    z = H.cycle(0, r.astype(ir.LD))
    assert not z[~free].any(), "the correction is 0 on the rows of no aggregate"
    # the scale of one application: what the cycle adds up is bounded by |z| + om |D^-1| (|r| + |A| |z|) entrywise; its maximum is the unit
    sc = np.abs(z) + H.om[0] * np.abs(H.dinv[0]) * (np.abs(r).astype(ir.LD) + H.A[0].amv(z))
    ratio = float(np.abs(z64.astype(ir.LD) - z[free]).max() / (ir.U * sc[free].max()))
    print(f"cycle of case {name}, float64 restatement against the reference: {ratio:.3g} u max s")
    assert ratio <= ir.C_AMG[1]
