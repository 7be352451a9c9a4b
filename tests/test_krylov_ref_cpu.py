"""The extended-precision Krylov reference (tests/krylov_ref.py) pinned, and the float64 checkers measured against it -- CPU only.

  1. closed forms: x_1 = (bt.bt / bt.At bt) S bt; on a 3x3 and a 5x5 SPD matrix iterate n is the exact solution to 1e-17 relative; BiCGStab on a 2x2
     matrix after 2 iterations likewise.
  2. the np.longdouble iterates stay within 0.01 u s_i of 60-digit mpmath on three small systems (0.003 u measured).
  3. the tolerance of tests/test_gpu_krylov_iterates.py is measured here: its systems, at their test sizes, rebuilt on the CPU (the C oracle assembles the
     same meshes; tests/segment_ref.py the network; the handle's crafted matrices on the oracle's pattern), through the three float64 checkers.
     r_cpu(k) = max_i |x_float64 - x_ref|_i / (u s_i); the GPU constant is c = 4 r_cpu rounded up to a power of two and stands in
     krylov_systems.BOUNDS next to the r_cpu it came from.  This file fails if a measured r_cpu no longer fits its c / 4, or exceeds 64 on
     any input: the cap is a condition on the inputs, not a measurement (such an input is replaced, never given a larger c).  The same for info.relres:
     the checkers' recurrence residual -- explicit r.r, and for the fused variant also its estimate alpha^2 Ap.Ap - r.r -- against the reference's,
     in units of u max(rho_k, rho_k-1): r_k = r_k-1 - alpha At p is rounded relative to r_k-1.  What the issue's own unit, u rho_k, would have to
     admit is recorded next to it (the checkers are thousands of u rho_k off where one iteration takes the residual down by orders of magnitude).
     Every system has an iteration the stop test can be aimed at (pick_stop).
     FDAPDE_KRYLOV_PROFILE=<path> writes the table (profiles/krylov_iterates.txt is such a run)."""
import os

import mpmath as mp
import numpy as np
import pytest

import krylov_ref as kr
import krylov_systems as G
import segment_ref as sg
from oracle import oracle as o

LD = kr.LD
U = kr.U


@pytest.fixture(scope="module")
def meshgen():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import meshgen as m

    o.build()
    return m


# ---- 1. closed forms ----------------------------------------------------------------------------------------------------------------------------
def _dense_csr(A):
    A = np.asarray(A, float)
    n = A.shape[0]
    return np.arange(0, n * n + 1, n), np.tile(np.arange(n), n), A.reshape(-1)


def _exact_solve(A, b, digits=60):
    with mp.workdps(digits):
        x = mp.lu_solve(mp.matrix([[mp.mpf(float(v)) for v in row] for row in A]), mp.matrix([mp.mpf(float(v)) for v in b]))
        return [x[i] for i in range(len(b))]


def _to_mp(v):
    """an np.longdouble as an mpf, exactly (two float64 pieces)"""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))


def test_first_iterate_closed_form():
    rng = np.random.default_rng(0)
    M = rng.standard_normal((6, 6))
    A = M @ M.T + 6 * np.eye(6)
    b = rng.standard_normal(6)
    rp, ci, v = _dense_csr(A)
    sy = kr.System(rp, ci, v, b)
    it = kr.cg_iterates(sy, None, 1)[0]
    Atb = sy.mv(sy.bt)
    x1 = (sy.bt @ sy.bt) / (sy.bt @ Atb) * sy.S * sy.bt
    assert np.abs(it.x - x1).max() <= 4 * np.finfo(LD).eps * np.abs(x1).max()
    assert (it.s >= np.abs(it.x)).all()


@pytest.mark.parametrize("n", [3, 5])
def test_cg_iterate_n_is_the_solution(n):
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = Q @ np.diag(np.linspace(1.0, 3.0, n)) @ Q.T
    A = 0.5 * (A + A.T)
    b = rng.standard_normal(n)
    its = kr.cg_iterates(_dense_csr(A), b, n)
    x = _exact_solve(A, b)
    with mp.workdps(60):
        err = max(abs(_to_mp(its[-1].x[i]) - x[i]) for i in range(n)) / max(abs(v) for v in x)
    assert err <= mp.mpf("1e-17"), err
    assert its[-1].rho <= 1e-17


def test_bicgstab_iterate_2_of_a_2x2_is_the_solution():
    A = np.array([[2.0, 0.7], [-0.4, 1.5]])
    b = np.array([1.0, -0.3])
    its = kr.bicgstab_iterates(_dense_csr(A), b, 2)
    x = _exact_solve(A, b)
    with mp.workdps(60):
        err = max(abs(_to_mp(its[-1].x[i]) - x[i]) for i in range(2)) / max(abs(v) for v in x)
    assert err <= mp.mpf("1e-17"), err


def test_dirichlet_reduction_and_front():
    """1-D Laplacian with Dirichlet ends: the module reduces the system itself; from a one-entry right-hand side the front moves one row per iteration and
    the scale is exactly 0 ahead of it"""
    n = 12
    A = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    bnd = np.zeros(n, np.uint8)
    bnd[[0, n - 1]] = 1
    g = np.linspace(1.0, 2.0, n)
    f = np.zeros(n)
    f[5] = 1.0
    rp, ci, v = _dense_csr(A)
    keep = v != 0
    rp = np.concatenate([[0], np.cumsum(keep.reshape(n, n).sum(axis=1))])
    sy = kr.System(rp, ci[keep], v[keep], f, bnd, g)
    assert sy.ni == n - 2 and sy.bt[0] != 0 and sy.bt[-1] != 0   # the lift reaches the rows next to the ends
    its = kr.cg_iterates(sy, None, 2)
    ahead = [2, 6, 7]   # interior rows with no neighbour among the rows of bt (0, 4, 9)
    assert (its[0].s[ahead] == 0).all() and (its[0].x[ahead] == 0).all() and its[0].s[4] > 0 and (its[1].s[ahead] > 0).all()
    u = sy.lift(its[1].x)
    assert u[0] == g[0] and u[-1] == g[-1]


# ---- 2. longdouble against 60 digits ------------------------------------------------------------------------------------------------------------
def _small_systems(meshgen):
    out = []
    for nx, react, adv in ((8, 0.4, False), (12, 50.0, False), (10, 0.4, True)):
        nodes, cells, bnd = meshgen.unit_square(nx)
        m = o.Mesh(nodes, cells, bnd)
        dofs, bd, nd, _ = o.enumerate_dofs(m, 1)
        op = -o.laplacian() + o.reaction(react)
        if adv:
            op = op + o.advection(np.array(G.ADV[:2]))
        A = o.assemble_operator(m, 1, dofs, nd, op)
        qn = o.quadrature_nodes(m, 1)
        f = o.assemble_forcing(m, 1, dofs, nd, G.forcing_of(qn, cells.shape[0], "smooth"))
        g = 0.25 * o.dofs_coords(m, 1, dofs, nd)[:, 0]
        out.append((A.rowptr, A.colidx, A.values, f, bd, g, "bicgstab" if adv else "cg"))
    return out


def test_longdouble_against_mpmath(meshgen):
    worst = 0.0
    for rp, ci, v, f, bd, g, method in _small_systems(meshgen):
        K = 3 if method == "bicgstab" else 12
        sy = kr.System(rp, ci, v, f, bd, g)
        its = kr.cg_iterates(sy, None, K) if method == "cg" else kr.bicgstab_iterates(sy, None, K)
        ref = kr.mp_iterates(rp, ci, v, f, K, bd, g, method=method)
        with mp.workdps(60):
            for it, (x, s, rho) in zip(its, ref):
                for i in range(sy.ni):
                    if s[i] == 0:
                        assert it.x[i] == 0 and it.s[i] == 0
                        continue
                    worst = max(worst, float(abs(_to_mp(it.x[i]) - x[i]) / (mp.mpf(U) * s[i])))
                    assert abs(_to_mp(it.s[i]) - s[i]) <= mp.mpf("1e-15") * s[i]
                assert abs(mp.mpf(it.rho) - rho) <= mp.mpf("1e-14") * rho
    print(f"longdouble against mpmath: worst {worst:.4f} u s_i")
    assert worst <= 0.01, worst


# ---- 3. the tolerance ---------------------------------------------------------------------------------------------------------------------------
def cpu_system(meshgen, name, rhs):
    """(rowptr, colidx, vals, f, bnd, g) of a system of the GPU tests, from the CPU checkers' assembly of the same mesh"""
    s = G.spec_of(name)
    nodes, cells, bnd = G.mesh_of(meshgen, s)
    if s["dim"] == 1:
        op = G.operator_of(o, s)
        dt, dbnd, nd = sg.dofs(cells, nodes.shape[0], bnd, s["order"])
        A = sg.assemble(nodes, cells, dt, nd, s["order"], op)
        qn = sg.quadrature_nodes(nodes, cells, s["order"])
        f = sg.forcing(nodes, cells, dt, nd, s["order"], G.forcing_of(qn, cells.shape[0], G.FORCING.get((name, rhs), rhs)))
        g = 0.25 * sg.dof_coords(nodes, cells, s["order"])[:, 0]
        return A.indptr, A.indices, A.data, f, dbnd, g
    m = o.Mesh(nodes, cells, bnd if s["dirichlet"] else np.zeros_like(bnd))
    dofs, bd, nd, _ = o.enumerate_dofs(m, s["order"])
    A = o.assemble_operator(m, s["order"], dofs, nd, G.operator_of(o, s))
    qn = o.quadrature_nodes(m, s["order"])
    f = o.assemble_forcing(m, s["order"], dofs, nd, G.forcing_of(qn, cells.shape[0], G.FORCING.get((name, rhs), rhs)))
    g = 0.25 * o.dofs_coords(m, s["order"], dofs, nd)[:, 0] if s["dirichlet"] else None
    return A.rowptr, A.colidx, A.values, f, (bd if s["dirichlet"] else None), g


def cpu_handle(meshgen, hname):
    s = G.HANDLES[hname]
    nodes, cells, bnd = meshgen.unit_square(s["nx"]) if s["dim"] == 2 else meshgen.unit_cube(s["nx"])
    m = o.Mesh(nodes, cells, bnd)
    dofs, _, nd, _ = o.enumerate_dofs(m, s["order"])
    A = o.assemble_operator(m, s["order"], dofs, nd, o.reaction(1.0))
    coords = o.dofs_coords(m, s["order"], dofs, nd)
    return A.rowptr, A.colidx, G.crafted_values(A.rowptr, A.colidx, seed=7), G.handle_rhs(coords, G.HANDLE_COLUMNS, seed=11)


def _measure(sy_data, method):
    """-> ({k: r_cpu}, worst relres error in units of u max(rho_k, rho_k-1), the same in units of u rho_k (the issue's wording), [rho_k])"""
    rp, ci, v, f, bd, g = sy_data
    K = max(G.K_BICG) if method == "bicgstab" else max(G.K_CG)
    sy = kr.System(rp, ci, v, f, bd, g)
    ref = kr.cg_iterates(sy, None, K) if method == "cg" else kr.bicgstab_iterates(sy, None, K)
    checkers = (kr.cg_float64, kr.cg_fused_float64) if method == "cg" else (kr.bicgstab_float64,)
    r, rel, rel_k = {}, 0.0, 0.0
    for chk in checkers:
        prev = 1.0
        for it, rf in zip(chk(sy, None, K), ref):
            r[it.k] = max(r.get(it.k, 0.0), kr.ratio(it.x, rf))
            den = U * max(prev, rf.rho)   # (r_k = r_{k-1} - alpha At p: the rounding of r_k is relative to r_{k-1} where the update cancels)
            rel = max(rel, abs(it.rho - rf.rho) / den)
            rel_k = max(rel_k, abs(it.rho - rf.rho) / (U * rf.rho))
            if it.rho_est is not None:
                rel = max(rel, abs(it.rho_est - rf.rho) / den)
                rel_k = max(rel_k, abs(it.rho_est - rf.rho) / (U * rf.rho))
            prev = rf.rho
    return r, rel, rel_k, [it.rho for it in ref]


def _inputs(meshgen):
    for name in G.SYSTEMS:
        method = "bicgstab" if G.spec_of(name)["adv"] else "cg"
        for rhs in G.RHS:
            yield f"{name}/{rhs}", method, cpu_system(meshgen, name, rhs), (name, rhs) not in G.NO_STOP
    for hname in G.HANDLES:
        rp, ci, v, B = cpu_handle(meshgen, hname)
        for j in range(B.shape[1]):
            yield f"handle {hname}/column {j}", "cg", (rp, ci, v, B[:, j], None, None), j < 2 or j == G.HANDLE_COLUMNS - 1


def test_checkers_fit_the_constants(meshgen):
    lines = []
    worst = {m: {kmax: 0.0 for kmax in G.BOUNDS[m]} for m in G.BOUNDS}
    worst_rel = {m: 0.0 for m in G.BOUNDS}
    worst_rel_k = {m: 0.0 for m in G.BOUNDS}   # what the issue's own normalisation, u rho_k, would have to admit: recorded, not used
    handle_rhos = {}
    for label, method, data, stops in _inputs(meshgen):
        r, rel, rel_k, rhos = _measure(data, method)
        worst_rel_k[method] = max(worst_rel_k[method], rel_k)
        if label.startswith("handle"):
            handle_rhos.setdefault(label.split("/")[0], []).append(rhos)
        assert max(r.values()) <= 64.0, f"{label}: its own float64 checker is {max(r.values()):.3g} u s_i off: replace the input, not the constant"
        for kmax in G.BOUNDS[method]:
            worst[method][kmax] = max(worst[method][kmax], max(v for k, v in r.items() if k <= kmax))
        worst_rel[method] = max(worst_rel[method], rel)
        pick = G.pick_stop(rhos, max(r))
        if stops:
            assert pick is not None, f"{label}: no iteration k <= {max(r)} whose residual drops below 0.7 of every earlier one"
        lines.append(f"cpu {label} [{method}]: " + " ".join(f"r_cpu({k})={v:.3g}" for k, v in sorted(r.items())) + f" relres={rel:.3g}u (of rho_k alone: {rel_k:.3g}u) stop@{pick[0] if pick else '-'}")
    for m in G.BOUNDS:
        for kmax, (r_rec, c) in G.BOUNDS[m].items():
            lines.append(f"constant {m} k<={kmax}: r_cpu = {worst[m][kmax]:.3g} (recorded {r_rec:g}), c = {c:g}")
        lines.append(f"constant {m} relres: {worst_rel[m]:.3g} u (recorded {G.RELRES[m][0]:g}), margin = {G.RELRES[m][1]:g} u of max(rho_k, rho_k-1); "
                     f"in units of u rho_k, the issue's wording, the checkers themselves are {worst_rel_k[m]:.3g} u off where the residual drops sharply")
    # the calls with several columns (6 side by side; 12 = batches of 8 and 4; 13 = the same and one column by itself): ONE tolerance between two
    # residual ratios of every column of the call
    for hname, rhos_of in handle_rhos.items():
        for n_cols in (6, 12, G.HANDLE_COLUMNS):
            pick = G.pick_stop_columns(rhos_of[:n_cols], max(G.K_CG))
            assert pick is not None, f"{hname}: no common tolerance for the first {n_cols} columns"
            lines.append(f"cpu {hname} {n_cols} columns: rtol={pick[0]:.4g} (margin {pick[2]:.3f}) stops at {pick[1]}")
    print("\n".join(lines))
    path = os.environ.get("FDAPDE_KRYLOV_PROFILE")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    for m in G.BOUNDS:
        for kmax, (r_rec, c) in G.BOUNDS[m].items():
            assert worst[m][kmax] <= r_rec and c == 2.0 ** np.ceil(np.log2(4.0 * r_rec)), (m, kmax, worst[m][kmax], r_rec, c)
        assert worst_rel[m] <= G.RELRES[m][0] and G.RELRES[m][1] == 2.0 ** np.ceil(np.log2(4.0 * G.RELRES[m][0])), (m, worst_rel[m])
