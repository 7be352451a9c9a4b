"""Every Krylov form's k-th iterate against the extended-precision reference of tests/krylov_ref.py.

`rtol = 1e-30, maxit = k` stops a solve after exactly k iterations and hands the iterate out.  In exact arithmetic that iterate is one vector, whatever the
recurrence variant, the storage, the partition and the hand-offs, so every form is held to

    |u_gpu - u_ref|_i <= c(k) u s_i + F_i,        u = 2^-53,

with s_i the magnitude of everything that was added up to make entry i (krylov_ref.py), F_i = 0 for the plain storage and the fixed-point bound documented
in kernels_persist.h for the symmetric one (krylov_ref.symmetric_storage_bound: derived, not measured).  Where s_i = 0 the Krylov front has not arrived: the
entry is exactly the Dirichlet lift.  A converged solve corrects its own mistakes; an iterate does not -- a dot product that drops a row or a workgroup's
partial, a wrong fused beta estimate, an operator wrong at 1e-11 in a few rows, a stop test one iteration late and a relres that is not the residual of what
is handed out all show here by orders of magnitude.

c(k) = 4 r_cpu(k) rounded up to a power of two, r_cpu the worst ratio of the float64 numpy checkers of the same recurrences on the same systems
(tests/test_krylov_ref_cpu.py measures it and fails if it no longer fits; profiles/krylov_iterates.txt).  Every test asserts that the form it names ran,
the two paths that leave no other trace -- k_small_front and the replay of a captured graph -- through fdapde_solver_trace.  The systems and constants
stand in tests/krylov_systems.py, which the CPU test shares.

FDAPDE_KRYLOV_PROFILE=<path> appends the worst ratio per form."""
import os

import numpy as np
import pytest

import krylov_ref as kr
from krylov_systems import (FORCING, HANDLE_COLUMNS, HANDLES, K_BICG, K_CG, NO_STOP, RELRES, RHS, c_of, crafted_values, forcing_of, handle_rhs, mesh_of,
                            operator_of, pick_stop, pick_stop_columns, spec_of)

U = kr.U


# ---- GPU side ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen

    assert capi.load().fdapde_device_count() >= 1
    return capi, meshgen


_REF = {}       # (system, rhs, method) -> (vals, System, [Iterate])
_WORST = {}     # form -> {k: ratio}


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("FDAPDE_KRYLOV_PROFILE")
    if path and _WORST:
        with open(path, "a") as fh:
            for form in sorted(_WORST):
                fh.write(f"gpu {form}: " + " ".join(f"{k}={v:.3g}" for k, v in sorted(_WORST[form].items(), key=lambda kv: str(kv[0]))) + "\n")


def _note(form, k, value):
    d = _WORST.setdefault(form, {})
    d[k] = max(d.get(k, 0.0), value)


def _context(env, name, rhs):
    capi, meshgen = env
    s = spec_of(name)
    nodes, cells, bnd = mesh_of(meshgen, s)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd if s["dirichlet"] else np.zeros_like(bnd))
    nd = c.dofs_build(s["order"])
    _, dbnd, coords = c.dofs_get()
    c.set_operator(operator_of(capi, s))
    c.set_forcing(forcing_of(c.quadrature_nodes(), cells.shape[0], FORCING.get((name, rhs), rhs)))
    g = 0.25 * coords[:, 0] if s["dirichlet"] else None
    c.set_dirichlet(g)
    c.init()
    c.tune("dense_rows", 0)
    rp, ci = c.pattern_get()
    vals = c.matrix_values(capi.MAT_STIFF)   # BEFORE the first solve: a Dirichlet solve leaves the row-zeroed matrix behind
    f = c.force()
    return c, s, (rp, ci, vals, f, dbnd if s["dirichlet"] else None, g)


def _reference(key, data, method, K):
    rp, ci, vals, f, bnd, g = data
    hit = _REF.get(key)
    if hit is None or not (np.array_equal(hit[0], vals) and np.array_equal(hit[1].f, f)):
        sy = kr.System(rp, ci, vals, f, bnd, g)
        its = kr.cg_iterates(sy, None, K) if method == "cg" else kr.bicgstab_iterates(sy, None, K)
        hit = _REF[key] = (vals, sy, its)
    return hit[1], hit[2]


def _check_iterate(form, method, sy, its, k, u, sym, max_len, tag=None):
    it = its[k - 1]
    bndmask = np.ones(sy.n, dtype=bool)
    bndmask[sy.interior] = False
    assert np.array_equal(u[bndmask], sy.gt[bndmask]), "Dirichlet entries are the data, exactly"
    x = u[sy.interior]
    err = np.abs(x.astype(kr.LD) - it.x)
    dead = it.s == 0
    assert not err[dead].any(), f"{form} k={k}: entries the Krylov front has not reached must be exactly the lift ({int((err[dead] != 0).sum())} are not)"
    bound = c_of(method, k) * U * it.s
    if sym:
        F = kr.symmetric_storage_bound(sy, its, k, max_len)
        live = ~dead
        _note(form + " [fixed-point share |err| / F]", tag or k, float((err[live] / F[live]).max()) if live.any() else 0.0)
        bound = bound + np.where(dead, 0, F)
    live = ~dead
    ratio = float((err[live] / (U * it.s[live])).max()) if live.any() else 0.0
    _note(form, tag or k, ratio)
    print(f"{form} k={k}: worst |err| / (u s) = {ratio:.3g}  (c = {c_of(method, k):g}{', + F' if sym else ''})")
    bad = err > bound
    assert not bad.any(), (form, k, ratio, int(bad.sum()), float((err / np.maximum(bound, 1e-300)).max()))


def _check_relres(form, method, its, k, relres, sy=None, max_len=0):
    """info.relres against the reference's ||r_k|| / ||bt||, relative to the larger of it and its predecessor: r_k = r_{k-1} - alpha At p is rounded
    relative to r_{k-1} where the update cancels (in units of u rho_k alone the float64 checkers themselves are 151 u off, tests/test_krylov_ref_cpu.py
    records it, against 52 u in this unit).  sy given (symmetric storage): plus what the documented fixed-point bound allows the residual"""
    rho = its[k - 1].rho
    den = U * max(rho, its[k - 2].rho if k > 1 else 1.0)
    slack = kr.symmetric_storage_residual_slack(sy, its, k, max_len) if sy is not None else 0.0
    _note(form + " [relres, units of u]", k, abs(relres - rho) / den)
    assert abs(relres - rho) <= RELRES[method][1] * den + slack, (form, k, relres, rho, abs(relres - rho) / den, slack)


def _run_solve_form(env, name, rhs, knobs, method, expect, form):
    """maxit runs k in K, then the stop test, on one context; `expect(c, info)` asserts the form"""
    capi, _ = env
    c, s, data = _context(env, name, rhs)
    try:
        for k_, v_ in knobs.items():
            if k_ != "check_every":
                c.tune(k_, v_)
        ce = knobs.get("check_every", 0)
        bicg = method == capi.SOLVER_BICGSTAB
        mname = "bicgstab" if bicg else "cg"
        Ks = K_BICG if bicg else K_CG
        sy, its = _reference((name, rhs, mname), data, mname, max(Ks))
        max_len = int(np.diff(data[0]).max())
        sym = None
        for k in Ks:
            info = c.solve(method=method, rtol=1e-30, maxit=k, check_every=ce, raise_on_noconv=False)
            assert info.iters == k and info.converged == 0 and info.method_used == method, (info.iters, info.converged, info.method_used)
            sym = expect(c, info)
            _check_iterate(form, mname, sy, its, k, c.solution(), sym, max_len)
            _check_relres(form, mname, its, k, info.relres, sy if sym else None, max_len)
        # the stop test: a tolerance between two residual ratios of the reference must stop the solve at exactly that iteration (the single-launch
        # BiCGStab sums r.r half an iteration late -- kernels_persist_bicg.h -- but x is final by then and the count is the same)
        pick = pick_stop([it.rho for it in its], max(Ks))
        if (name, rhs) in NO_STOP:
            assert pick is None
            return
        assert pick is not None, "the system was chosen to have such an iteration (tests/test_krylov_ref_cpu.py checks it)"
        k, rtol = pick
        info = c.solve(method=method, rtol=rtol, check_every=ce)
        assert info.converged == 1 and info.iters == k, (info.iters, k, info.relres, rtol)
        expect(c, info)
        _check_iterate(form, mname, sy, its, k, c.solution(), sym, max_len, tag=f"stop@{k}")
        _check_relres(form, mname, its, k, info.relres, sy if sym else None, max_len)
    finally:
        c.close()


# ---- single-launch CG ----------------------------------------------------------------------------------------------------------------------------
# (system, knobs, expected layout: kind (2 streaming | 3 resident), sym, workgroups (exact, or ">=2"), rows per thread (or None), partition (or None))
# front: fdapde_solver_trace's small_front -- k_small_front takes a one-workgroup layout of the PLAIN storage only (solve_prepare), so under persist_sym = 1
# the knob small_front_rows selects nothing: the two symmetric sq20 cases run the same launches, and say so by asserting front = 0 in both
PERSIST_CG = [
    ("sq20", dict(persist_sym=0), dict(sym=0, wg=1, front=1)),
    ("sq20", dict(persist_sym=1), dict(sym=1, wg=1, front=0)),
    ("sq20", dict(persist_sym=0, small_front_rows=0), dict(sym=0, wg=1, front=0)),
    ("sq20", dict(persist_sym=1, small_front_rows=0), dict(sym=1, wg=1, front=0)),
    ("sq60", dict(persist_sym=0, persist_partition=0), dict(sym=0, wg=2, kind=3, part=0)),
    ("sq60", dict(persist_sym=1, persist_partition=0), dict(sym=1, wg=2, kind=3, part=0)),
    ("sq60", dict(persist_sym=0, persist_partition=1), dict(sym=0, wg=2, kind=3, part=1)),
    ("sq60", dict(persist_sym=1, persist_partition=1), dict(sym=1, wg=2, kind=3, part=1)),
    # (rows of up to 65 entries: the symmetric blocks are resident; the plain ones stream even at the smallest block, 2 rows per thread)
    ("cube12p2", dict(persist_sym=0), dict(sym=0, kind=2, rpt=2)),
    ("cube12p2", dict(persist_sym=1), dict(sym=1, kind=3, rpt=2)),
    ("cube25", dict(persist_max_wg=2, persist_sym=1, persist_partition=0), dict(sym=1, wg=2, kind=2, rpt=16, part=0)),   # the benchmark's instantiation
    ("cube25", dict(persist_max_wg=2, persist_sym=1, persist_partition=1), dict(sym=1, wg=2, kind=2, rpt=16, part=1)),
    ("cube25", dict(persist_max_wg=2, persist_sym=0, persist_partition=0), dict(sym=0, wg=2, kind=2, rpt=16, part=0)),
    ("cube25", dict(persist_max_wg=2, persist_sym=0, persist_partition=1), dict(sym=0, wg=2, kind=2, rpt=16, part=1)),
    ("cube25", dict(persist_max_wg=4, persist_sym=0), dict(sym=0, wg=4, rpt=8)),
    ("cube25", dict(persist_max_wg=4, persist_sym=1), dict(sym=1, wg=4, rpt=8)),
    ("cube25", dict(persist_max_wg=8, persist_sym=0), dict(sym=0, wg=8, rpt=4)),
    ("cube25", dict(persist_max_wg=8, persist_sym=1), dict(sym=1, wg=8, rpt=4)),
    ("sq200", dict(persist_max_wg=4), dict(sym=0, rpt=24, kind=2)),   # the wide form: x in HBM
    ("sq150free", dict(persist_sym=0), dict(sym=0)),
    ("sq150free", dict(persist_sym=1), dict(sym=1)),
]


def _id(case):
    return case[0] + "-" + "-".join(f"{k}{v}" for k, v in case[1].items())


def _expect_layout(want, dirichlet):
    solves = [0]

    def expect(c, info):
        solves[0] += 1
        lay = c.solver_layout_kind(dirichlet)
        assert info.persistent == 1, "the single launch must have run"
        assert lay["sym"] == want["sym"], lay
        if "wg" in want:
            assert lay["workgroups"] == want["wg"], lay
        if "kind" in want:
            assert lay["kind"] == want["kind"], lay
        else:
            assert lay["kind"] in (2, 3), lay
        if "rpt" in want:
            assert lay["rows_per_thread"] == want["rpt"], lay
        if "part" in want:
            assert c.solver_layout_partition(dirichlet) == want["part"]
        if "front" in want and solves[0] > 1:   # (a context's first solve builds the layout's column table and leaves the front to the separate kernels)
            assert c.solver_trace()["small_front"] == want["front"], "k_small_front in front of the launch, or the separate kernels"
        return want["sym"] == 1
    return expect


@pytest.mark.gpu
@pytest.mark.parametrize("rhs", RHS)
@pytest.mark.parametrize("case", PERSIST_CG, ids=_id)
def test_single_launch_cg_iterates(env, case, rhs):
    capi, _ = env
    name, knobs, want = case
    _run_solve_form(env, name, rhs, knobs, capi.SOLVER_CG_FUSED, _expect_layout(want, spec_of(name)["dirichlet"]), "k_cg_persist " + _id(case))


# ---- multi-launch solvers ------------------------------------------------------------------------------------------------------------------------
def _multi_cases():
    out = []
    for name in ("cube16", "sq24p2"):
        for blocked in (0, 2):   # (the default, 1, keeps the CSR kernel on systems this small: 2 is what runs k_spmv_blocked here)
            out.append((name, "SOLVER_CG", dict(persist=0, blocked=blocked)))
            out.append((name, "SOLVER_CG_SR", dict(persist=0, blocked=blocked)))
            for lazy in (0, 1):
                for graph in (0, 1):
                    kn = dict(persist=0, blocked=blocked, cgf_lazy=lazy, use_graph=graph)
                    if graph:
                        kn["check_every"] = 2   # (a graph replays whole even chunks: with the default of 32 no run of <= 12 iterations would replay one)
                    out.append((name, "SOLVER_CG_FUSED", kn))
            out.append((name + "adv", "SOLVER_BICGSTAB", dict(persist=0, blocked=blocked)))
    return out



@pytest.mark.gpu
@pytest.mark.parametrize("rhs", RHS)
@pytest.mark.parametrize("case", _multi_cases(), ids=lambda cs: cs[0] + "-" + cs[1] + "-" + "-".join(f"{k}{v}" for k, v in cs[2].items()))
def test_multi_launch_iterates(env, case, rhs):
    capi, _ = env
    name, mname, knobs = case

    def expect(c, info):
        assert info.persistent == 0
        assert c.solver_layout_kind(True)["kind"] == (1 if knobs["blocked"] else 0), "CSR kernel with blocked = 0, blocked ELL with 2"
        if "use_graph" in knobs:
            # a capture or an instantiation that fails falls back to plain launches without a word: the replays are counted.  With check_every = 2
            # every whole pair of iterations is one replay: an odd budget ends with one plain launch, a solve that converges in an odd iteration
            # inside a replayed pair (whose second half then does nothing)
            pairs = (info.iters + 1) // 2 if info.converged else info.iters // 2
            assert c.solver_trace()["graph_replays"] == (pairs if knobs["use_graph"] else 0), (c.solver_trace(), info.iters)
        return False

    _run_solve_form(env, name, rhs, knobs, getattr(capi, mname), expect, f"multi-launch {mname} {name} " + " ".join(f"{k}={v}" for k, v in knobs.items()))


# ---- single-launch BiCGStab ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rhs", RHS)
@pytest.mark.parametrize("name,knobs,wg", [("sq60adv", {}, 2), ("cube25adv", dict(persist_max_wg=8), 8)])
def test_single_launch_bicgstab_iterates(env, name, knobs, wg, rhs):
    capi, _ = env

    def expect(c, info):
        lay = c.solver_layout_kind(True)
        assert info.persistent == 1 and lay["sym"] == 0 and lay["workgroups"] == wg and lay["rows_per_thread"] <= 8, lay
        return False

    _run_solve_form(env, name, rhs, knobs, capi.SOLVER_BICGSTAB, expect, f"k_bicg_persist {name}")


# ---- the factor-once handle ----------------------------------------------------------------------------------------------------------------------
def _handle(env, hname):
    capi, meshgen = env
    s = HANDLES[hname]
    nodes, cells, bnd = meshgen.unit_square(s["nx"]) if s["dim"] == 2 else meshgen.unit_cube(s["nx"])
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(s["order"])
    _, _, coords = c.dofs_get()
    c.tune("dense_rows", 0)
    rp, ci = c.pattern_get()
    vals = crafted_values(rp, ci, seed=7)
    return c, rp, ci, vals, coords


# (form, knobs, columns of a call, how the call deals them out: the sizes of the groups whose iterations info.iters adds up -- columns side by side or
#  one by one count each for itself, a batch of 8 / 4 counts its slowest column: include/fdapde_hip.h)
HANDLE_FORMS = [
    ("direct", dict(persist_single_rows=8192, persist_direct=1), 1, (1,)),
    ("general", dict(persist_single_rows=8192, persist_direct=0), 1, (1,)),
    ("one-column", dict(), 1, (1,)),
    ("side-by-side", dict(), 6, (1,) * 6),
    ("batches", dict(persist=0), 12, (8, 4)),
    ("batches-and-one", dict(persist=0), HANDLE_COLUMNS, (8, 4, 1)),   # 13 columns: what the batches leave goes through e_lin_solve's column-by-column loop
    ("direct-sym", dict(persist_single_rows=8192, persist_direct=1, persist_sym=1), 1, (1,)),
    ("general-sym", dict(persist_single_rows=8192, persist_direct=0, persist_sym=1), 1, (1,)),
    ("one-column-sym", dict(persist_sym=1), 1, (1,)),
    ("side-by-side-sym", dict(persist_sym=1), 6, (1,) * 6),
]


@pytest.mark.gpu
@pytest.mark.parametrize("form,knobs,n_cols,groups", HANDLE_FORMS, ids=[f[0] for f in HANDLE_FORMS])
@pytest.mark.parametrize("hname", list(HANDLES))
def test_handle_iterates(env, hname, form, knobs, n_cols, groups):
    capi, _ = env
    c, rp, ci, vals, coords = _handle(env, hname)
    try:
        for k_, v_ in knobs.items():
            c.tune(k_, v_)
        c.lin_compute(values=vals, symmetric=True)
        B = handle_rhs(coords, max(n_cols, 2), seed=11)
        refs = []
        for j in range(B.shape[1]):
            sy = kr.System(rp, ci, vals, B[:, j])
            refs.append((sy, kr.cg_iterates(sy, None, max(K_CG))))
        max_len = int(np.diff(rp).max())
        sym = knobs.get("persist_sym", 0) == 1
        name = f"handle {hname} {form}"
        starts = np.concatenate([[0], np.cumsum(groups)])

        def call_iters(ks):   # info.iters of one call whose column j ran ks[j] iterations
            return sum(max(ks[a:b]) for a, b in zip(starts[:-1], starts[1:]))

        def check_form(info):
            lay = c.solver_layout_kind(False)
            assert info.method_used == capi.SOLVER_CG_FUSED
            if "persist" in knobs:
                assert info.persistent == 0
            else:
                assert info.persistent == 1 and lay["sym"] == (1 if sym else 0), lay
            if form.startswith("direct"):
                assert lay["workgroups"] == 1 and info.t_solve_ms == 0.0, "the direct launch reports no stream time: the general path does"
            if form.startswith("general"):
                assert lay["workgroups"] == 1 and info.t_solve_ms > 0.0

        # one-column forms: a smooth and a unit-vector right-hand side, one call each
        calls = [(B, refs)] if n_cols > 1 else [(B[:, 0], refs[:1]), (B[:, 1], refs[1:2])]
        for b, mine in calls:
            for k in K_CG:
                X, info = c.lin_solve(b, method=capi.SOLVER_CG_FUSED, rtol=1e-30, maxit=k, raise_on_noconv=False)
                assert info.converged == 0 and info.iters == call_iters([k] * len(mine)), (info.converged, info.iters)
                check_form(info)
                X = X.reshape(X.shape[0], -1)
                for j, (sy, its) in enumerate(mine):
                    _check_iterate(name, "cg", sy, its, k, X[:, j], sym, max_len)
                wsy, wits = max(mine, key=lambda m_: m_[1][k - 1].rho)   # (relres of a call: its worst column)
                _check_relres(name, "cg", wits, k, info.relres, wsy if sym else None, max_len)
            # the stop test: ONE tolerance between two residual ratios of every column of the call (tests/test_krylov_ref_cpu.py checks that there is
            # one).  Every column must stop at its OWN iteration k_j and hand out its own k_j-th iterate -- a column that has finished is frozen while
            # the others of its launch or batch go on -- and the call reports the worst column's residual
            if len(mine) == 1:
                k, rtol = pick_stop([it.rho for it in mine[0][1]], max(K_CG))
                ks = [k]
            else:
                rtol, ks, margin = pick_stop_columns([[it.rho for it in its] for _, its in mine], max(K_CG))
                if sym:   # (what the fixed-point accumulators may move a residual by is far inside the margin as well)
                    assert max(kr.symmetric_storage_residual_slack(sy, its, k, max_len) for (sy, its), k in zip(mine, ks)) <= 1e-3 * (margin - 1.0) * rtol
            X, info = c.lin_solve(b, method=capi.SOLVER_CG_FUSED, rtol=rtol)
            assert info.converged == 1 and info.iters == call_iters(ks), (info.iters, ks, rtol)
            check_form(info)
            X = X.reshape(X.shape[0], -1)
            for j, ((sy, its), k) in enumerate(zip(mine, ks)):
                _check_iterate(name, "cg", sy, its, k, X[:, j], sym, max_len, tag=f"stop@{min(ks)}..{max(ks)}" if len(ks) > 1 else f"stop@{k}")
            (wsy, wits), wk = max(zip(mine, ks), key=lambda m_: m_[0][1][m_[1] - 1].rho)
            _check_relres(name, "cg", wits, wk, info.relres, wsy if sym else None, max_len)
    finally:
        c.close()


# ---- a junction of 2 000 arms under the symmetric storage ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rhs", RHS)
def test_star_network_symmetric_storage(env, rhs):
    """the longest row there is against the fixed-point scale: max_len = 2 001 enters the accumulator's quantum, so this is what the symmetric form's accuracy
    really is on a junction; the share of the documented bound it uses is recorded (profiles/krylov_iterates.txt)"""
    capi, _ = env
    _run_solve_form(env, "star", rhs, dict(persist_sym=1), capi.SOLVER_CG_FUSED, _expect_layout(dict(sym=1), True), "k_cg_persist star-2000 persist_sym1")
