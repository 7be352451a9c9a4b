"""The 2 x 2 block handle's two Krylov stages at the k-th iterate, against the extended-precision reference of tests/block_iter_ref.py.

`rtol = 1e-30, maxit = k` stops a solve after exactly k iterations and hands the iterate out.  A flexible outer iteration controlled by its true residual
corrects its preconditioner's mistakes, so a converged answer says little about the cycle; the k-th iterate says everything: with the aggregates fixed
it is ONE vector in exact arithmetic.

FDAPDE_SOLVER_BLOCK_AMG (csrc/eng_block_amg.hip, the k_bamg_* kernels).  After the first solve the device's own hierarchy is read back --
fdapde_amg_hierarchy and every level's fdapde_amg_aggregates -- and the reference hierarchy is built from the caller's blocks and those maps; its rows
and entries must be the device's on every level.  Per field (f: the first block row, g: the second; lambda scales them differently, and the coarse solve
spreads its rounding over the whole domain)

    max |x_gpu - x_ref| <= c_amg(k) u max s,        u = 2^-53,  s = sum_j |y_j| |z_j| entrywise,
    |info.relres - rho_k| <= c_amg(k) u || |A| s || / ||b||, and info.relres within 1e-12 relative of the residual of the vector handed out.

The handle's GMRES stage (block_gmres, the k_gm_* kernels on D^-1 A): entrywise |x_gpu - x_ref|_i <= c_gm(k) u s_i, s = sum_j |y_j| |v_j|, exactly 0 where
s_i = 0 (the Krylov front has not arrived), and relres against rho_k of the scaled system in the same form.  The same with fdapde_block_set_obs's term
live (an areal and a pointwise Psi, each under block_obs_team = 8 and = 64 against one reference; constants of their own by the same rule).

c(k) = 4 r_cpu(k) rounded up to a power of two, r_cpu the worst ratio of the float64 numpy checkers of the same schemes against the reference on the same
cases (tests/test_block_iter_cpu.py measures it on the oracle's matrices and fails if it no longer fits or exceeds 2^12; profiles/block_iterates.txt).

FDAPDE_BLOCK_ITER_PROFILE=<path> appends the worst ratio per case and k."""
import ctypes as C
import os

import numpy as np
import pytest

import block_iter_ref as ir
import block_ref as br

pytestmark = pytest.mark.gpu
U = ir.U


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, meshgen


_live = {}      # (system, knobs) -> dict of the context and what was built on it
_worst = {}     # line -> {k: ratio}


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _live.values():
        s["c"].close()
    _live.clear()
    path = os.environ.get("FDAPDE_BLOCK_ITER_PROFILE")
    if path and _worst:
        with open(path, "a") as fh:
            for line in sorted(_worst):
                fh.write(f"gpu {line}: " + " ".join(f"{k}={v:.3g}" for k, v in sorted(_worst[line].items())) + "\n")


def _note(line, k, value):
    d = _worst.setdefault(line, {})
    d[k] = max(d.get(k, 0.0), value)


def _context(env, system, knobs):
    """one context per (system, knobs), its block handle computed from the device's own stiff / mass matrices"""
    capi, meshgen = env
    key = (system, tuple(sorted(knobs.items())))
    if key not in _live:
        mesh, order, lam, advection = ir.AMG_CASES[system][:4]
        nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
        c = capi.Context(0)
        c.mesh_upload(nodes, cells, bnd)
        nd = c.dofs_build(order)
        c.tune("amg_coarse_rows", ir.AMG_COARSE_ROWS)
        c.tune("amg_setup_check", 1)
        for k_, v_ in knobs.items():
            c.tune(k_, v_)
        op = -capi.laplacian()
        if advection:
            op = op + capi.advection([4.0, -2.0] if nodes.shape[1] == 2 else [4.0, -2.0, 1.0])
        c.set_operator(op)
        c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
        c.init()
        rp, ci = c.pattern_get()
        rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
        obs = br.observed_nodes(nodes.shape[0])
        blocks = br.smoothing_blocks(rp, ci, c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS), obs, lam, nd)
        c.block_compute(*blocks, symmetric=not advection)
        _live[key] = dict(c=c, rp=rp, ci=ci, blocks=blocks, n=nd, b=br.smoothing_rhs(obs, lam, nd), restart=knobs.get("gmres_m", 50),
                          A=ir.BlockCsr(rp, ci, np.stack(blocks, axis=1), ir.LD))
    return _live[key]


def _solve(env, s, b, method, k):
    capi = env[0]
    x, info = s["c"].block_solve(b, method=method, rtol=1e-30, maxit=k, raise_on_noconv=False)
    assert info.iters == k and info.converged == 0 and info.method_used == method, (info.iters, info.converged, info.method_used)
    assert np.all(np.isfinite(x))
    return x, info


def _multilevel(env, name):
    """the case's context after its first multilevel solve, with the device's hierarchy read back and the reference built on it"""
    capi = env[0]
    system_knobs = ir.AMG_CASES[name][4]
    s = _context(env, name, system_knobs)
    if "H" not in s:
        c = s["c"]
        _solve(env, s, s["b"], capi.SOLVER_BLOCK_AMG, 1)
        h = c.amg_hierarchy(capi.AMG_OF_BLOCK)
        levels = len(h["rows"])
        aggs = [c.amg_aggregates(capi.AMG_OF_BLOCK, l) for l in range(levels - 1)]
        for l, agg in enumerate(aggs):
            assert agg.dtype == np.int32 and agg.shape == (h["rows"][l] // 2,)
            assert agg.min() == 0 and agg.max() == h["rows"][l + 1] // 2 - 1 and len(np.unique(agg)) == h["rows"][l + 1] // 2, "a map onto the next level's rows"
        H = ir.Hierarchy(s["rp"], s["ci"], s["blocks"], s["n"], aggs)
        # preconditions of the comparison: the reference's levels are the device's
        assert [2 * r for r in H.rows] == h["rows"], (H.rows, h["rows"])
        assert [4 * e for e in H.entries] == h["nnz"], (H.entries, h["nnz"])
        s["h"], s["aggs"], s["H"] = h, aggs, H
        print(f"case {name}: rows per level {h['rows']}, absorbed {h['absorbed']}")
    return s


def _teams(h):
    """the lane count of every level that has a next one, as level_vectors computes it: entries per row <= 12 -> 8, else 16"""
    return [8 if (nnz / 4) / (rows / 2) <= 12.0 else 16 for rows, nnz in zip(h["rows"][:-1], h["nnz"][:-1])]


def _residual(s, x, b):
    r = ir.interleave(b).astype(ir.LD) - s["A"].mv(ir.interleave(x).astype(ir.LD))
    bl = np.asarray(b, dtype=ir.LD)
    return float(np.sqrt(r @ r) / np.sqrt(bl @ bl))


@pytest.mark.parametrize("name", list(ir.AMG_CASES))
def test_multilevel_iterates(env, name):
    capi = env[0]
    ks = ir.AMG_CASES[name][5]
    s = _multilevel(env, name)
    h = s["h"]
    if name in "abcdef":
        assert len(h["rows"]) >= 3, "a level with GCR steps"
    if name == "b":
        assert len(h["rows"]) >= 5, "GCR nested three deep"
    if name == "d":
        assert _teams(h)[0] == 16 and int(np.diff(s["rp"]).max()) > 16, "rows of more than 16 entries: two passes of a 16-lane team"
    if name == "e":
        assert h["absorbed"] == 1 and max(int(np.bincount(a).max()) for a in s["aggs"]) > 4, "some aggregate has more than four members"
    if name == "g":
        assert len(h["rows"]) == 2, "the correction is the dense level alone"
    its = ir.fgmres_iterates(s["H"], s["b"], max(ks), s["restart"])
    if name == "h":
        assert s["restart"] == 3 and max(ks) > 3, "the outer iteration restarts from its true residual inside the run"
    bad = []
    for k in ks:
        x, info = _solve(env, s, s["b"], capi.SOLVER_BLOCK_AMG, k)
        assert s["c"].amg_hierarchy(capi.AMG_OF_BLOCK) == h, "the hierarchy of the first solve serves every later one"
        ref = its[k - 1]
        ratios = ir.field_ratios(x, ref)
        rr = ir.relres_ratio(info.relres, ref)
        res = _residual(s, x, s["b"])
        _note(f"block_amg {name}", k, max(ratios))
        _note(f"block_amg {name} [relres]", k, rr)
        print(f"block_amg {name} k={k}: worst |err| / (u max s) per field = {ratios[0]:.3g} / {ratios[1]:.3g}, relres {rr:.3g} (c = {ir.C_AMG[k]:g}), "
              f"relres {info.relres:.3e} against the residual of the vector handed out: {abs(info.relres - res) / res:.1e} relative")
        if not max(ratios) <= ir.C_AMG[k]:
            bad.append((k, "iterate", max(ratios) / ir.C_AMG[k]))
        if not rr <= ir.C_AMG[k]:
            bad.append((k, "relres", rr / ir.C_AMG[k]))
        if not abs(info.relres - res) <= 1e-12 * res:
            bad.append((k, "relres is not the residual of the vector handed out", info.relres, res))
    assert not bad, (name, "(k, what, times the bound)", bad)   # (every k is run and printed before the verdict)


def test_both_lane_widths_and_three_levels(env):
    """over the whole case list: both team widths occur on a level with a next one, and cases a .. f have at least three levels"""
    teams = set()
    for name in ir.AMG_CASES:
        h = _multilevel(env, name)["h"]
        teams.update(_teams(h))
        if name in "abcdef":
            assert len(h["rows"]) >= 3, (name, h["rows"])
    assert teams == {8, 16}, teams


@pytest.mark.parametrize("name", list(ir.GMRES_CASES))
def test_gmres_stage_iterates(env, name):
    capi = env[0]
    system, knobs, rhs, ks = ir.GMRES_CASES[name]
    s = _context(env, system, knobs)
    b = s["b"] if rhs == "smoothing" else ir.unit_rhs(s["n"], ir.interior_dof(s["rp"], s["n"]))
    its = ir.gmres_iterates(s["rp"], s["ci"], s["blocks"], s["n"], b, max(ks), s["restart"])
    if knobs.get("gmres_m"):
        assert max(ks) > knobs["gmres_m"], "the cycle restarts inside the run"
    bad = []
    for k in ks:
        x, info = _solve(env, s, b, capi.SOLVER_GMRES, k)
        ref = its[k - 1]
        dead = ref.s == 0
        if rhs == "unit":
            assert dead.any(), "the front has not reached every entry"
        assert not x[dead].any(), f"{name} k={k}: entries the Krylov front has not reached must be exactly 0 ({int((x[dead] != 0).sum())} are not)"
        ratio = ir.entry_ratio(x, ref)
        rr = ir.relres_ratio(info.relres, ref)
        _note(f"gmres {name}", k, ratio)
        _note(f"gmres {name} [relres]", k, rr)
        print(f"gmres {name} k={k}: worst |err| / (u s) = {ratio:.3g}, relres {rr:.3g} (c = {ir.C_GMRES[k]:g}), {int(dead.sum())} dead entries")
        err = np.abs(x.astype(ir.LD) - ref.x)
        if (err > ir.C_GMRES[k] * U * ref.s).any():
            bad.append((k, "iterate", ratio / ir.C_GMRES[k]))
        if not rr <= ir.C_GMRES[k]:
            bad.append((k, "relres", rr / ir.C_GMRES[k]))
    assert not bad, (name, "(k, what, times the bound)", bad)   # (every k is run and printed before the verdict)


@pytest.mark.parametrize("team", ir.OBS_TEAMS)
@pytest.mark.parametrize("name", list(ir.GMRES_OBS_CASES))
def test_gmres_stage_iterates_with_a_factored_term(env, oracle, name, team):
    """the stage with fdapde_block_set_obs's term live (k_obs_gather / k_obs_scatter behind k_block_spmv, the term's share in D^-1): the same bounds, with
    constants of their own by the same rule, under both team widths against ONE reference"""
    import block_obs_ref as bo
    import kron_obs_ref as ko

    capi, meshgen = env
    system, design, ks = ir.GMRES_OBS_CASES[name]
    mesh, order, lam, advection = ir.AMG_CASES[system][:4]
    s = _context(env, system, dict(block_obs_team=team))
    c, nd = s["c"], s["n"]
    nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
    om = oracle.Mesh(np.ascontiguousarray(nodes, dtype=float), np.ascontiguousarray(cells, dtype=np.int32), np.ascontiguousarray(bnd, dtype=np.uint8))
    dofs, _, ond, _ = oracle.enumerate_dofs(om, order)
    assert ond == nd and np.array_equal(c.dofs_get()[0], dofs), "the oracle and the library number the DOFs alike"
    Psi = ko.design_psi(oracle, om, None, order, dofs, nd, design)
    rows = np.diff(Psi.indptr)
    assert (rows.max() > 64) if name == "a-areal" else (rows.max() <= 3), "an areal row is longer than a team of 64; a pointwise row holds one cell's DOFs"
    blocks = bo.smoothing_blocks(s["rp"], s["ci"], c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS), lam, nd)
    b = bo.smoothing_rhs(Psi, lam, nd)
    c.block_compute(*blocks, symmetric=True)   # (the context is this test's own: block_obs_team is part of its key)
    c.block_set_obs(Psi, weights=None, scale=-1.0)
    info = c.block_obs_info()
    assert info["team_rows"] == team and info["team_cols"] == team and info["nnz"] == Psi.nnz, "the team width under test"
    its = ir.gmres_iterates(s["rp"], s["ci"], blocks, nd, b, max(ks), obs=(Psi, None, -1.0))
    bad = []
    for k in ks:
        x, inf = _solve(env, s, b, capi.SOLVER_GMRES, k)
        ref = its[k - 1]
        assert not x[ref.s == 0].any()
        ratio, rr = ir.entry_ratio(x, ref), ir.relres_ratio(inf.relres, ref)
        _note(f"gmres_obs {name} team {team}", k, ratio)
        _note(f"gmres_obs {name} team {team} [relres]", k, rr)
        print(f"gmres_obs {name} team {team} k={k}: worst |err| / (u s) = {ratio:.3g}, relres {rr:.3g} (c = {ir.C_GMRES_OBS[k]:g})")
        if (np.abs(x.astype(ir.LD) - ref.x) > ir.C_GMRES_OBS[k] * U * ref.s).any():
            bad.append((k, "iterate", ratio / ir.C_GMRES_OBS[k]))
        if not rr <= ir.C_GMRES_OBS[k]:
            bad.append((k, "relres", rr / ir.C_GMRES_OBS[k]))
    assert not bad, (name, team, "(k, what, times the bound)", bad)   # (every k is run and printed before the verdict)


def test_the_getter_refuses_what_it_cannot_answer(env):
    capi, meshgen = env
    never = _context(env, "a", dict(amg_coarse_rows=32))   # (a context of its own: its block handle is computed, no multilevel solve has run)
    _solve(env, never, never["b"], capi.SOLVER_GMRES, 1)
    for call in (lambda: never["c"].amg_aggregates(capi.AMG_OF_BLOCK, 0), lambda: never["c"].amg_hierarchy(capi.AMG_OF_BLOCK)):
        with pytest.raises(capi.FdapdeError) as e:
            call()
        assert e.value.status == capi.ENOTINIT, "no hierarchy before the first multilevel solve"
    s = _multilevel(env, "g")
    c, levels, n0 = s["c"], len(s["h"]["rows"]), s["n"]
    for which in (capi.AMG_OF_SOLVE, capi.AMG_OF_HANDLE):   # (a context with a block hierarchy only: the scalar ones are not live)
        for call in (lambda: c.amg_aggregates(which, 0), lambda: c.amg_damping(which)):
            with pytest.raises(capi.FdapdeError) as e:
                call()
            assert e.value.status == capi.ENOTINIT
    om = c.amg_damping(capi.AMG_OF_BLOCK)
    assert om.shape == (levels,) and (om[:-1] == ir.OMEGA).all() and om[-1] == 0.0, "0.7 on every level that has a next one"
    assert np.array_equal(np.sort(c.amg_order(capi.AMG_OF_BLOCK)), np.arange(n0)), "level 0's block rows are the DOFs, each once"
    for level in (-1, levels - 1, levels):   # (the last level has no next one)
        with pytest.raises(capi.FdapdeError) as e:
            c.amg_aggregates(capi.AMG_OF_BLOCK, level)
        assert e.value.status == capi.EINVAL
    buf = np.full(n0, -7, dtype=np.int32)
    rows = C.c_int64(-1)
    rc = c.lib.fdapde_amg_aggregates(c._ctx, 2, 0, C.c_int64(n0 - 1), buf.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rows))
    assert rc == capi.EINVAL and rows.value == n0 and (buf == -7).all(), "a buffer one entry short is refused untouched"
    assert c.lib.fdapde_amg_aggregates(c._ctx, 3, 0, C.c_int64(n0), buf.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rows)) == capi.EINVAL
    assert c.lib.fdapde_amg_aggregates(c._ctx, 2, 0, C.c_int64(n0), buf.ctypes.data_as(C.POINTER(C.c_int32)), None) == capi.OK
    assert np.array_equal(buf, s["aggs"][0])
    # the same calls succeed once a scalar solve has run on that context: the factor-once handle's hierarchy (which = 1) of stiffness + mass
    c.lin_compute(values=c.matrix_values(capi.MAT_STIFF) + c.matrix_values(capi.MAT_MASS), symmetric=True)
    _, info = c.lin_solve(np.ones(n0), method=capi.SOLVER_AMG, rtol=1e-10)
    assert info.converged == 1 and info.method_used == capi.SOLVER_AMG
    hs = c.amg_hierarchy(capi.AMG_OF_HANDLE)
    assert len(hs["rows"]) >= 2 and hs["rows"][0] == n0
    agg, om = c.amg_aggregates(capi.AMG_OF_HANDLE, 0), c.amg_damping(capi.AMG_OF_HANDLE)
    assert agg.shape == (n0,) and agg.min() == 0 and agg.max() == hs["rows"][1] - 1 and len(np.unique(agg)) == hs["rows"][1]
    assert om.shape == (len(hs["rows"]),) and (om[:-1] > 0.0).all() and om[-1] == 0.0
    with pytest.raises(capi.FdapdeError) as e:
        c.amg_aggregates(capi.AMG_OF_SOLVE, 0)
    assert e.value.status == capi.ENOTINIT, "fdapde_solve's is still not live"
    assert np.array_equal(c.amg_aggregates(capi.AMG_OF_BLOCK, 0), s["aggs"][0]) and c.amg_hierarchy(capi.AMG_OF_BLOCK) == s["h"], "the block hierarchy stays"
    m = capi.Context(devices=[0, 0])
    assert m.lib.fdapde_amg_aggregates(m._ctx, 2, 0, C.c_int64(n0), buf.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rows)) == capi.EUNSUPPORTED
    assert m.lib.fdapde_amg_aggregates(m._ctx, 0, 0, C.c_int64(n0), buf.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rows)) == capi.EUNSUPPORTED
    m.close()
