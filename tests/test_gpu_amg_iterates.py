"""FDAPDE_SOLVER_AMG (csrc/eng_amg.hip) at the k-th iterate, against the extended-precision reference of tests/amg_iter_ref.py.

`rtol = 1e-30, maxit = k` stops a solve after exactly k iterations and hands the iterate out.  The outer iteration is flexible GMRES controlled by its true
residual, so a converged answer says little about the cycle, and the column-by-column comparison of tests/test_gpu_amg_cols.py holds a kernel to itself at
another width; the k-th iterate against an independent restatement says everything: with the aggregates and the damping fixed it is ONE vector in exact
arithmetic.

After the first solve the device's own hierarchy is read back -- fdapde_amg_hierarchy, every level's fdapde_amg_aggregates, fdapde_amg_damping and fdapde_amg_order -- and the
reference is built from the caller's matrix on those maps and that damping; its rows and entries must be the device's on every level, and every omega within
OMEGA_RTOL of the np.longdouble restatement of level_prepare's estimator.  Then, per case and k, with u = 2^-53 and s = sum_j |y_j| |z_j| entrywise,

    max |x_gpu - x_ref| <= c(k) u max s over the free entries,   |info.relres - rho_k| <= c(k) u || |K| s || / ||r_lift||,

and info.relres within 1e-12 relative of the extended-precision residual of the vector handed out.  c(k) = 4 r_cpu(k) rounded up to a power of two, r_cpu the
worst ratio of the float64 numpy checker of the same scheme against the reference on the same cases (tests/test_amg_iter_cpu.py measures it on the oracle's
matrices and fails if it no longer fits or exceeds 2^12; profiles/amg_iterates.txt).

The cases (amg_iter_ref.AMG_CASES; `amg_coarse_rows` = 64, `amg_setup_check` = 1): a 2-D P1 through fdapde_solve with Dirichlet data, b the same operator
through the handle with five levels, c advection through fdapde_solve (GCR steps), d 3-D P1 with absorption, e 2-D P2, f the dense level alone, h 3-D P2
(16-lane teams); g: b and d at `amg_cols` = 8, every column against its own reference.

FDAPDE_AMG_ITER_PROFILE=<path> appends the worst ratio per case and k."""
import os

import numpy as np
import pytest

import amg_iter_ref as ir

pytestmark = pytest.mark.gpu
U = ir.U


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, meshgen


_live = {}      # case -> dict of the context and what was built on it
_worst = {}     # line -> {k: ratio}


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _live.values():
        s["c"].close()
    _live.clear()
    path = os.environ.get("FDAPDE_AMG_ITER_PROFILE")
    if path and _worst:
        with open(path, "a") as fh:
            for line in sorted(_worst):
                fh.write(f"gpu {line}: " + " ".join(f"{k}={v:.3g}" for k, v in sorted(_worst[line].items())) + "\n")


def _note(line, k, value):
    d = _worst.setdefault(line, {})
    d[k] = max(d.get(k, 0.0), value)


def _context(env, name):
    """one context per case: the system in the caller's numbering as K u = rhs from `lift`, read before any solve"""
    capi, meshgen = env
    if name not in _live:
        mesh, order, kind, path, knobs = ir.AMG_CASES[name][:5]
        nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
        c = capi.Context(0)
        c.mesh_upload(nodes, cells, bnd)
        nd = c.dofs_build(order)
        c.tune("amg_coarse_rows", ir.AMG_COARSE_ROWS)
        c.tune("amg_setup_check", 1)
        for k_, v_ in knobs.items():
            c.tune(k_, v_)
        _, bd, coords = c.dofs_get()
        bd = np.asarray(bd, dtype=bool)
        op = -capi.laplacian() + capi.reaction(2.0) if kind == "reaction" else -capi.laplacian() + capi.advection(ir.ADVECTION) + capi.reaction(1.0)
        c.set_operator(op)
        c.set_forcing(ir.forcing(c.quadrature_nodes()))
        g = ir.dirichlet_data(coords)
        if path == "solve":
            c.set_dirichlet(g)
        c.init()
        rp, ci = c.pattern_get()
        rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
        a = c.matrix_values(capi.MAT_STIFF)
        sym = kind == "reaction"
        if path == "solve":
            K = ir.unit_rows(rp, ci, a, bd)
            rhs, lift, which = np.where(bd, g, c.force()), np.where(bd, g, 0.0), capi.AMG_OF_SOLVE
        else:
            K, bd = a, np.zeros(nd, dtype=bool)
            c.lin_compute(values=a, symmetric=sym)
            rhs, lift, which = ir.Csr(rp, ci, a, np.float64).mv(np.prod(np.cos(np.pi * coords), axis=1)), None, capi.AMG_OF_HANDLE
        _live[name] = dict(c=c, rp=rp, ci=ci, K=K, n=nd, rhs=rhs, lift=lift, bnd=bd, free=~bd, g=g, coords=coords, sym=sym, path=path, which=which,
                           A=ir.Csr(rp, ci, K, ir.LD))
    return _live[name]


def _solve(env, s, k, rhs=None):
    """-> (x, info) of the solve stopped at iteration k; rhs: other columns for the handle"""
    capi = env[0]
    if s["path"] == "solve":
        info = s["c"].solve(method=capi.SOLVER_AMG, rtol=1e-30, maxit=k, raise_on_noconv=False)
        x = s["c"].solution()
    else:
        x, info = s["c"].lin_solve(s["rhs"] if rhs is None else rhs, method=capi.SOLVER_AMG, rtol=1e-30, maxit=k, raise_on_noconv=False)
    assert info.method_used == capi.SOLVER_AMG and np.all(np.isfinite(x))
    return x, info


def _read_back(s):
    c, which = s["c"], s["which"]
    h = c.amg_hierarchy(which)
    return h, [c.amg_aggregates(which, l) for l in range(len(h["rows"]) - 1)], c.amg_damping(which)


def _multilevel(env, name):
    """the case's context after its first solve, with the device's hierarchy read back and the reference built on it"""
    s = _context(env, name)
    if "H" not in s:
        _solve(env, s, 1)
        h, aggs, om = _read_back(s)
        levels = len(h["rows"])
        assert om.dtype == np.float64 and om.shape == (levels,) and om[-1] == 0.0 and (om[:-1] > 0.0).all(), om
        for l, agg in enumerate(aggs):
            assert agg.dtype == np.int32 and agg.shape == (h["rows"][l],)
            used = agg[agg >= 0]
            assert agg.min() >= -1 and used.max() == h["rows"][l + 1] - 1 and len(np.unique(used)) == h["rows"][l + 1], "a map onto the next level's rows"
            assert np.array_equal(agg < 0, s["bnd"] if l == 0 else np.zeros(len(agg), dtype=bool)), "a row of no aggregate is a Dirichlet row of level 0"
        H = ir.Hierarchy(s["rp"], s["ci"], s["K"], aggs, om[:-1], s["sym"])
        # preconditions of the comparison: the reference's levels are the device's, and its damping the restated estimator's
        assert H.rows == h["rows"], (H.rows, h["rows"])
        assert H.entries[1:] == h["nnz"][1:] and len(s["ci"]) == h["nnz"][0], (H.entries, h["nnz"])
        order = s["c"].amg_order(s["which"])
        assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(s["n"])), "level 0's rows are the DOFs, each once"
        est = H.estimated_damping(order)
        rel = [abs(float((ir.LD(float(w)) - e) / e)) for w, e in zip(om[:-1], est)]
        s.update(h=h, aggs=aggs, om=om, H=H, teams=ir.teams(h["rows"], h["nnz"]), om_rel=rel)
        print(f"case {name}: rows per level {h['rows']}, teams {s['teams']}, absorbed {h['absorbed']}, omega {[float(w) for w in om]}, "
              f"relative to the restated estimator {['%.1e' % r for r in rel]} (bound {ir.OMEGA_RTOL:.1e})")
        if rel:
            _note(f"omega {name}", 0, max(rel))
    return s


def _residual(s, x, rhs, lift):
    """the extended-precision residual of x relative to the lift's, and the float64 evaluation's own share of it: (row length + 2) u (|rhs| + |K| |x|) entrywise"""
    b, xl = np.asarray(rhs, dtype=float).astype(ir.LD), np.asarray(x, dtype=float).astype(ir.LD)
    r = b - s["A"].mv(xl)
    r0 = b if lift is None else b - s["A"].mv(np.asarray(lift, dtype=float).astype(ir.LD))
    e = np.abs(b) + s["A"].amv(xl)
    return float(np.sqrt(r @ r) / np.sqrt(r0 @ r0)), float((int(np.diff(s["rp"]).max()) + 2) * U * np.sqrt(e @ e) / np.sqrt(r0 @ r0))


def _unchanged(s):
    h, aggs, om = _read_back(s)
    return h == s["h"] and all(np.array_equal(a, b) for a, b in zip(aggs, s["aggs"])) and np.array_equal(om, s["om"])


@pytest.mark.parametrize("name", list(ir.AMG_CASES))
def test_hierarchy_is_the_reference_s_and_the_damping_the_estimator_s(env, name):
    s = _multilevel(env, name)
    h, teams = s["h"], s["teams"]
    assert all(r <= ir.OMEGA_RTOL for r in s["om_rel"]), (name, "omega per level relative to the restated estimator", s["om_rel"], ir.OMEGA_RTOL)
    if name in "ace":
        assert len(h["rows"]) >= 3, h["rows"]
    if name == "a":
        assert teams[0] == 4 and s["bnd"].any() and np.array_equal(s["aggs"][0] == -1, s["bnd"]), "agg == -1 exactly on the Dirichlet DOFs"
    if name == "b":
        assert len(h["rows"]) >= 5 and s["sym"], "flexible CG nested three deep"
    if name == "c":
        A1 = s["H"].A[1].dense()
        assert not s["sym"] and np.abs(A1 - A1.T).max() > 1e-6 * np.abs(A1).max(), "GCR steps on a non-symmetric Galerkin chain"
    if name == "d":
        assert h["absorbed"] == 1 and max(int(np.bincount(a).max()) for a in s["aggs"]) > 4 and teams[0] == 8, (h, teams)
    if name == "e":
        length = np.diff(s["rp"])[s["free"]]
        passes = -(-length // teams[0])   # (2-D P2: 9 entries on an edge DOF's row, 19 on a vertex's, 8 lanes)
        assert length.max() > teams[0] and passes.min() < passes.max(), "rows longer than one team pass, long and short rows (other pass counts) on one level"
    if name == "f":
        assert len(h["rows"]) == 1 and s["bnd"].any(), "the dense level alone, with its boundary mask"
    if name == "h":
        assert teams[0] == 16, teams


def test_every_team_width_has_a_level(env):
    """over the whole case list: team widths 4, 8 and 16 each occur on a level with a next one"""
    assert {t for name in ir.AMG_CASES for t in _multilevel(env, name)["teams"]} == {4, 8, 16}


@pytest.mark.parametrize("name", list(ir.AMG_CASES))
def test_iterates(env, name):
    ks = ir.AMG_CASES[name][5]
    s = _multilevel(env, name)
    one_level = len(s["h"]["rows"]) == 1
    its = ir.iterates(s["H"], s["rhs"], max(ks), s["lift"])
    bad = []
    for k in ks:
        x, info = _solve(env, s, k)
        assert _unchanged(s), "the hierarchy of the first solve serves every later one"
        if one_level:   # (the preconditioner is the inverse: the Krylov space may be exhausted at once)
            assert info.iters <= 1
            if info.iters == 0:
                assert np.array_equal(x, s["lift"])
                continue
        else:
            assert info.iters == k and info.converged == 0, (info.iters, info.converged)
        ref = its[k - 1]
        if s["path"] == "solve" and not one_level:
            assert np.array_equal(x[s["bnd"]], s["g"][s["bnd"]]), "the boundary entries of the iterate are the data, exactly"
        ratio = ir.iterate_ratio(x, ref, s["free"])
        rr = ir.relres_ratio(info.relres, ref)
        res, rounding = _residual(s, x, s["rhs"], s["lift"])
        # the residual of the vector handed out.  On the dense level alone it is a rounding of x, of the size of what its float64 evaluation on the device
        # carries itself: that floor is added there, and only there
        floor = rounding if one_level else 0.0
        _note(f"amg {name}", k, ratio)
        _note(f"amg {name} [relres]", k, rr)
        print(f"amg {name} k={k}: worst |err| / (u max s) = {ratio:.3g}, relres {rr:.3g} (c = {ir.C_AMG[k]:g}), relres {info.relres:.3e} against the residual "
              f"of the vector handed out: {abs(info.relres - res) / res:.1e} relative")
        if not ratio <= ir.C_AMG[k]:
            bad.append((k, "iterate", ratio / ir.C_AMG[k]))
        if not rr <= ir.C_AMG[k]:
            bad.append((k, "relres", rr / ir.C_AMG[k]))
        if not abs(info.relres - res) <= 1e-12 * res + floor:
            bad.append((k, "relres is not the residual of the vector handed out", info.relres, res))
    assert not bad, (name, "(k, what, times the bound)", bad)   # (every k is run and printed before the verdict)


@pytest.mark.parametrize("name", list(ir.COLS_CASES))
def test_columns_side_by_side(env, name):
    """case g: eight columns at `amg_cols` = 8 -- smooth, a unit vector, zeros, one scaled by 1e-150, four random --, every column against the reference of
    THAT column, not against the one-column run; info carries the summed iterations and the worst relres"""
    capi = env[0]
    s = _multilevel(env, name)
    c = s["c"]
    B = ir.columns(ir.Csr(s["rp"], s["ci"], s["K"], np.float64).mv, s["coords"], np.arange(s["n"]), s["n"])
    live = [j for j in range(B.shape[1]) if B[:, j].any()]
    assert len(live) == 7 and not B[:, 2].any()
    ks = ir.COLS_CASES[name]
    refs = {j: ir.iterates(s["H"], B[:, j], max(ks)) for j in live}
    c.tune("amg_cols", 8)
    bad = []
    for k in ks:
        t0 = c.amg_cols_trace(capi.AMG_OF_HANDLE)
        X, info = _solve(env, s, k, rhs=B)
        t1 = c.amg_cols_trace(capi.AMG_OF_HANDLE)
        assert {key: t1[key] - t0[key] for key in t0} == dict(batches=1, batched_cols=8, single_cols=0), (t0, t1)
        assert _unchanged(s), "the hierarchy of the first solve serves every later one"
        assert info.iters == k * len(live) and info.converged == 0, (info.iters, info.converged)   # (the zero column takes no iteration)
        assert not X[:, 2].any(), "the zero column is exactly zero"
        worst_res = 0.0
        for j in live:
            ref = refs[j][k - 1]
            ratio = ir.iterate_ratio(X[:, j], ref, s["free"])
            worst_res = max(worst_res, _residual(s, X[:, j], B[:, j], None)[0])
            _note(f"amg {name} cols", k, ratio)
            print(f"amg {name} amg_cols 8 k={k} column {j}: worst |err| / (u max s) = {ratio:.3g} (c = {ir.C_AMG[k]:g})")
            if not ratio <= ir.C_AMG[k]:
                bad.append((k, j, "iterate", ratio / ir.C_AMG[k]))
        # info.relres is the worst column's: |max a - max b| <= max |a - b|, every column's own bound at most the largest one
        rho, scale = max(refs[j][k - 1].rho for j in live), max(refs[j][k - 1].res_scale for j in live)
        rr = abs(info.relres - rho) / (U * scale)
        _note(f"amg {name} cols [relres]", k, rr)
        print(f"amg {name} amg_cols 8 k={k}: relres {rr:.3g} (c = {ir.C_AMG[k]:g}), against the worst residual of the vectors handed out: "
              f"{abs(info.relres - worst_res) / worst_res:.1e} relative")
        if not rr <= ir.C_AMG[k]:
            bad.append((k, "relres", rr / ir.C_AMG[k]))
        if not abs(info.relres - worst_res) <= 1e-12 * worst_res:
            bad.append((k, "relres is not the worst residual of the vectors handed out", info.relres, worst_res))
    assert not bad, (name, "(k, column, what, times the bound)", bad)


def test_the_getters_answer_for_live_hierarchies_only(env):
    """fdapde_amg_aggregates / fdapde_amg_damping: FDAPDE_ENOTINIT before the first multilevel solve, for the other scalar hierarchy, and for a handle
    hierarchy fdapde_lin_compute has outlived; FDAPDE_EINVAL for a level without a next one, a short buffer, a fourth kind"""
    import ctypes as C

    capi = env[0]
    s = _multilevel(env, "a")
    c, levels, n0 = s["c"], len(s["h"]["rows"]), s["n"]
    for call in (lambda: c.amg_aggregates(capi.AMG_OF_HANDLE, 0), lambda: c.amg_damping(capi.AMG_OF_HANDLE), lambda: c.amg_damping(capi.AMG_OF_BLOCK),
                 lambda: c.amg_order(capi.AMG_OF_HANDLE), lambda: c.amg_order(capi.AMG_OF_BLOCK)):
        with pytest.raises(capi.FdapdeError) as e:
            call()
        assert e.value.status == capi.ENOTINIT
    for level in (-1, levels - 1, levels):
        with pytest.raises(capi.FdapdeError) as e:
            c.amg_aggregates(capi.AMG_OF_SOLVE, level)
        assert e.value.status == capi.EINVAL
    buf = np.full(n0, -7, dtype=np.int32)
    rows = C.c_int64(-1)
    ip = buf.ctypes.data_as(C.POINTER(C.c_int32))
    assert c.lib.fdapde_amg_aggregates(c._ctx, 0, 0, C.c_int64(n0 - 1), ip, C.byref(rows)) == capi.EINVAL and rows.value == n0 and (buf == -7).all()
    assert c.lib.fdapde_amg_aggregates(c._ctx, 0, 0, C.c_int64(n0), ip, None) == capi.OK and np.array_equal(buf, s["aggs"][0])
    assert c.lib.fdapde_amg_order(c._ctx, 0, C.c_int64(n0 - 1), ip, C.byref(rows)) == capi.EINVAL and c.lib.fdapde_amg_order(c._ctx, 3, C.c_int64(n0), ip, None) == capi.EINVAL
    om = np.full(levels, -7.0)
    nl = C.c_int32(-1)
    dp = om.ctypes.data_as(C.POINTER(C.c_double))
    assert c.lib.fdapde_amg_damping(c._ctx, 3, levels, C.byref(nl), dp) == capi.EINVAL and c.lib.fdapde_amg_damping(c._ctx, 0, 1, C.byref(nl), None) == capi.EINVAL
    assert c.lib.fdapde_amg_damping(c._ctx, 0, 1, C.byref(nl), dp) == capi.OK and nl.value == levels and om[0] == s["om"][0] and (om[1:] == -7.0).all()
    # the handle's hierarchy: live from its first solve until fdapde_lin_compute outlives it
    t = _multilevel(env, "d")
    ct = t["c"]
    assert len(ct.amg_aggregates(capi.AMG_OF_HANDLE, 0)) == t["n"]
    ct.lin_compute(values=t["K"], symmetric=t["sym"])
    for call in (lambda: ct.amg_aggregates(capi.AMG_OF_HANDLE, 0), lambda: ct.amg_damping(capi.AMG_OF_HANDLE), lambda: ct.amg_order(capi.AMG_OF_HANDLE)):
        with pytest.raises(capi.FdapdeError) as e:
            call()
        assert e.value.status == capi.ENOTINIT
    _solve(env, t, 1)   # (the same matrix: the same hierarchy again)
    h, aggs, om = _read_back(t)
    assert h["rows"] == t["h"]["rows"] and all(np.array_equal(a, b) for a, b in zip(aggs, t["aggs"])) and np.array_equal(om, t["om"])
    t["h"] = h   # (its set-up time is the new build's)
