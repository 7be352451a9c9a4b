"""FDAPDE_SOLVER_BLOCK_AMG with the factored data term carried through the hierarchy (knob block_amg_obs = 1; csrc/eng_block_amg.hip, host_obs.cpp obs_coarsen,
kernels_obs.h k_obs_gather_acc / k_obs_scatter_store, kernels_block.h k_bamg_spmv_dots' ADD form), amg_coarse_rows = 256 unless said otherwise.
  1. areal solves against the explicit system sp.bmat of the four blocks + scale Psi^T W Psi (tests/block_obs_ref.py) and SuperLU, within the budgets
     tests/test_block_obs_amg_cpu.py holds the restatement to half of, in fewer iterations than the GMRES stage of the same handle, under both team widths;
  2. other term shapes: weights with exact zeros, a11 on the pattern plus a term, a pointwise Psi against the same system through fdapde_gram_pointwise;
  3. one level: the merged dense inverse alone;
  4. k-th iterates against the extended-precision reference of tests/block_obs_amg_iter_ref.py, built on the DEVICE's aggregates;
  5. the levels as data (fdapde_block_obs_amg_levels) against numpy on the device's aggregates;
  6. columns one by one;
  7. the life cycle of the knob, the term and the hierarchy.
FDAPDE_BLOCK_OBS_AMG_PROFILE=<path> appends the worst iterate ratios per case and k."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import block_amg_ref as ba
import block_iter_ref as ir
import block_obs_amg_iter_ref as oir
import block_obs_amg_ref as boa
import block_obs_ref as bo
import block_ref as br

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = os.path.join(ROOT, "tests", "golden", "mesh")
U = ir.U


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, workloads
    from oracle import oracle as o

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    o.build()
    return capi, workloads, o


_spaces, _systems, _worst = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _spaces.values():
        s["c"].close()
    _spaces.clear()
    path = os.environ.get("FDAPDE_BLOCK_OBS_AMG_PROFILE")
    if path and _worst:
        with open(path, "a") as fh:
            for line in sorted(_worst):
                fh.write(f"gpu {line}: " + " ".join(f"{k}={v:.3g}" for k, v in sorted(_worst[line].items())) + "\n")


def _new_space(env, name, order, carry=1):
    capi, _, o = env
    m = o.load_mesh(os.path.join(MESHES, name))
    c = capi.Context(0)
    c.mesh_upload(np.ascontiguousarray(m.nodes), np.ascontiguousarray(m.cells, dtype=np.int32), np.ascontiguousarray(m.boundary))
    nd = c.dofs_build(order)
    dofs, _, ond, _ = o.enumerate_dofs(m, order)
    assert ond == nd and np.array_equal(c.dofs_get()[0], dofs), "the oracle and the library number the DOFs alike"
    rp, ci = c.pattern_get()
    c.tune("amg_coarse_rows", boa.COARSE_ROWS)
    c.tune("block_amg_obs", carry)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    return {"c": c, "nd": nd, "rp": np.asarray(rp, dtype=np.int64), "ci": np.asarray(ci, dtype=np.int64), "mesh": m, "dofs": dofs,
            "r1": c.matrix_values(capi.MAT_STIFF), "r0": c.matrix_values(capi.MAT_MASS)}


def _space(env, name, order):
    if (name, order) not in _spaces:
        _spaces[(name, order)] = _new_space(env, name, order)
    return _spaces[(name, order)]


def _areal(env, s, name, order, regions):
    o = env[2]
    return bo.areal_psi(o, s["mesh"], order, s["dofs"], s["nd"], bo.incidence(o, s["mesh"], name, regions))


def _system(env, name, order, lam, regions):
    """-> (space, A, b, Psi, blocks, LU solution); the handle is computed and the term set by the caller"""
    s = _space(env, name, order)
    key = (name, order, lam, regions)
    if key not in _systems:
        Psi = _areal(env, s, name, order, regions)
        blocks = bo.smoothing_blocks(s["rp"], s["ci"], s["r1"], s["r0"], lam, s["nd"])
        A = bo.system(s["rp"], s["ci"], blocks, s["nd"], Psi)
        b = bo.smoothing_rhs(Psi, lam, s["nd"])
        _systems[key] = (A, b, Psi, blocks, spl.splu(A.tocsc()).solve(b))
    return (s,) + _systems[key]


def _set(s, blocks, Psi, weights=None, team=0, symmetric=True):
    c = s["c"]
    c.tune("block_obs_team", team)
    c.block_compute(*blocks, symmetric=symmetric)
    c.block_set_obs(Psi, weights)
    c.tune("block_obs_team", 0)


def _check_solve(capi, A, b, x, info, x_lu, cap, what):
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    print(f"{what}: iterations {info.iters} (budget {cap}), relres {info.relres:.2e}, recomputed {res:.2e}, error against LU {err:.2e}")
    assert info.converged == 1 and info.method_used == capi.SOLVER_BLOCK_AMG
    assert res <= 1e-9
    assert err <= 1e-6
    assert info.iters <= cap
    return res, err


# ---- 1. solves, areal -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order,lam,regions", boa.AREAL_CASES)
def test_areal_solves_with_the_term_carried(env, name, order, lam, regions):
    capi = env[0]
    s, A, b, Psi, blocks, x_lu = _system(env, name, order, lam, regions)
    c = s["c"]
    rows = np.diff(Psi.indptr)
    if regions == 2 and name == "unit_square_16":
        assert rows.max() == (81 if order == 1 else 289), "two to five trips of a 64-lane team"
    if regions == 4:
        assert Psi.shape[0] == 16, "fewer rows than the 32 a T = 8 workgroup takes: the partial block"
    cap = boa.budget(order)
    _set(s, blocks, Psi)
    x, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ba.RTOL)
    h = c.amg_hierarchy(capi.AMG_OF_BLOCK)
    lv = c.block_amg_obs_levels()
    print(f"{name} P{order} lambda {lam:g}, {regions}: rows {h['rows']}, nnz(Psi_l) {lv['nnz']}, teams {lv['team_rows']} / {lv['team_cols']}")
    assert len(h["rows"]) >= 2
    _check_solve(capi, A, b, x, info, x_lu, cap, f"{name} P{order} lambda {lam:g}, {regions}")
    xg, ig = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=bo.RTOL, maxit=bo.MAXIT_CAP, raise_on_noconv=False)
    print(f"  the GMRES stage on the same handle: {ig.iters} iterations, converged {ig.converged}")
    assert info.iters < ig.iters
    for team in (8, 64):
        _set(s, blocks, Psi, team=team)
        assert c.block_obs_info()["team_rows"] == team
        xt, it = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ba.RTOL)
        lv = c.block_amg_obs_levels()
        assert set(lv["team_rows"]) == {team} and set(lv["team_cols"]) == {team}
        _check_solve(capi, A, b, xt, it, x_lu, cap, f"  block_obs_team {team}")


# ---- 2. other term shapes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [1e-2, 1e-4])
def test_weights_with_exact_zeros(env, lam):
    capi = env[0]
    s, _, b, Psi, blocks, _ = _system(env, "unit_square_16", 1, lam, 4)
    rng = np.random.default_rng(5)
    w = rng.uniform(0.5, 1.5, Psi.shape[0])
    w[rng.uniform(size=len(w)) < 0.3] = 0.0
    assert (w == 0.0).any(), "a whole region switched off"
    A = bo.system(s["rp"], s["ci"], blocks, s["nd"], Psi, w)
    _set(s, blocks, Psi, w)
    x, info = s["c"].block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ba.RTOL)
    _check_solve(capi, A, b, x, info, spl.splu(A.tocsc()).solve(b), ba.BUDGET_P1, f"lambda {lam:g}, {int((w == 0).sum())} of {len(w)} weights zero")


@pytest.mark.parametrize("lam", [1e-2, 1e-4])
def test_a11_on_the_pattern_plus_a_term(env, lam):
    capi = env[0]
    s, _, b, Psi, blocks, _ = _system(env, "unit_square_16", 1, lam, 4)
    obs = br.observed_nodes(s["mesh"].n_nodes)
    with_a11 = (-br.gram_selection_values(s["rp"], s["ci"], obs, s["nd"]),) + tuple(blocks[1:])
    A = bo.system(s["rp"], s["ci"], with_a11, s["nd"], Psi)
    _set(s, with_a11, Psi)
    x, info = s["c"].block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ba.RTOL)
    _check_solve(capi, A, b, x, info, spl.splu(A.tocsc()).solve(b), ba.BUDGET_P1, f"lambda {lam:g}, a11 on the pattern plus the term")


@pytest.mark.parametrize("lam", [1e-2, 1e-4])
def test_pointwise_term_against_the_gram_matrix_on_the_pattern(env, lam):
    """400 random locations: the factored term carried through the levels against -fdapde_gram_pointwise's values in a11 and the pattern-only hierarchy.  Both
    stop at rtol 1e-12 on the true residual of (up to the rounding of the Gram entries) one matrix, so each solution's error is the condition number times
    1e-12 and they agree to 1e-8; the two hierarchies have the same aggregates and, in exact arithmetic, the same levels: the counts are within 3"""
    capi = env[0]
    s = _space(env, "unit_square_16", 1)
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    pts = np.random.default_rng(9).uniform(0.0, 1.0, size=(400, 2))
    cells, vals = c.eval_pointwise_raw(pts)
    assert (cells >= 0).all()
    nb = vals.shape[1]
    Psi = sp.csr_matrix((vals.reshape(-1), (np.repeat(np.arange(len(pts)), nb), s["dofs"][cells].reshape(-1))), shape=(len(pts), nd))
    Psi.sum_duplicates()
    Psi.sort_indices()
    blocks = bo.smoothing_blocks(rp, ci, s["r1"], s["r0"], lam, nd)
    b = bo.smoothing_rhs(Psi, lam, nd)
    A = bo.system(rp, ci, blocks, nd, Psi)
    x_lu = spl.splu(A.tocsc()).solve(b)
    G = c.gram_pointwise(cells, vals)
    c.block_compute(-G, *blocks[1:], symmetric=True)
    xg, ig = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=1e-12)
    hg = c.amg_hierarchy(capi.AMG_OF_BLOCK)
    with pytest.raises(capi.FdapdeError) as e:
        c.block_amg_obs_levels()
    assert e.value.status == capi.ENOTINIT, "a hierarchy without a term"
    _set(s, blocks, Psi)
    xt, it = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=1e-12)
    ht, lv = c.amg_hierarchy(capi.AMG_OF_BLOCK), c.block_amg_obs_levels()
    diff = np.linalg.norm(xt - xg) / np.linalg.norm(xg)
    print(f"lambda {lam:g}: iterations {it.iters} (term carried) / {ig.iters} (gram on the pattern), |x_term - x_gram| / |x_gram| = {diff:.2e}, rows {ht['rows']}, "
          f"nnz(Psi_l) {lv['nnz']}, error against LU {np.linalg.norm(xt - x_lu) / np.linalg.norm(x_lu):.2e}")
    assert ig.converged == 1 and it.converged == 1 and it.method_used == capi.SOLVER_BLOCK_AMG
    assert ht["rows"] == hg["rows"], "the aggregates do not depend on the term"
    assert it.iters <= ba.BUDGET_P1 and ig.iters <= ba.BUDGET_P1
    assert diff <= 1e-8
    assert abs(it.iters - ig.iters) <= 3
    assert np.linalg.norm(xt - x_lu) <= 1e-6 * np.linalg.norm(x_lu)


# ---- 3. one level ---------------------------------------------------------------------------------------------------------------------------------
def test_one_level_is_the_merged_dense_inverse(env):
    capi = env[0]
    s, A, b, Psi, blocks, x_lu = _system(env, "unit_square_16", 1, 1e-2, 4)
    c = s["c"]
    c.tune("amg_coarse_rows", 600)
    try:
        _set(s, blocks, Psi)
        x, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ba.RTOL)
        h, lv = c.amg_hierarchy(capi.AMG_OF_BLOCK), c.block_amg_obs_levels()
    finally:
        c.tune("amg_coarse_rows", boa.COARSE_ROWS)
    assert h["rows"] == [578] and lv["nnz"] == [Psi.nnz]
    _check_solve(capi, A, b, x, info, x_lu, 2, "one merged dense level")


# ---- 4. k-th iterates -----------------------------------------------------------------------------------------------------------------------------
_refs = {}


def _note(line, k, value):
    d = _worst.setdefault(line, {})
    d[k] = max(d.get(k, 0.0), value)


@pytest.mark.parametrize("team", oir.TEAMS)
@pytest.mark.parametrize("name", list(oir.CASES))
def test_iterates_with_the_term_carried(env, name, team):
    """rtol = 1e-30, maxit = k hands out the k-th iterate; the reference is built on the device's aggregates, one per case for both team widths.  Entrywise
    |x_k - x_ref|_i <= c(k) u s_i wherever s_i > 0, the residual within c(k) u res_scale of the reference's, and per field max |x_k - x_ref| <= c_f(k) u max s
    (constants: tests/test_block_obs_amg_iter_cpu.py)"""
    capi = env[0]
    fixture, order, lam, regions = oir.CASES[name]
    s, A, b, Psi, blocks, _ = _system(env, fixture, order, lam, regions)
    c = s["c"]
    _set(s, blocks, Psi, team=team)
    assert c.block_obs_info()["team_rows"] == team

    def stop_at(k):
        x, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=1e-30, maxit=k, raise_on_noconv=False)
        assert info.iters == k and info.converged == 0 and info.method_used == capi.SOLVER_BLOCK_AMG and np.all(np.isfinite(x))
        return x, info

    stop_at(1)
    h, lv = c.amg_hierarchy(capi.AMG_OF_BLOCK), c.block_amg_obs_levels()
    aggs = [c.amg_aggregates(capi.AMG_OF_BLOCK, l) for l in range(len(h["rows"]) - 1)]
    if name not in _refs:
        H = oir.TermHierarchy(s["rp"], s["ci"], blocks, s["nd"], aggs, Psi)
        _refs[name] = (aggs, H, ir.fgmres_iterates(H, b, max(oir.KS)))
    aggs0, H, its = _refs[name]
    assert all(np.array_equal(a, a0) for a, a0 in zip(aggs, aggs0)), "the aggregates do not depend on the team width"
    # preconditions of the comparison: the reference's levels are the device's
    assert [2 * r for r in H.rows] == h["rows"] and [4 * e for e in H.entries] == h["nnz"] and H.psi_nnz == lv["nnz"]
    if name in ("sq-p2-4x4", "sphere-p1-2"):
        assert len(h["rows"]) >= 3, "a level with GCR steps: the term inside y = A x"
    bad = []
    for k in oir.KS:
        x, info = stop_at(k)
        ref = its[k - 1]
        ratio, fields, rr = ir.entry_ratio(x, ref), max(ir.field_ratios(x, ref)), ir.relres_ratio(info.relres, ref)
        _note(f"block_obs_amg {name} team {team}", k, ratio)
        _note(f"block_obs_amg {name} team {team} [field]", k, fields)
        _note(f"block_obs_amg {name} team {team} [relres]", k, rr)
        print(f"block_obs_amg {name} team {team} k={k}: worst |err|_i / (u s_i) = {ratio:.3g} (c = {oir.C_OBS_AMG[k]:g}), per field / (u max s) = {fields:.3g} "
              f"(c = {oir.C_OBS_AMG_FIELD[k]:g}), relres {rr:.3g}")
        err = np.abs(x.astype(ir.LD) - ref.x)
        live = ref.s > 0
        if (err[live] > oir.C_OBS_AMG[k] * U * ref.s[live]).any():
            bad.append((k, "iterate, entrywise", ratio / oir.C_OBS_AMG[k]))
        if not fields <= oir.C_OBS_AMG_FIELD[k]:
            bad.append((k, "iterate, per field", fields / oir.C_OBS_AMG_FIELD[k]))
        if not rr <= oir.C_OBS_AMG[k]:
            bad.append((k, "relres", rr / oir.C_OBS_AMG[k]))
    assert not bad, (name, team, "(k, what, times the bound)", bad)   # (every k is run and printed before the verdict)


# ---- 5. levels as data ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order,regions", [("unit_square_16", 2, 2), ("unit_sphere", 1, 2), ("quasi_circle", 1, "golden")])
def test_levels_as_data(env, name, order, regions):
    capi = env[0]
    s, A, b, Psi, blocks, _ = _system(env, name, order, 1e-4, regions)
    c = s["c"]
    for team in (0, 8, 64):
        _set(s, blocks, Psi, team=team)
        with pytest.raises(capi.FdapdeError) as e:   # (the new term dropped the hierarchy)
            c.block_amg_obs_levels()
        assert e.value.status == capi.ENOTINIT
        c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=ba.RTOL)
        h, lv = c.amg_hierarchy(capi.AMG_OF_BLOCK), c.block_amg_obs_levels()
        levels = len(h["rows"])
        assert all(len(lv[key]) == levels for key in ("nnz", "longest_row", "team_rows", "team_cols"))
        aggs = [c.amg_aggregates(capi.AMG_OF_BLOCK, l) for l in range(levels - 1)]
        S = abs(Psi.sign()).tocsr()
        longest = [int(np.diff(S.indptr).max())]
        for agg in aggs:
            S = (S @ sp.csr_matrix((np.ones(len(agg)), (np.arange(len(agg)), agg)), shape=(len(agg), int(agg.max()) + 1))).tocsr()
            longest.append(int(np.diff(S.indptr).max()))
        print(f"{name} P{order} team {team}: rows {h['rows']}, nnz(Psi_l) {lv['nnz']}, longest row {lv['longest_row']}, teams {lv['team_rows']} / {lv['team_cols']}")
        assert lv["nnz"] == boa.levels_nnz(Psi, aggs)
        assert all(a >= b_ for a, b_ in zip(lv["nnz"], lv["nnz"][1:])), "the counts do not increase"
        assert lv["longest_row"] == longest
        rule = lambda rows, nnz: team if team else (64 if nnz > 16 * rows else 8)   # obs_team_width
        assert lv["team_rows"] == [rule(Psi.shape[0], z) for z in lv["nnz"]]
        assert lv["team_cols"] == [rule(r // 2, z) for r, z in zip(h["rows"], lv["nnz"])]


# ---- 6. columns -----------------------------------------------------------------------------------------------------------------------------------
def test_columns_go_one_by_one(env):
    capi = env[0]
    s, A, b, Psi, blocks, x_lu = _system(env, "unit_square_16", 1, 1e-2, 4)
    c = s["c"]
    _set(s, blocks, Psi)
    rng = np.random.default_rng(4)
    B = np.stack([b, rng.standard_normal(len(b)), bo.smoothing_rhs(Psi, 1e-2, s["nd"], seed=7)], axis=1)
    X, info = c.block_solve(B, method=capi.SOLVER_BLOCK_AMG, rtol=ba.RTOL)
    assert info.converged == 1 and info.iters <= 3 * ba.BUDGET_P1
    for j in range(3):
        assert np.linalg.norm(B[:, j] - A @ X[:, j]) <= 1e-9 * np.linalg.norm(B[:, j])
    assert np.linalg.norm(X[:, 0] - x_lu) <= 1e-6 * np.linalg.norm(x_lu)
    assert c.amg_cols_trace(capi.AMG_OF_BLOCK) == dict(batches=0, batched_cols=0, single_cols=3)


# ---- 7. life cycle --------------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(env):
    capi = env[0]
    lam = 1e-2
    s = _new_space(env, "unit_square_16", 1, carry=1)
    never = _new_space(env, "unit_square_16", 1, carry=0)   # a context that never has a term, the knob at its default
    try:
        c, n, nd, rp, ci = s["c"], never["c"], s["nd"], s["rp"], s["ci"]
        Psi = _areal(env, s, "unit_square_16", 1, 4)
        blocks = bo.smoothing_blocks(rp, ci, s["r1"], s["r0"], lam, nd)
        b = bo.smoothing_rhs(Psi, lam, nd)
        # the knob at 1 and no term: bit for bit the default (a11 on the pattern makes the pattern-only system regular)
        obs = br.observed_nodes(s["mesh"].n_nodes)
        plain = br.smoothing_blocks(rp, ci, s["r1"], s["r0"], obs, lam, nd)
        bp = br.smoothing_rhs(obs, lam, nd)
        xs = np.random.default_rng(2).standard_normal(2 * nd)

        def same_bits():
            assert np.array_equal(c.block_spmv(xs), n.block_spmv(xs))
            for method in (capi.SOLVER_GMRES, capi.SOLVER_BLOCK_AMG):
                x1, i1 = c.block_solve(bp, method=method)
                x0, i0 = n.block_solve(bp, method=method)
                assert i1.converged == 1 and i1.iters == i0.iters and np.array_equal(x1, x0), method

        c.block_compute(*plain, symmetric=True)
        n.block_compute(*plain, symmetric=True)
        same_bits()
        with pytest.raises(capi.FdapdeError) as e:
            c.block_amg_obs_levels()
        assert e.value.status == capi.ENOTINIT, "a hierarchy without a carried term"
        # a term, then a second one with other weights: the LU solution of the NEW system
        c.block_compute(*blocks, symmetric=True)
        c.block_set_obs(Psi)
        x, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG)
        A = bo.system(rp, ci, blocks, nd, Psi)
        assert info.converged == 1 and np.linalg.norm(x - spl.splu(A.tocsc()).solve(b)) <= 1e-6 * np.linalg.norm(x)
        w = np.random.default_rng(8).uniform(0.5, 2.0, Psi.shape[0])
        c.block_set_obs(Psi, w)
        with pytest.raises(capi.FdapdeError) as e:
            c.block_amg_obs_levels()
        assert e.value.status == capi.ENOTINIT, "the new term dropped the hierarchy"
        xw, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG)
        Aw = bo.system(rp, ci, blocks, nd, Psi, w)
        xw_lu = spl.splu(Aw.tocsc()).solve(b)
        assert info.converged == 1 and np.linalg.norm(xw - xw_lu) <= 1e-6 * np.linalg.norm(xw_lu)
        assert np.linalg.norm(xw - x) > 1e-3 * np.linalg.norm(x), "another system"
        # the knob back to 0: the refusal, naming the knob; the hierarchy is gone
        c.tune("block_amg_obs", 0)
        with pytest.raises(capi.FdapdeError) as e:
            c.block_solve(b, method=capi.SOLVER_BLOCK_AMG)
        assert e.value.status == capi.EUNSUPPORTED and "term" in str(e.value) and "block_amg_obs" in str(e.value)
        with pytest.raises(capi.FdapdeError) as e:
            c.amg_hierarchy(capi.AMG_OF_BLOCK)
        assert e.value.status == capi.ENOTINIT
        with pytest.raises(capi.FdapdeError) as e:
            c.tune("block_amg_obs", 2)
        assert e.value.status == capi.EINVAL
        c.tune("block_amg_obs", 1)
        x2, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG)
        assert info.converged == 1 and np.array_equal(x2, xw), "the same hierarchy built again: the same bits"
        # clearing the term and solving equals, bit for bit, a context that never had a term
        c.block_compute(*plain, symmetric=True)
        c.block_set_obs(Psi)
        c.block_solve(bp, method=capi.SOLVER_BLOCK_AMG, raise_on_noconv=False)
        c.block_set_obs(None)
        same_bits()
        # block_compute drops the term and the hierarchy
        c.block_set_obs(Psi)
        c.block_solve(bp, method=capi.SOLVER_BLOCK_AMG, raise_on_noconv=False)
        c.block_amg_obs_levels()
        c.block_compute(*plain, symmetric=True)
        for call in (c.block_obs_info, c.block_amg_obs_levels, lambda: c.amg_hierarchy(capi.AMG_OF_BLOCK)):
            with pytest.raises(capi.FdapdeError) as e:
                call()
            assert e.value.status == capi.ENOTINIT
        same_bits()
    finally:
        s["c"].close()
        never["c"].close()
