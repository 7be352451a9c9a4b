"""The Kronecker-sum handle's two Krylov stages at the k-th iterate, against the extended-precision reference of tests/kron_iter_ref.py.

`rtol = 1e-30, maxit = k` stops a solve after exactly k iterations and hands the iterate out.  A flexible outer iteration controlled by its true residual
corrects its preconditioner's mistakes, so a converged answer says little about the cycle; the k-th iterate says everything: with the aggregates fixed
it is ONE vector in exact arithmetic.

FDAPDE_SOLVER_KRON_AMG (csrc/eng_kron_amg.hip, the k_kamg_* kernels).  After the first solve the device's own hierarchy is read back --
fdapde_kron_amg_hierarchy and every level's fdapde_kron_amg_aggregates -- and the reference hierarchy is built from the caller's terms and those maps; its
DOFs and entries must be the device's on every level (q n_l rows, q^2 nnz_l entries).  Per unknown r = 0 .. q - 1 (the n entries of one unknown are a field)

    max |x_gpu - x_ref| <= c_amg(k) u max s,        u = 2^-53,  s = sum_j |y_j| |z_j| entrywise,
    |info.relres - rho_k| <= c_amg(k) u || |A| s || / ||b||, and info.relres within 1e-12 relative of the residual of the vector handed out.

The handle's GMRES stage (kron_gmres through handle_gmres, operator launch_kron_op, with a factored term the k_kron_obs_* kernels behind it): entrywise
|x_gpu - x_ref|_i <= c_gm(k) u s_i, s = sum_j |y_j| |v_j|, exactly 0 where s_i = 0 (the Krylov front has not arrived), and relres against rho_k of the
scaled system in the same form.

c(k) = 4 r_cpu(k) rounded up to a power of two, r_cpu the worst ratio of the float64 numpy checkers of the same schemes against the reference on the same
cases (tests/test_kron_iter_cpu.py measures it on the oracle's matrices and fails if a constant is not the rule's value or exceeds 2^12;
profiles/kron_iterates.txt).

FDAPDE_KRON_ITER_PROFILE=<path> appends the worst ratio per case and k."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import block_iter_ref as ir
import block_ref as br
import kron_amg_ref as ka
import kron_iter_ref as ki
import kron_obs_ref as ko

pytestmark = pytest.mark.gpu
U = ki.U


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, meshgen


_live = {}      # (mesh, order, system or case, knobs) -> dict of the context and what was built on it
_worst = {}     # line -> {k: ratio}
_host = {}      # case -> seconds of host-side reference work


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _live.values():
        s["c"].close()
    _live.clear()
    path = os.environ.get("FDAPDE_KRON_ITER_PROFILE")
    if path and _worst:
        with open(path, "a") as fh:
            for line in sorted(_worst):
                fh.write(f"gpu {line}: " + " ".join(f"{k}={v:.3g}" for k, v in sorted(_worst[line].items())) + "\n")


def _note(line, k, value):
    d = _worst.setdefault(line, {})
    d[k] = max(d.get(k, 0.0), value)


def _space(env, mesh, order, key, knobs):
    """one context per key with the space built, R1 = stiff(-laplacian) and R0 = mass assembled on the device, and the knobs set"""
    capi, meshgen = env
    key = (mesh, order, key, tuple(sorted(knobs.items())))
    if key not in _live:
        nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
        c = capi.Context(0)
        c.mesh_upload(nodes, cells, bnd)
        nd = c.dofs_build(order)
        for k_, v_ in knobs.items():
            c.tune(k_, v_)
        c.set_operator(-capi.laplacian())
        c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
        c.init()
        rp, ci = c.pattern_get()
        _live[key] = dict(c=c, rp=np.asarray(rp, dtype=np.int64), ci=np.asarray(ci, dtype=np.int64), n=nd, r1=c.matrix_values(capi.MAT_STIFF),
                          r0=c.matrix_values(capi.MAT_MASS), obs=br.observed_nodes(nodes.shape[0]), nodes=nodes, cells=cells, bnd=bnd,
                          restart=knobs.get("gmres_m", 50))
    return _live[key]


def _context(env, system, knobs):
    """the context of (system, knobs) with the system's handle computed"""
    case = ki.SYSTEMS[system]
    s = _space(env, case[1], case[2], system, knobs)
    if "terms" not in s:
        s["terms"], s["q"], s["b"] = ki.system(case, s["rp"], s["ci"], s["r1"], s["r0"], s["obs"])
        s["c"].kron_compute(s["terms"])
        Ts, Ss, _ = ka.merge(s["terms"])
        s["n_s"] = len(Ss)
        s["A"] = ki.KronCsr(s["rp"], s["ci"], Ts, Ss, ki.LD)
    return s


def _solve(env, s, b, method, k, columns=1):
    x, info = s["c"].kron_solve(b, method=method, rtol=1e-30, maxit=k, raise_on_noconv=False)
    assert info.iters == columns * k and info.converged == 0 and info.method_used == method, (info.iters, info.converged, info.method_used)
    assert np.all(np.isfinite(x))
    return x, info


def _team(q):
    Q = 2
    while Q < q:
        Q *= 2
    return Q


def _multilevel(env, name):
    """the case's context after its first multilevel solve, with the device's hierarchy read back and the reference built on it"""
    capi = env[0]
    system, knobs, _ = ki.AMG_CASES[name]
    knobs = dict(knobs, amg_setup_check=1)
    s = _context(env, system, knobs)
    if "H" not in s:
        c, q = s["c"], s["q"]
        _solve(env, s, s["b"], capi.SOLVER_KRON_AMG, 1)
        h = c.kron_amg_hierarchy()
        levels = len(h["rows"])
        aggs = [c.kron_amg_aggregates(l) for l in range(levels - 1)]
        for l, agg in enumerate(aggs):
            assert agg.dtype == np.int32 and agg.shape == (h["rows"][l] // q,)
            assert agg.min() == 0 and agg.max() == h["rows"][l + 1] // q - 1 and len(np.unique(agg)) == h["rows"][l + 1] // q, "a map onto the next level's DOFs"
        t0 = time.perf_counter()
        H = ki.Hierarchy(s["rp"], s["ci"], s["terms"], s["n"], aggs)
        _host[name] = time.perf_counter() - t0
        # preconditions of the comparison: the reference's levels are the device's
        assert [q * r for r in H.rows] == h["rows"], (H.rows, h["rows"])
        assert [q * q * e for e in H.entries] == h["nnz"], (H.entries, h["nnz"])
        assert h["rows"][-1] <= ki.LAST_LEVEL_ROWS
        s["h"], s["aggs"], s["H"] = h, aggs, H
        print(f"case {name}: q = {q}, n_S = {s['n_s']}, rows per level {h['rows']}, absorbed {h['absorbed']}, reference hierarchy built in {_host[name]:.1f} s on the host")
    return s


def _preconditions(name, s):
    """what the case is there to reach, asserted from the device's own hierarchy and the system's pattern"""
    h, q, n, n_s = s["h"], s["q"], s["n"], s["n_s"]
    Q = _team(q)
    levels = len(h["rows"])
    dofs = [r // q for r in h["rows"]]
    if name in ki.THREE_LEVELS:
        assert levels >= 3, "a level with GCR steps"
    if name not in ("i", "j", "o", "p"):
        assert n == 289, "a partly empty last workgroup at every team width"
    if name in ("a", "m"):
        assert q == 6 and Q == 8, "idle lanes in a team of 8"
    if name in ("b", "c"):
        assert Q == 2 and q == {"b": 1, "c": 2}[name]
    if name in ("d", "e", "n"):
        T = ka.merge(s["terms"])[0][0]
        assert q == 5 and (np.count_nonzero(np.triu(T, 1)) == 0 and np.count_nonzero(np.tril(T, -2)) == 0 if name != "e" else np.all(T != 0)), "a band to skip / none"
    if name in ("f", "f+"):
        assert q == 16 and (n_s * q * q <= ki.LDS_FACTOR_DOUBLES) == (name == "f") and n_s == (4 if name == "f" else 5), "the time factors in LDS at the limit / from global memory above it"
    if name in ("g", "o", "p"):
        assert q == 33 and Q == 64 and n_s * q * q > ki.LDS_FACTOR_DOUBLES
    if name == "h":
        assert q == Q == 64
    if name == "i":
        assert h["absorbed"] == 1 and max(int(np.bincount(a).max()) for a in s["aggs"]) > 4, "some aggregate has more than four members"
    if name == "j":
        lens = np.diff(s["rp"])
        assert (lens % 4 != 0).any() and lens.min() < 8 and lens.max() > 16, "rows whose length is no multiple of 4 beside short ones: the unrolled gather and its tail"
    if name == "k":
        assert levels == 1 and q * n <= ki.AMG_CASES[name][1]["amg_coarse_rows"], "the correction is the dense level alone"
    if name == "l":
        assert levels == 2, "the cycle without GCR steps"
    if name == "m":
        assert s["restart"] == 3 and max(ki.AMG_CASES[name][2]) > 3, "the outer iteration restarts from its true residual inside the run"
    if name == "o":
        assert n * Q > 256 * 1024, "more rows than 1 024 workgroups hold: np at its cap on level 0"
    if name == "p":
        assert levels >= 3 and dofs[1] * Q > 256 * 1024, "level 1 runs k_kamg_spmv_dots (a GCR level) on more rows than its 1 024 workgroups hold: the row loop's second trip"


def _residual(s, x, b):
    return ki.residual(s["A"], b, x)


@pytest.mark.parametrize("name", list(ki.AMG_CASES))
def test_multilevel_iterates(env, name):
    capi = env[0]
    ks = ki.AMG_CASES[name][2]
    s = _multilevel(env, name)
    h, q = s["h"], s["q"]
    _preconditions(name, s)
    columns = [s["b"], ki.second_column(s["b"])] if name == "n" else [s["b"]]
    t0 = time.perf_counter()
    its = [ki.fgmres_iterates(s["H"], b, max(ks), s["restart"]) for b in columns]
    _host[name] = _host.get(name, 0.0) + time.perf_counter() - t0
    print(f"case {name}: host-side reference {_host[name]:.1f} s in all")
    bad = []
    for k in ks:
        X, info = _solve(env, s, np.column_stack(columns) if len(columns) > 1 else columns[0], capi.SOLVER_KRON_AMG, k, len(columns))
        assert s["c"].kron_amg_hierarchy()["rows"] == h["rows"] and s["c"].kron_amg_hierarchy()["nnz"] == h["nnz"], "the hierarchy of the first solve serves every later one"
        assert all(np.array_equal(s["c"].kron_amg_aggregates(l), a) for l, a in enumerate(s["aggs"]))
        for col, (b, ref_its) in enumerate(zip(columns, its)):
            x = X[:, col] if len(columns) > 1 else X
            ref = ref_its[k - 1]
            ratios = ki.field_ratios(x, ref, q)
            res = _residual(s, x, b)
            tag = f"kron_amg {name}" + (f" column {col}" if len(columns) > 1 else "")
            _note(tag, k, max(ratios))
            line = f"{tag} k={k}: worst |err| / (u max s) over the {q} unknowns = {max(ratios):.3g} (unknown {int(np.argmax(ratios))})"
            if len(columns) == 1:   # (info of a several-column call is the last column's relres and the summed count)
                rr = ki.relres_ratio(info.relres, ref)
                _note(tag + " [relres]", k, rr)
                line += f", relres {rr:.3g} (c = {ki.C_AMG[k]:g}), relres {info.relres:.3e} against the residual of the vector handed out: {abs(info.relres - res) / res:.1e} relative"
                if not rr <= ki.C_AMG[k]:
                    bad.append((k, "relres", rr / ki.C_AMG[k]))
                # (one level: the iterate is the solution and both residuals are rounding -- the device's own evaluation of b - A x in float64 is then
                # exact to a rounding of every term, u (|A| |x| + |b|), not to 1e-12 of a residual of 1e-16)
                floor = ki.C_AMG[k] * U * ki.residual_scale(s["A"], b, x) if len(h["rows"]) == 1 else 0.0
                if not abs(info.relres - res) <= 1e-12 * res + floor:
                    bad.append((k, "relres is not the residual of the vector handed out", info.relres, res))
            else:
                line += f" (c = {ki.C_AMG[k]:g}); residual of the vector handed out {res:.3e}, the reference's {ref.rho:.3e}"
                if not abs(res - ref.rho) <= ki.C_AMG[k] * U * ref.res_scale + 1e-12 * res:
                    bad.append((k, col, "residual", res, ref.rho))
            print(line)
            if not max(ratios) <= ki.C_AMG[k]:
                bad.append((k, col, "iterate", max(ratios) / ki.C_AMG[k]))
    assert not bad, (name, "(k, what, times the bound)", bad)   # (every k is run and printed before the verdict)


def _gmres_checks(name, tag, k, x, info, ref, constants, rhs, bad):
    dead = ref.s == 0
    if rhs == "unit":
        assert dead.any(), "the front has not reached every entry"
    assert not x[dead].any(), f"{name} k={k}: entries the Krylov front has not reached must be exactly 0 ({int((x[dead] != 0).sum())} are not)"
    ratio = ki.entry_ratio(x, ref)
    rr = ki.relres_ratio(info.relres, ref)
    _note(f"{tag} {name}", k, ratio)
    _note(f"{tag} {name} [relres]", k, rr)
    print(f"{tag} {name} k={k}: worst |err| / (u s) = {ratio:.3g}, relres {rr:.3g} (c = {constants[k]:g}), {int(dead.sum())} dead entries")
    err = np.abs(x.astype(ki.LD) - ref.x)
    if (err > constants[k] * U * ref.s).any():
        bad.append((k, "iterate", ratio / constants[k]))
    if not rr <= constants[k]:
        bad.append((k, "relres", rr / constants[k]))


@pytest.mark.parametrize("name", list(ki.GMRES_CASES))
def test_gmres_stage_iterates(env, name):
    capi = env[0]
    system, knobs, rhs, ks = ki.GMRES_CASES[name]
    s = _context(env, system, knobs)
    b = s["b"] if rhs == "system" else ki.unit_rhs(s["n"], s["q"], ir.interior_dof(s["rp"], s["n"]))
    its = ki.gmres_iterates(s["rp"], s["ci"], s["terms"], s["n"], b, max(ks), s["restart"])
    if knobs.get("gmres_m"):
        assert max(ks) > knobs["gmres_m"], "the cycle restarts inside the run"
    bad = []
    for k in ks:
        x, info = _solve(env, s, b, capi.SOLVER_GMRES, k)
        _gmres_checks(name, "gmres", k, x, info, its[k - 1], ki.C_GMRES, rhs, bad)
    assert not bad, (name, "(k, what, times the bound)", bad)   # (every k is run and printed before the verdict)


@pytest.mark.parametrize("name", list(ki.GMRES_OBS_CASES))
def test_gmres_stage_iterates_with_a_factored_term(env, oracle, name):
    capi = env[0]
    case = ki.GMRES_OBS_CASES[name]
    mesh, m, p, lam, design, miss, phi, knobs, edit, ks = case
    s = _space(env, mesh, 1, "obs-" + name, knobs)
    c, n = s["c"], s["n"]
    om = oracle.Mesh(np.ascontiguousarray(s["nodes"], dtype=float), np.ascontiguousarray(s["cells"], dtype=np.int32), np.ascontiguousarray(s["bnd"], dtype=np.uint8))
    dofs, _, nd, _ = oracle.enumerate_dofs(om, 1)
    assert nd == n and np.array_equal(c.dofs_get()[0], dofs), "the oracle and the library number the DOFs alike"
    Psi = ko.design_psi(oracle, om, None, 1, dofs, nd, design)
    if edit == "holes":
        Psi = ki.with_holes(Psi)
    terms, q, b, obs, phi_given = ki.obs_system(case, s["rp"], s["ci"], s["r1"], s["r0"], Psi)
    rows, cols = np.diff(Psi.indptr), np.bincount(Psi.indices, minlength=n)
    if design[0] == "tiles":
        assert rows.min() >= 100, "areal rows of hundreds of entries"
    else:
        assert rows.max() <= 3, "pointwise rows: one cell's DOFs"
    if edit == "holes":
        assert (rows == 0).sum() >= 1 and (cols == 0).sum() >= 1, "an empty row of Psi and an empty row of Psi^T"
    assert (obs["W"] == 0).any(), "missing observations: exact zeros among the weights"
    c.kron_compute(terms, symmetric=True)
    c.kron_set_obs(Psi, Phi=phi_given, weights=obs["W"], scale=obs["scale"])
    info = c.kron_obs_info()
    assert info["p"] == p and info["n_obs"] == Psi.shape[0] and info["nnz"] == Psi.nnz
    form = knobs.get("kron_obs_form", 0)
    if form:
        assert info["form_rows"] == form and info["form_cols"] == form, "the kernel form under test"
    if phi == "null":
        assert phi_given is None and p < q
    if phi == "dense":
        assert p > q and _team(max(p, q)) > _team(q), "the term's team is wider than the product's"
    its = ki.gmres_iterates(s["rp"], s["ci"], terms, n, b, max(ks), obs=obs)
    bad = []
    for k in ks:
        x, inf = _solve(env, s, b, capi.SOLVER_GMRES, k)
        _gmres_checks(name, "gmres_obs", k, x, inf, its[k - 1], ki.C_GMRES_OBS, "system", bad)
    assert not bad, (name, "(k, what, times the bound)", bad)   # (every k is run and printed before the verdict)


def test_the_getter_refuses_what_it_cannot_answer(env):
    """what tests/test_gpu_kron_amg.py leaves open: levels outside the hierarchy, a short buffer, a one-level hierarchy, and that neither a GMRES solve nor
    the hierarchy of another context answers for this one"""
    capi = env[0]
    s = _multilevel(env, "c")
    c, levels, n0, q = s["c"], len(s["h"]["rows"]), s["n"], s["q"]
    for level in (-1, levels - 1, levels):   # (the last level has no next one)
        with pytest.raises(capi.FdapdeError) as e:
            c.kron_amg_aggregates(level)
        assert e.value.status == capi.EINVAL
    buf = np.full(n0, -7, dtype=np.int32)
    rows = C.c_int64(-1)
    rc = c.lib.fdapde_kron_amg_aggregates(c._ctx, 0, C.c_int64(n0 - 1), buf.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rows))
    assert rc == capi.EINVAL and rows.value == n0 and (buf == -7).all(), "a buffer one entry short is refused untouched"
    assert c.lib.fdapde_kron_amg_aggregates(c._ctx, 0, C.c_int64(n0), buf.ctypes.data_as(C.POINTER(C.c_int32)), None) == capi.OK
    assert np.array_equal(buf, s["aggs"][0])
    rc = c.lib.fdapde_kron_amg_aggregates(c._ctx, 1, C.c_int64(n0), buf.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rows))
    assert rc == capi.OK and rows.value == s["h"]["rows"][1] // q and np.array_equal(buf[:rows.value], s["aggs"][1]), "level 1 counts its own DOFs"
    one = _multilevel(env, "k")   # one level: there is a hierarchy, and no level of it has a next one
    assert len(one["h"]["rows"]) == 1 and one["h"]["rows"][0] == one["q"] * one["n"]
    with pytest.raises(capi.FdapdeError) as e:
        one["c"].kron_amg_aggregates(0)
    assert e.value.status == capi.EINVAL
    never = _context(env, "d", {})   # (the GMRES cases' context: its handle is computed, no multilevel solve has run on it)
    _solve(env, never, never["b"], capi.SOLVER_GMRES, 1)
    for call in (lambda: never["c"].kron_amg_aggregates(0), never["c"].kron_amg_hierarchy):
        with pytest.raises(capi.FdapdeError) as e:
            call()
        assert e.value.status == capi.ENOTINIT, "no hierarchy before the first multilevel solve"
    for which in (capi.AMG_OF_SOLVE, capi.AMG_OF_HANDLE, capi.AMG_OF_BLOCK):   # (a context with a Kronecker hierarchy only: the others' getters are not live)
        with pytest.raises(capi.FdapdeError) as e:
            c.amg_hierarchy(which)
        assert e.value.status == capi.ENOTINIT
    assert c.kron_amg_hierarchy()["rows"] == s["h"]["rows"], "the hierarchy stays"
