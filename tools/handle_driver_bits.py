"""The block and Kronecker handles through their shared solve driver (csrc/eng_handle.h), and the scalar entry points through FDAPDE_SOLVER_AMG's outer run
(csrc/amg_setup.h), against the parent commit's library: the same bits, and no slower.

  handle_driver_bits.py PARENT_LIB [OUT]          (OUT defaults to profiles/handle_driver_bits.txt)
  handle_driver_bits.py --time PARENT_LIB [OUT]   (OUT defaults to profiles/handle_driver_time.txt)

PARENT_LIB is libfdapde_hip.so built from the parent commit.  Every run is one fresh process per library and case (FDAPDE_HIP_LIB chooses the library).

Bits.  A case is a handle (block, kron), one of the three fixtures of tests/test_gpu_kron.py and a data term live or not.  Inside it, on a freshly computed
matrix each: every method (FDAPDE_SOLVER_GMRES, FDAPDE_SOLVER_DENSE, the open method, FDAPDE_SOLVER_BLOCK_AMG / _KRON_AMG), one and five columns, in place and
out of place.  Compared: x byte for byte (its SHA-256), info.iters, relres (as bits), converged, method_used -- or, where the call is refused, the status and
the message.  The parent runs twice first: a sub-case where it does not repeat itself is reported with that difference instead of being compared.
A third kind of case, "scalar", runs one fixture through fdapde_solve with FDAPDE_SOLVER_AMG (with and without Dirichlet data), fdapde_solve_parabolic with it
over three steps (the start from x0: every step after the first starts from the step before) and fdapde_lin_solve with it at 1, 5 and 8 columns under
`amg_cols` 8 and 1, in place and out of place.  A scalar sub-case must SOLVE: a status other than FDAPDE_OK / FDAPDE_ENOCONV ends the tool with an error instead of
being compared as a refusal (fdapde_solve_parabolic must converge as well).

Time.  Host overhead per column is what the driver could have changed: 64 columns through each stage (GMRES, DENSE, multilevel) at 289 DOFs, wall time of
the call; the "scalar" rows are 64 columns through fdapde_lin_solve under FDAPDE_SOLVER_AMG and one solve at the size of amg_cols_time.py (29 791 DOFs,
eight columns).  The two libraries alternate, five windows each, every window a fresh process with one warm-up call per figure.  The gate: this tree's median is at
most the largest of the parent's five windows.  (One solve per stage at the sizes of DESIGN 14 / 15: block_amg_time.py --driver-guard, kron_time.py
--driver-guard; they append to the same file.)"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FIXTURES = [("unit_square_16", 1), ("c_shaped", 2), ("unit_sphere", 1)]
LAMBDA = 1e-2
M_TIME = 2   # time nodes of the space-time system: q = 4


def _setup(handle, name, order):
    """-> (capi, context, compute(), set_term(), rows)"""
    import block_ref as br
    import kron_ref as kr
    import scipy.sparse as sp
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, workloads

    nodes, cells, bnd = workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", name))
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(order)
    c.tune("amg_coarse_rows", 256)
    c.tune("block_amg_obs", 1)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    rp, ci = c.pattern_get()
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    obs = br.observed_nodes(nodes.shape[0])
    psi = sp.csr_matrix((np.ones(len(obs)), (np.arange(len(obs)), np.asarray(obs))), shape=(len(obs), nd))
    if handle == "block":
        blocks = br.smoothing_blocks(rp, ci, r1, r0, obs, LAMBDA, nd)
        return capi, c, lambda: c.block_compute(*blocks, symmetric=True), lambda: c.block_set_obs(psi), 2 * nd
    terms = kr.spacetime_terms(rp, ci, r1, r0, obs, LAMBDA, LAMBDA, M_TIME)
    return capi, c, lambda: c.kron_compute(terms, symmetric=True), lambda: c.kron_set_obs(psi), 2 * M_TIME * nd


def _methods(capi, handle):
    return [("GMRES", capi.SOLVER_GMRES), ("DENSE", capi.SOLVER_DENSE), ("open", capi.SOLVER_AUTO),
            ("AMG", capi.SOLVER_BLOCK_AMG if handle == "block" else capi.SOLVER_KRON_AMG)]


def bits_child(handle, name, order, term):
    capi, c, compute, set_term, rows = _setup(handle, name, int(order))
    solve = c.block_solve if handle == "block" else c.kron_solve
    inplace = c.block_solve_inplace if handle == "block" else c.kron_solve_inplace
    B = np.random.default_rng(5).standard_normal((rows, 5))
    for mname, method in _methods(capi, handle):
        for ncols in (1, 5):
            for place in ("out", "in"):
                compute()   # (a fresh matrix: the rent-or-buy count, the inverse and the hierarchy start over)
                if term == "term":
                    set_term()
                row = {"sub": f"{mname} {ncols} col {'out of' if place == 'out' else 'in'} place"}
                try:
                    if place == "out":
                        X, info = solve(B[:, :ncols].copy(), method=method, maxit=1000, raise_on_noconv=False)
                    else:
                        X = np.asfortranarray(B[:, :ncols].copy())
                        info = inplace(X, method=method, maxit=1000)
                    row.update(x=hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest(), iters=int(info.iters), relres=float(info.relres).hex(),
                               converged=int(info.converged), method_used=int(info.method_used))
                except capi.FdapdeError as e:
                    row.update(status=int(e.status), message=str(e))
                print("ROW " + json.dumps(row), flush=True)
    c.close()


def _scalar(name, order, op=None, dirichlet=False, times=None):
    """-> (capi, context, n_dofs) with the operator's system assembled (-laplacian + reaction(1) unless op says otherwise); times: one forcing column per time
    point (what fdapde_solve_parabolic takes)"""
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, workloads

    c = capi.Context(0)
    c.mesh_upload(*workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", name)))
    nd = c.dofs_build(order)
    c.tune("amg_coarse_rows", 256)
    c.set_operator(op(capi) if op else -capi.laplacian() + capi.reaction(1.0))
    qn = c.quadrature_nodes()
    f = np.sin(2.0 * qn[:, 0]) + 1.0
    c.set_forcing(f if times is None else np.stack([(1.0 + t) * f for t in times], axis=1))
    if dirichlet:
        c.set_dirichlet(c.dofs_get()[2].sum(axis=1))
    c.init()
    return capi, c, nd


def _row(sub, x, info):
    return {"sub": sub, "x": hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest(), "iters": int(info.iters), "relres": float(info.relres).hex(),
            "converged": int(info.converged), "method_used": int(info.method_used)}


def scalar_child(name, order):
    import ctypes as C

    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi

    order = int(order)
    rows = []

    def attempt(sub, run):   # (a scalar sub-case that does not reach the solver compares nothing: it is an error, not a row)
        try:
            x, info = run()
        except capi.FdapdeError as e:
            raise SystemExit(f"{name} P{order}, {sub}: status {e.status} ({e}); the case must solve")
        assert info.method_used == capi.SOLVER_AMG and info.iters > 0, (sub, info.method_used, info.iters)
        rows.append(_row(sub, x, info))

    for sub, dirichlet in (("solve AMG", False), ("solve AMG, Dirichlet data", True)):
        _, c, nd = _scalar(name, order, None, dirichlet)
        attempt(sub, lambda: (lambda info: (c.solution(), info))(c.solve(method=capi.SOLVER_AMG, maxit=1000, raise_on_noconv=False)))
        c.close()
    times = np.linspace(0.0, 0.3, 4)
    _, c, nd = _scalar(name, order, lambda capi: -capi.laplacian() + capi.reaction(1.0) + capi.dt(), True, times)
    coords = c.dofs_get()[2]
    g = np.stack([(1.0 + t) * coords.sum(axis=1) for t in times], axis=1)
    attempt("solve_parabolic AMG, three steps", lambda: c.solve_parabolic(times, np.cos(coords[:, 0]), dirichlet=g, method=capi.SOLVER_AMG))
    c.close()
    _, c, nd = _scalar(name, order)
    B = np.random.default_rng(7).standard_normal((nd, 8))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def lin(method, ncols, place):
        c.lin_compute(capi.MAT_STIFF, symmetric=True)   # (a fresh handle: the hierarchy starts over)
        flat = np.ascontiguousarray(B[:, :ncols].T).reshape(-1)
        out = flat if place == "in" else np.zeros_like(flat)
        opt, info = capi.Options(method=method, maxit=1000, rtol=1e-10, assembly=0, check_every=0, time_spmv=0), capi.Info()
        rc = c.lib.fdapde_lin_solve(c._ctx, C.byref(opt), dp(flat), ncols, dp(out), C.byref(info))
        if rc not in (capi.OK, capi.ENOCONV):
            c._check(rc)
        return out, info

    for cols in (8, 1):
        c.tune("amg_cols", cols)
        for ncols in (1, 5, 8):
            for place in ("out", "in"):
                attempt(f"lin_solve AMG amg_cols {cols}, {ncols} col {place} place", lambda: lin(capi.SOLVER_AMG, ncols, place))
    c.close()
    for r in rows:
        print("ROW " + json.dumps(r), flush=True)


def time_child(handle):
    rows_out = []
    if handle == "scalar":
        capi, c, nd = _scalar("unit_square_16", 1)
        B = np.random.default_rng(6).standard_normal((nd, 64))
        c.lin_compute(capi.MAT_STIFF, symmetric=True)
        c.lin_solve(B, method=capi.SOLVER_AMG, maxit=1000, raise_on_noconv=False)   # warm-up: buffers, the hierarchy
        t0 = time.perf_counter()
        _, info = c.lin_solve(B, method=capi.SOLVER_AMG, maxit=1000, raise_on_noconv=False)
        rows_out.append({"what": f"unit_square_16 P1, {nd} rows, 64 columns, fdapde_lin_solve AMG", "ms": (time.perf_counter() - t0) * 1e3, "iters": int(info.iters)})
        c.close()
        # one solve at the size of tools/amg_cols_time.py (unit_cube(30), 29 791 DOFs, eight columns side by side)
        from fdapde_core_amd import meshgen

        c = capi.Context(0)
        c.mesh_upload(*meshgen.unit_cube(30))
        nd = c.dofs_build(1)
        c.set_operator(-capi.laplacian() + capi.reaction(1.0))
        c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
        c.init()
        c.lin_compute(capi.MAT_STIFF, symmetric=True)
        B = np.random.default_rng(8).standard_normal((nd, 8))
        c.lin_solve(B, method=capi.SOLVER_AMG)
        t0 = time.perf_counter()
        _, info = c.lin_solve(B, method=capi.SOLVER_AMG)
        rows_out.append({"what": f"unit_cube(30) P1, {nd} rows, 8 columns, fdapde_lin_solve AMG", "ms": (time.perf_counter() - t0) * 1e3, "iters": int(info.iters)})
        c.close()
        for r in rows_out:
            print("ROW " + json.dumps(r), flush=True)
        return
    for name, order, ncols, stages in (("unit_square_16", 1, 64, ("GMRES", "DENSE", "AMG")),):
        capi, c, compute, _, rows = _setup(handle, name, order)
        solve = c.block_solve if handle == "block" else c.kron_solve
        B = np.random.default_rng(6).standard_normal((rows, ncols))
        compute()
        for mname, method in _methods(capi, handle):
            if mname not in stages:
                continue
            solve(B, method=method, maxit=1000, raise_on_noconv=False)   # warm-up: buffers, the inverse, the hierarchy
            t0 = time.perf_counter()
            _, info = solve(B, method=method, maxit=1000, raise_on_noconv=False)
            rows_out.append({"what": f"{name} P{order}, {rows} rows, {ncols} column{'s' if ncols > 1 else ''}, {mname}", "ms": (time.perf_counter() - t0) * 1e3,
                             "iters": int(info.iters)})
        c.close()
    for r in rows_out:
        print("ROW " + json.dumps(r), flush=True)


def _child(args, lib):
    env = dict(os.environ)
    if lib:
        env["FDAPDE_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, env=env, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"a child process failed ({args}, {lib or 'this tree'}): rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return [json.loads(line[4:]) for line in r.stdout.splitlines() if line.startswith("ROW ")]


def bits_main(parent_lib, out_path):
    out = [f"tools/handle_driver_bits.py on an MI355X, {time.strftime('%Y-%m-%d %H:%M:%S')}",
           "x (SHA-256), iters, relres (bits), converged, method_used -- or status and message of a refusal -- of the parent commit's library and this tree's", ""]
    bad = 0
    for handle in ("block", "kron", "scalar"):
        for name, order in FIXTURES:
            for term in ("plain", "term") if handle != "scalar" else ("",):
                args = ["--bits-child", handle, name, str(order), term] if handle != "scalar" else ["--scalar-child", name, str(order)]
                p1, p2, new = _child(args, parent_lib), _child(args, parent_lib), _child(args, None)
                assert len(p1) == len(p2) == len(new) == (16 if handle != "scalar" else 15)
                for a, b, n in zip(p1, p2, new):
                    head = f"{handle:5s} {name} P{order} {term:5s} {a['sub']:28s}"
                    what = f"refused, status {a['status']}" if "status" in a else f"method {a['method_used']}, {a['iters']} iterations, converged {a['converged']}"
                    if a != b:
                        diff = sorted(k for k in a if a[k] != b.get(k))
                        out.append(f"{head}: the parent does not repeat itself ({', '.join(diff)}): not compared")
                        bad += 1
                    elif a == n:
                        out.append(f"{head}: equal ({what})")
                    else:
                        diff = sorted(k for k in a if a[k] != n.get(k))
                        out.append(f"{head}: DIFFERENT in {', '.join(diff)}: parent {json.dumps(a)} | this tree {json.dumps(n)}")
                        bad += 1
                print(f"{handle} {name} P{order} {term}: done", flush=True)
    out += ["", f"{'every line says equal' if bad == 0 else str(bad) + ' lines do NOT say equal'}"]
    text = "\n".join(out) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)
    return 1 if bad else 0


def time_main(parent_lib, out_path):
    out = [f"tools/handle_driver_bits.py --time on an MI355X, {time.strftime('%Y-%m-%d %H:%M:%S')}",
           "wall time of one fdapde_block_solve / fdapde_kron_solve / fdapde_lin_solve call, ms; five windows per library, alternating, every window a fresh process with one warm-up call",
           "the gate: this tree's median <= the largest of the parent's five windows", ""]
    bad = 0
    for handle in ("block", "kron", "scalar"):
        got = {"parent": {}, "new": {}}
        for window in range(5):
            for who, lib in (("parent", parent_lib), ("new", None)):
                for r in _child(["--time-child", handle], lib):
                    got[who].setdefault(r["what"], []).append(r["ms"])
            print(f"{handle}: window {window + 1} of 5 done", flush=True)
        for what in got["parent"]:
            p, n = got["parent"][what], got["new"][what]
            ok = float(np.median(n)) <= max(p)
            bad += 0 if ok else 1
            out.append(f"{handle:5s} {what}: parent {np.median(p):.3f} (smallest {min(p):.3f}, largest {max(p):.3f}) | this tree {np.median(n):.3f} "
                       f"(smallest {min(n):.3f}, largest {max(n):.3f}) -> {'within' if ok else 'OUTSIDE'} the parent's spread")
    out += ["", f"{'every figure within the gate' if bad == 0 else str(bad) + ' figures OUTSIDE the gate'}"]
    text = "\n".join(out) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)
    return 1 if bad else 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] == ["--bits-child"]:
        bits_child(*argv[1:])
    elif argv[:1] == ["--scalar-child"]:
        scalar_child(*argv[1:])
    elif argv[:1] == ["--time-child"]:
        time_child(argv[1])
    elif argv[:1] == ["--time"] and len(argv) >= 2:
        sys.exit(time_main(os.path.abspath(argv[1]), argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "handle_driver_time.txt")))
    elif len(argv) >= 1 and not argv[0].startswith("--"):
        sys.exit(bits_main(os.path.abspath(argv[0]), argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "handle_driver_bits.txt")))
    else:
        raise SystemExit(__doc__)
