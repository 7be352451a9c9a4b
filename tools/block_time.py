#!/usr/bin/env python3
"""The 2 x 2 block handle on sizes a user would run: nothing here is compared against a gate -- no earlier number exists for this operator.

  * k_block_spmv (the Krylov stage's operator on D^-1 A): HIP events around REPS launches behind three warm-up launches (fdapde_block_bench_spmv), repeated
    five times -> median, smallest, largest; bytes per launch from the model 36 nnz + 4 (n + 1) + 32 n, and that over the 8 TB/s HBM peak.  Beside it: FOUR
    launches of the scalar SpMV kernel on the same pattern (fdapde_bench_spmv x 4, fused dot partials included: the launch inside CG) -- the only way the
    parent of this change could apply four blocks.  Sizes: C2's (unit_square(708): 502 681 DOFs) and a 3-D P1 space of 1 685 159 DOFs (unit_cube(118)).
  * one smoothing solve (observations at half of the nodes, lambda 1e-4, rtol 1e-10, at most 2 000 iterations of GMRES(50)) at those sizes: iterations and
    the host clock around the call (it ends in a stream synchronise).
  * the dense stage at 2 n = 578 and 2 178 (unit_square_16 / _32): the inversion, then the host clock around calls of one column and of 64.

usage: block_time.py [OUT]      (OUT defaults to profiles/block_time.txt)

block_time.py --obs [OUT] [--parent-lib PATH]   (OUT defaults to profiles/block_obs_time.txt): the factored data term of fdapde_block_set_obs, every measurement
a fresh process, HIP events around 200 operator applications behind 3 warm-ups, the median of five windows:
  (a) the operator with a term live -- areal Psi over 32 x 32 tiles and pointwise Psi of 10^6 random locations on the 2-D mesh, areal Psi over 8^3 tiles on the
      3-D mesh, each under block_obs_team 0 (the rule), 8 and 64: time, bytes by the model of fdapde_block_bench_spmv, rate;
  (b) one GMRES solve of the pointwise smoothing system with the term factored against the same library with fdapde_gram_pointwise's values in a11;
  (c) the guard: the operator with NO term live, this library and the parent commit's (PATH: its libfdapde_hip.so) alternating -- the new median against the
      spread of the parent's five windows."""
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
LAMBDA = 1e-4


def smoothing_blocks(c, capi, n_nodes):
    """the four blocks on the pattern for R1 = stiff() of -laplacian (symmetric: R1^T = R1), R0 = mass(), Psi = the identity's rows at half of the nodes"""
    rp, ci = c.pattern_get()
    nd = len(rp) - 1
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    obs = np.sort(np.random.default_rng(0).choice(n_nodes, n_nodes // 2, replace=False))
    rows = np.repeat(np.arange(nd, dtype=np.int64), np.diff(rp))
    diag_slot = np.flatnonzero(ci == rows)
    assert len(diag_slot) == nd
    a11 = np.zeros(len(ci))
    a11[diag_slot[obs]] = -1.0
    rng = np.random.default_rng(1)
    b = np.zeros(2 * nd)
    b[obs] = -rng.standard_normal(len(obs))
    b[nd:] = LAMBDA * 0.1 * rng.standard_normal(nd)
    return (a11, LAMBDA * r1, LAMBDA * r1, LAMBDA * r0), b, nd, len(ci)


def space(capi, mesh):
    nodes, cells, bnd = mesh
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(1)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.zeros(c.quadrature_nodes().shape[0]))
    c.init()
    return c, nodes.shape[0]


def spread(v):
    return f"{np.median(v):.4f} ms (smallest {min(v):.4f}, largest {max(v):.4f})"


def large(capi, label, mesh, out):
    c, n_nodes = space(capi, mesh)
    blocks, b, nd, nnz = smoothing_blocks(c, capi, n_nodes)
    c.block_compute(*blocks, symmetric=True)
    blk, sca = [], []
    by_blk = by_sca = 0.0
    for _ in range(5):   # the two alternate inside one process
        ms, by_blk = c.block_bench_spmv(200)
        blk.append(ms)
        ms, by_sca = c.bench_spmv(200)
        sca.append(4.0 * ms)
    med = float(np.median(blk))
    out.append(f"{label}: {nd} DOFs, {nnz} pattern entries")
    out.append(f"  k_block_spmv                     {spread(blk)}; {by_blk / 1e6:.1f} MB per launch by the model -> {by_blk / (med * 1e-3) / 1e12:.2f} TB/s, "
               f"{100 * by_blk / (med * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")
    out.append(f"  4 x the scalar SpMV launch       {spread(sca)}; 4 x {by_sca / 1e6:.1f} MB by its model")
    t0 = time.perf_counter()
    x, info = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000, raise_on_noconv=False)
    wall = time.perf_counter() - t0
    out.append(f"  smoothing solve, lambda {LAMBDA:g}:    GMRES(50) iterations {info.iters}, converged {info.converged}, relres {info.relres:.2e}, {1e3 * wall:.1f} ms "
               f"({1e3 * wall / max(info.iters, 1):.3f} ms per iteration)")
    c.close()


def dense(capi, workloads, name, out):
    c, n_nodes = space(capi, workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", name)))
    blocks, b, nd, _ = smoothing_blocks(c, capi, n_nodes)
    c.block_compute(*blocks, symmetric=True)
    t0 = time.perf_counter()
    c.block_solve(b, method=capi.SOLVER_DENSE)
    first = time.perf_counter() - t0
    B = np.random.default_rng(2).standard_normal((2 * nd, 64))
    one, many = [], []
    for _ in range(5):
        c.block_solve(b, method=capi.SOLVER_DENSE), c.block_solve(B, method=capi.SOLVER_DENSE)
    for _ in range(50):
        t0 = time.perf_counter()
        c.block_solve(b, method=capi.SOLVER_DENSE)
        one.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        c.block_solve(B, method=capi.SOLVER_DENSE)
        many.append(1e3 * (time.perf_counter() - t0) / 64)
    x, info = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000, raise_on_noconv=False)
    t0 = time.perf_counter()
    x, info = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000, raise_on_noconv=False)
    gm = 1e3 * (time.perf_counter() - t0)
    out.append(f"{name}: 2 n = {2 * nd}: first dense call (inversion + one column) {1e3 * first:.2f} ms; per column, one per call {spread(one)}; "
               f"per column, 64 per call {spread(many)}; the same column by GMRES(50): {info.iters} iterations, {gm:.2f} ms")
    c.close()


# ---- --obs: the factored data term (fdapde_block_set_obs) -------------------------------------------------------------------------------------------
# Every measurement is a process of its own (--obs-child ...) that prints one JSON line: HIP events around 200 operator applications behind 3 warm-ups
# (fdapde_block_bench_spmv), five windows -> median, smallest, largest.
def _tiles_psi(c, mesh, k):
    """areal Psi over k boxes per axis of the bounding box (a cell belongs to the box of its barycentre), from fdapde_cell_integrals"""
    import ctypes as C

    import scipy.sparse as sp

    nodes, cells, _ = mesh
    bary = nodes[cells].mean(axis=1)
    lo, hi = nodes.min(axis=0), nodes.max(axis=0)
    ijk = np.minimum((k * (bary - lo) / (hi - lo)).astype(np.int64), k - 1)
    box = np.zeros(len(cells), dtype=np.int64)
    for d in range(nodes.shape[1]):
        box = box * k + ijk[:, d]
    ids, region = np.unique(box, return_inverse=True)
    s = c.sizes()
    nb = s["n_basis"]
    meas, pint = np.zeros(len(cells)), np.zeros((len(cells), nb))
    dp = C.POINTER(C.c_double)
    c._check(c.lib.fdapde_cell_integrals(c._ctx, meas.ctypes.data_as(dp), pint.ctypes.data_as(dp)))
    dofs, _, _ = c.dofs_get()
    D = np.bincount(region, weights=meas, minlength=len(ids))
    psi = sp.csr_matrix((pint.reshape(-1) / np.repeat(D[region], nb), (np.repeat(region, nb), dofs.reshape(-1))), shape=(len(ids), s["n_dofs"]))
    psi.sum_duplicates()
    psi.sort_indices()
    return psi


def _pointwise_psi(c, mesh, n_locs):
    import scipy.sparse as sp

    nodes = mesh[0]
    pts = np.random.default_rng(4).uniform(nodes.min(axis=0), nodes.max(axis=0), size=(n_locs, nodes.shape[1]))
    cells, vals = c.eval_pointwise_raw(pts)
    ok = np.flatnonzero(cells >= 0)   # (a location that was not found gives an empty row)
    dofs, _, _ = c.dofs_get()
    nb = vals.shape[1]
    psi = sp.csr_matrix((vals[ok].reshape(-1), (np.repeat(ok, nb), dofs[cells[ok]].reshape(-1))), shape=(n_locs, c.sizes()["n_dofs"]))
    psi.sort_indices()
    return psi, cells, vals


def obs_child(argv):
    """--obs-child KIND MESH TEAM: KIND areal | pointwise (the operator), solve_term | solve_gram (one GMRES solve), guard (no term live)"""
    import json

    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen

    kind, which, team = argv[0], argv[1], int(argv[2])
    mesh = meshgen.unit_square(708) if which == "sq" else meshgen.unit_cube(118)
    c, n_nodes = space(capi, mesh)
    rp, ci = c.pattern_get()
    nd = len(rp) - 1
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    res = {"kind": kind, "mesh": which, "n_dofs": nd, "pattern_nnz": len(ci), "lib": os.path.basename(os.path.dirname(capi.LIB_PATH))}
    if kind == "guard":
        blocks, _, _, _ = smoothing_blocks(c, capi, n_nodes)
        c.block_compute(*blocks, symmetric=True)
    else:
        c.block_compute(None, LAMBDA * r1, LAMBDA * r1, LAMBDA * r0, symmetric=True)
    if kind in ("areal", "pointwise", "solve_term", "solve_gram"):
        if kind == "areal":
            psi = _tiles_psi(c, mesh, 32 if which == "sq" else 8)
        else:
            psi, cells, vals = _pointwise_psi(c, mesh, 1000000)
        res.update(n_obs=psi.shape[0], nnz=int(psi.nnz), longest_row=int(np.diff(psi.indptr).max()), longest_col=int(np.bincount(psi.indices, minlength=nd).max()))
    if kind in ("solve_term", "solve_gram"):
        rng = np.random.default_rng(1)
        b = np.concatenate([-(psi.T @ rng.standard_normal(psi.shape[0])), LAMBDA * 0.1 * rng.standard_normal(nd)])
        t0 = time.perf_counter()
        if kind == "solve_term":
            c.block_set_obs(psi)
        else:
            c.block_compute(-c.gram_pointwise(cells, vals), LAMBDA * r1, LAMBDA * r1, LAMBDA * r0, symmetric=True)
        res["setup_ms"] = 1e3 * (time.perf_counter() - t0)
        c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000, raise_on_noconv=False)   # (warm-up: the work buffers)
        t0 = time.perf_counter()
        x, info = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000, raise_on_noconv=False)
        res.update(solve_ms=1e3 * (time.perf_counter() - t0), iters=info.iters, converged=info.converged, relres=info.relres)
    else:
        if kind != "guard":
            c.tune("block_obs_team", team)
            c.block_set_obs(psi)
            info = c.block_obs_info()
            res.update(team_rows=info["team_rows"], team_cols=info["team_cols"])
        win, by = [], 0.0
        for _ in range(5):
            ms, by = c.block_bench_spmv(200)
            win.append(ms)
        res.update(windows_ms=win, bytes=by)
    c.close()
    print("OBS_RESULT " + json.dumps(res))


def obs_main(out_path, parent_lib):
    import json
    import subprocess

    def child(kind, which, team=0, lib=None):
        env = dict(os.environ)
        if lib:
            env["FDAPDE_HIP_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--obs-child", kind, which, str(team)], capture_output=True, text=True, env=env, timeout=600)
        for line in r.stdout.splitlines():
            if line.startswith("OBS_RESULT "):
                print(line, file=sys.stderr, flush=True)   # (progress)
                return json.loads(line[len("OBS_RESULT "):])
        raise SystemExit(f"child {kind} {which} {team} failed:\n{r.stdout}\n{r.stderr}")

    def op_line(r):
        med = float(np.median(r["windows_ms"]))
        return (f"{spread(r['windows_ms'])}; {r['bytes'] / 1e6:.1f} MB by the model -> {r['bytes'] / (med * 1e-3) / 1e12:.2f} TB/s, "
                f"{100 * r['bytes'] / (med * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")

    out = [f"tools/block_time.py --obs on {socket.gethostname()} (MI355X), {time.strftime('%Y-%m-%d %H:%M:%S')}",
           "HIP events around 200 operator applications behind 3 warm-ups, five windows (median, smallest, largest), every line a process of its own", ""]
    out.append("(a) the Krylov stage's operator with a data term live: k_block_spmv + k_obs_gather + k_obs_scatter")
    base = child("guard", "sq")
    out.append(f"2-D P1, unit_square(708): {base['n_dofs']} DOFs, {base['pattern_nnz']} pattern entries; without a term {op_line(base)}")
    for kind, teams in (("areal", (0, 8, 64)), ("pointwise", (0, 8, 64))):
        for team in teams:
            r = child(kind, "sq", team)
            out.append(f"  {kind:9s} Psi {r['n_obs']} x {r['n_dofs']}, {r['nnz']} entries, longest row {r['longest_row']} / column {r['longest_col']}; block_obs_team {team} -> "
                       f"{r['team_rows']} / {r['team_cols']} lanes: {op_line(r)}")
    base3 = child("guard", "cube")
    out.append(f"3-D P1, unit_cube(118): {base3['n_dofs']} DOFs, {base3['pattern_nnz']} pattern entries; without a term {op_line(base3)}")
    for team in (0, 8, 64):
        r = child("areal", "cube", team)
        out.append(f"  areal     Psi {r['n_obs']} x {r['n_dofs']}, {r['nnz']} entries, longest row {r['longest_row']} / column {r['longest_col']}; block_obs_team {team} -> "
                   f"{r['team_rows']} / {r['team_cols']} lanes: {op_line(r)}")
    out += ["", "(b) one GMRES(50) solve of the pointwise smoothing system (2-D mesh, 10^6 random locations, lambda 1e-4, rtol 1e-10): the term factored against "
            "fdapde_gram_pointwise's values in a11"]
    for kind, label in (("solve_term", "factored (fdapde_block_set_obs)"), ("solve_gram", "on the pattern (fdapde_gram_pointwise)")):
        r = child(kind, "sq")
        out.append(f"  {label:40s} set-up {r['setup_ms']:.1f} ms; iterations {r['iters']}, converged {r['converged']}, relres {r['relres']:.2e}, {r['solve_ms']:.1f} ms "
                   f"({r['solve_ms'] / max(r['iters'], 1):.3f} ms per iteration)")
    out += ["", "(c) the guard: fdapde_block_bench_spmv with NO term live, this library and the parent commit's alternating"]
    if parent_lib:
        for which, pairs in (("sq", 2), ("cube", 1)):
            for _ in range(pairs):
                new, old = child("guard", which), child("guard", which, lib=parent_lib)
                med = float(np.median(new["windows_ms"]))
                inside = min(old["windows_ms"]) <= med <= max(old["windows_ms"])
                out.append(f"  {which:4s} this library {spread(new['windows_ms'])} | the parent's {spread(old['windows_ms'])} -> the new median "
                           f"{'lies within' if inside else 'is OUTSIDE'} the parent's spread")
    else:
        out.append("  (no --parent-lib given: not measured)")
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--obs-child":
        return obs_child(sys.argv[2:])
    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen, workloads

    if capi.load().fdapde_device_count() < 1:
        raise SystemExit("block_time.py needs a HIP device; a CPU run says nothing about these times")
    if len(sys.argv) > 1 and sys.argv[1] == "--obs":
        rest = sys.argv[2:]
        parent = None
        if "--parent-lib" in rest:
            i = rest.index("--parent-lib")
            parent = os.path.abspath(rest[i + 1])
            del rest[i:i + 2]
        return obs_main(rest[0] if rest else os.path.join(ROOT, "profiles", "block_obs_time.txt"), parent)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "block_time.txt")
    out = [f"tools/block_time.py on {socket.gethostname()} (MI355X), {time.strftime('%Y-%m-%d %H:%M:%S')}", ""]
    large(capi, "2-D P1, unit_square(708) (C2's size)", meshgen.unit_square(708), out)
    large(capi, "3-D P1, unit_cube(118)", meshgen.unit_cube(118), out)
    out.append("")
    dense(capi, workloads, "unit_square_16", out)
    dense(capi, workloads, "unit_square_32", out)
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
