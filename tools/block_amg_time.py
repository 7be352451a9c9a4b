#!/usr/bin/env python3
"""FDAPDE_SOLVER_BLOCK_AMG against the block handle's GMRES stage on the two sizes of DESIGN 14's table: nothing here is compared against a gate -- nobody
had measured this before.

  * 2-D P1, unit_square(708): 502 681 DOFs; 3-D P1, unit_cube(118): 1 685 159 DOFs; observations at half of the nodes, lambda 1e-4 and 1e-2, rtol 1e-10.
  * per case: the hierarchy's rows per level (2 n_l) and set-up time (first BLOCK_AMG solve - second), then the host clock around one solve (it ends in a
    stream synchronise) by FDAPDE_SOLVER_BLOCK_AMG under `amg_absorb` 0 and 1 (a context each) and by FDAPDE_SOLVER_GMRES in the same process, alternating,
    five times each -> median, smallest, largest, and the iterations of each.  GMRES(50) is the stage the handle had before, untouched: the baseline.
  * --trace: the 2-D case, lambda 1e-4, one set-up and three solves, nothing else -- what a `rocprofv3 --kernel-trace --stats -- python tools/block_amg_time.py
    --trace` run wraps (the script does not start the profiler itself); --stats DIR OUT appends the top kernels of that run's *kernel_stats.csv to OUT.

  * --obs: the stage with the factored data term carried through the hierarchy (knob block_amg_obs = 1) on the three inputs of profiles/block_obs_time.txt --
    2-D areal 32 x 32 tiles, the same mesh with 10^6 random points, 3-D areal 8^3 tiles --, lambda 1e-2 and 1e-4, `amg_absorb` 1 and the default, against the
    GMRES(50) stage of the same handle, measured the same way (median of 5 alternating, set-up = first solve - second): iterations, ms per solve and per outer
    iteration, the set-up split into the pattern hierarchy and the term's share (FDAPDE_DEBUG_SETUP's line, read back from stderr), nnz(Psi_l) per level, the
    launches the term adds per outer iteration.  --obs-guard PARENT_LIB: the NO-term solves of this tool by this library and by the parent commit's
    (a path to its libfdapde_hip.so), a process each, alternating: the new median must lie inside the parent's spread.
  * --driver-guard PARENT_LIB: the handle's solve path against the parent commit's -- one FDAPDE_SOLVER_GMRES and one FDAPDE_SOLVER_BLOCK_AMG solve of this
    tool's own systems (no term, lambda 1e-4), five windows per process, the two libraries alternating twice; the gate: this library's median is at most the
    largest of the parent's windows.  Appends to profiles/handle_driver_time.txt.

usage: block_amg_time.py [OUT]      (OUT defaults to profiles/block_amg_time.txt)
       block_amg_time.py --trace
       block_amg_time.py --stats DIR OUT
       block_amg_time.py --obs [OUT] [sq-areal|sq-points|cube-areal ...]      (OUT defaults to profiles/block_obs_amg_time.txt; appends)
       block_amg_time.py --obs-guard PARENT_LIB [OUT]
       block_amg_time.py --driver-guard PARENT_LIB [OUT [sq|cube ...]]"""
import csv
import glob
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def smoothing_blocks(c, capi, n_nodes, lam):
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
    b[nd:] = lam * 0.1 * rng.standard_normal(nd)
    return (a11, lam * r1, lam * r1, lam * r0), b, nd


def space(capi, mesh, absorb=2):
    nodes, cells, bnd = mesh
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(1)
    c.tune("amg_absorb", absorb)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.zeros(c.quadrature_nodes().shape[0]))
    c.init()
    return c, nodes.shape[0]


def spread(v):
    return f"{np.median(v):.1f} ms (smallest {min(v):.1f}, largest {max(v):.1f})"


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def case(capi, arms, n_nodes, lam, out):
    """arms: {amg_absorb: context}; the GMRES stage runs on the first of them"""
    amg, live = {}, {}
    for absorb, c in arms.items():
        blocks, b, nd = smoothing_blocks(c, capi, n_nodes, lam)
        c.block_compute(*blocks, symmetric=True)
        amg[absorb] = lambda c=c, b=b: c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=1e-10, raise_on_noconv=False)
    c0 = next(iter(arms.values()))
    gm = lambda: c0.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000, raise_on_noconv=False)
    out.append(f"  lambda {lam:g}:")
    for absorb, c in arms.items():
        try:
            _, t_first = timed(amg[absorb])
        except capi.FdapdeError as e:   # (a refusal is a result too)
            out.append(f"    amg_absorb {absorb}: FDAPDE_SOLVER_BLOCK_AMG refused: {e}")
            continue
        _, t_second = timed(amg[absorb])
        h = c.amg_hierarchy(capi.AMG_OF_BLOCK)
        live[absorb] = f"rows per level {' / '.join(str(r) for r in h['rows'])}; set-up {t_first - t_second:.1f} ms (first solve {t_first:.1f} - second {t_second:.1f})"
    gm()   # (its buffers are allocated by the first call)
    t_amg, i_amg, t_gm, i_gm = {absorb: [] for absorb in live}, {}, [], None
    for _ in range(5):
        for absorb in live:
            (_, i_amg[absorb]), t = timed(amg[absorb])
            t_amg[absorb].append(t)
        (_, i_gm), t = timed(gm)
        t_gm.append(t)
    for absorb in live:
        i, t = i_amg[absorb], t_amg[absorb]
        out.append(f"    amg_absorb {absorb}: {live[absorb]}")
        out.append(f"      FDAPDE_SOLVER_BLOCK_AMG {i.iters} iterations, converged {i.converged}, relres {i.relres:.2e} (unscaled), {spread(t)}, "
                   f"{np.median(t) / max(i.iters, 1):.2f} ms per iteration; against GMRES {np.median(t) / np.median(t_gm):.2f} x the time")
    out.append(f"    FDAPDE_SOLVER_GMRES       {i_gm.iters} iterations, converged {i_gm.converged}, relres {i_gm.relres:.2e} (D^-1-scaled), {spread(t_gm)}, "
               f"{np.median(t_gm) / max(i_gm.iters, 1):.2f} ms per iteration")


# ---- --obs: the data term carried through the hierarchy ------------------------------------------------------------------------------------------
def term_launches(levels):
    """launches the term adds per outer iteration of a hierarchy of `levels` levels: level m < levels - 1 is cycled 2^m times (the K-cycle), each cycle adds
    k_obs_gather + k_obs_scatter behind the restriction and k_obs_gather_acc + k_obs_scatter behind the post-smoothing; each of the 2^m products y = A x of a
    level 1 <= m < levels - 1 adds k_obs_gather + k_obs_scatter_store; the outer iteration's own product adds two"""
    return sum(4 * 2 ** m for m in range(levels - 1)) + sum(2 * 2 ** m for m in range(1, levels - 1)) + 2


def _stderr_of(fn):
    """run fn with the process's stderr (the library writes FDAPDE_DEBUG_SETUP's line there) captured -> (result, text)"""
    import tempfile

    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            r = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return r, tmp.read().decode(errors="replace")


def obs_case(capi, arms, psi, lam, out):
    import re

    amg, live = {}, {}
    for absorb, c in arms.items():
        rp, ci = c.pattern_get()
        nd = len(rp) - 1
        r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
        c.block_compute(None, lam * r1, lam * r1, lam * r0, symmetric=True)
        t0 = time.perf_counter()
        c.block_set_obs(psi)
        t_set = 1e3 * (time.perf_counter() - t0)
        rng = np.random.default_rng(1)
        b = np.concatenate([-(psi.T @ rng.standard_normal(psi.shape[0])), lam * 0.1 * rng.standard_normal(nd)])
        amg[absorb] = lambda c=c, b=b: c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=1e-10, raise_on_noconv=False)
    c0 = next(iter(arms.values()))
    gm = lambda: c0.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000, raise_on_noconv=False)
    out.append(f"  lambda {lam:g} (fdapde_block_set_obs {t_set:.1f} ms):")
    os.environ["FDAPDE_DEBUG_SETUP"] = "1"
    for absorb, c in arms.items():
        try:
            (_, t_first), err = _stderr_of(lambda: timed(amg[absorb]))
        except capi.FdapdeError as e:   # (a refusal is a result too)
            out.append(f"    amg_absorb {absorb}: FDAPDE_SOLVER_BLOCK_AMG refused: {e}")
            continue
        _, t_second = timed(amg[absorb])
        h, lv = c.amg_hierarchy(capi.AMG_OF_BLOCK), c.block_amg_obs_levels()
        m = re.search(r"set-up ([0-9.]+) ms \(the data term ([0-9.]+)\)", err)
        split = f"of the build's {float(m.group(1)):.1f} ms the pattern hierarchy {float(m.group(1)) - float(m.group(2)):.1f}, the term (coarsening on the host, uploads, g_l) {float(m.group(2)):.1f}" if m else "no split reported"
        live[absorb] = (f"rows per level {' / '.join(str(r) for r in h['rows'])}; nnz(Psi_l) {' / '.join(str(z) for z in lv['nnz'])}; lanes {lv['team_rows']} / {lv['team_cols']}; "
                        f"set-up {t_first - t_second:.1f} ms (first solve {t_first:.1f} - second {t_second:.1f}; {split}); the term adds {term_launches(len(h['rows']))} launches per outer iteration")
    del os.environ["FDAPDE_DEBUG_SETUP"]
    gm()
    t_amg, i_amg, t_gm, i_gm = {absorb: [] for absorb in live}, {}, [], None
    for _ in range(5):
        for absorb in live:
            (_, i_amg[absorb]), t = timed(amg[absorb])
            t_amg[absorb].append(t)
        (_, i_gm), t = timed(gm)
        t_gm.append(t)
    for absorb in live:
        i, t = i_amg[absorb], t_amg[absorb]
        out.append(f"    amg_absorb {absorb}: {live[absorb]}")
        out.append(f"      FDAPDE_SOLVER_BLOCK_AMG {i.iters} iterations, converged {i.converged}, relres {i.relres:.2e} (unscaled), {spread(t)}, "
                   f"{np.median(t) / max(i.iters, 1):.2f} ms per iteration; against GMRES {np.median(t) / np.median(t_gm):.2f} x the time")
    out.append(f"    FDAPDE_SOLVER_GMRES       {i_gm.iters} iterations, converged {i_gm.converged}, relres {i_gm.relres:.2e} (D^-1-scaled), {spread(t_gm)}, "
               f"{np.median(t_gm) / max(i_gm.iters, 1):.2f} ms per iteration")


OBS_INPUTS = {"sq-areal": ("2-D P1, unit_square(708), areal 32 x 32 tiles", "sq", ("tiles", 32)),
              "sq-points": ("2-D P1, unit_square(708), 10^6 random points", "sq", ("points", 1000000)),
              "cube-areal": ("3-D P1, unit_cube(118), areal 8^3 tiles", "cube", ("tiles", 8))}


def obs_main(capi, meshgen, out_path, which):
    import block_time as bt   # (the designs of profiles/block_obs_time.txt)

    out = [f"tools/block_amg_time.py --obs on {socket.gethostname()} (MI355X), {time.strftime('%Y-%m-%d %H:%M:%S')}",
           "host clock around one solve (it ends in a stream synchronise), median of 5 alternating (smallest, largest); block_amg_obs = 1, rtol 1e-10", ""]
    for name in which:
        label, mesh_kind, (design, size) = OBS_INPUTS[name]
        mesh = meshgen.unit_square(708) if mesh_kind == "sq" else meshgen.unit_cube(118)
        arms = {absorb: space(capi, mesh, absorb)[0] for absorb in (1, 2)}
        for c in arms.values():
            c.tune("block_amg_obs", 1)
        c0 = arms[1]
        psi = bt._tiles_psi(c0, mesh, size) if design == "tiles" else bt._pointwise_psi(c0, mesh, size)[0]
        del mesh
        out.append(f"{label}: {c0.sizes()['n_dofs']} DOFs; Psi {psi.shape[0]} x {psi.shape[1]}, {psi.nnz} entries, longest row {int(np.diff(psi.indptr).max())}")
        for lam in (1e-2, 1e-4):
            at = len(out)
            obs_case(capi, arms, psi, lam, out)
            print("\n".join(out[at - 1 if lam == 1e-2 else at:]), flush=True)
        for c in arms.values():
            c.close()
        out.append("")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as fh:
        fh.write("\n".join(out) + "\n")


def guard_child(which):
    """five NO-term BLOCK_AMG solves (lambda 1e-4, amg_absorb at its default) of this tool's own system -> one GUARD_RESULT line"""
    import json

    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen

    c, n_nodes = space(capi, meshgen.unit_square(708) if which == "sq" else meshgen.unit_cube(118))
    blocks, b, _ = smoothing_blocks(c, capi, n_nodes, 1e-4)
    c.block_compute(*blocks, symmetric=True)
    solve = lambda: c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=1e-10, raise_on_noconv=False)
    solve(), solve()
    times = []
    for _ in range(5):
        (_, info), t = timed(solve)
        times.append(t)
    c.close()
    print("GUARD_RESULT " + json.dumps({"ms": times, "iters": info.iters, "lib": capi.LIB_PATH}))


def driver_guard_child(which):
    """five GMRES and five BLOCK_AMG solves (no term, lambda 1e-4) of this tool's own system, each behind two warm-up solves -> one GUARD_RESULT line"""
    import json

    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen

    c, n_nodes = space(capi, meshgen.unit_square(708) if which == "sq" else meshgen.unit_cube(118))
    blocks, b, _ = smoothing_blocks(c, capi, n_nodes, 1e-4)
    c.block_compute(*blocks, symmetric=True)
    res = {"lib": capi.LIB_PATH}
    for name, method, maxit in (("GMRES", capi.SOLVER_GMRES, 2000), ("BLOCK_AMG", capi.SOLVER_BLOCK_AMG, 200)):
        solve = lambda: c.block_solve(b, method=method, rtol=1e-10, maxit=maxit, raise_on_noconv=False)
        solve(), solve()
        times = []
        for _ in range(5):
            (_, info), t = timed(solve)
            times.append(t)
        res[name] = {"ms": times, "iters": info.iters}
    c.close()
    print("GUARD_RESULT " + json.dumps(res))


def driver_guard_main(parent_lib, out_path, tool=__file__, cases=("sq", "cube"), what="fdapde_block_solve, this tool's systems (no term, lambda 1e-4)"):
    """shared with kron_time.py --driver-guard (tool: the script whose --driver-guard-child runs a case)"""
    import json
    import subprocess

    def child(which, lib):
        env = dict(os.environ)
        if lib:
            env["FDAPDE_HIP_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(tool), "--driver-guard-child", which], capture_output=True, text=True, env=env, timeout=600)
        for line in r.stdout.splitlines():
            if line.startswith("GUARD_RESULT "):
                return json.loads(line[len("GUARD_RESULT "):])
        raise SystemExit(f"guard child {which} failed:\n{r.stdout}\n{r.stderr}")

    out = ["", f"tools/{os.path.basename(tool)} --driver-guard on an MI355X, {time.strftime('%Y-%m-%d %H:%M:%S')}",
           f"one solve of {what}, wall time of the call, ms; this library and the parent commit's, a process each, alternating twice, five windows per process",
           "the gate: this library's median <= the largest of the parent's windows"]
    bad = 0
    for which in cases:
        new, old = {}, {}
        for _ in range(2):
            for got, lib in ((new, None), (old, parent_lib)):
                r = child(which, lib)
                assert lib is None or os.path.samefile(r.pop("lib"), parent_lib), "the parent's library ran"
                r.pop("lib", None)
                for name, v in r.items():
                    got.setdefault(name, {"ms": [], "iters": v["iters"]})["ms"] += v["ms"]
        for name in new:
            assert new[name]["iters"] == old[name]["iters"], "the same count from both libraries"
            ok = float(np.median(new[name]["ms"])) <= max(old[name]["ms"])
            bad += 0 if ok else 1
            out.append(f"  {which:4s} {name:16s} {new[name]['iters']} iterations: this library {spread(new[name]['ms'])} | the parent's {spread(old[name]['ms'])} -> "
                       f"{'within' if ok else 'OUTSIDE'} the gate")
    print("\n".join(out), flush=True)
    with open(out_path, "a") as fh:
        fh.write("\n".join(out) + "\n")
    return 1 if bad else 0


def guard_main(parent_lib, out_path):
    import json
    import subprocess

    def child(which, lib):
        env = dict(os.environ)
        if lib:
            env["FDAPDE_HIP_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child", which], capture_output=True, text=True, env=env, timeout=600)
        for line in r.stdout.splitlines():
            if line.startswith("GUARD_RESULT "):
                return json.loads(line[len("GUARD_RESULT "):])
        raise SystemExit(f"guard child {which} failed:\n{r.stdout}\n{r.stderr}")

    out = [f"tools/block_amg_time.py --obs-guard on {socket.gethostname()} (MI355X), {time.strftime('%Y-%m-%d %H:%M:%S')}",
           "the guard: one FDAPDE_SOLVER_BLOCK_AMG solve with NO term live (lambda 1e-4, this tool's system), this library and the parent commit's, a process each, alternating twice, 5 solves per process"]
    for which in ("sq", "cube"):
        new, old, it = [], [], None
        for _ in range(2):
            r = child(which, None)
            new += r["ms"]
            it = r["iters"]
            r = child(which, parent_lib)
            old += r["ms"]
            assert os.path.samefile(r["lib"], parent_lib) and r["iters"] == it, "the parent's library ran, with the same count"
        inside = min(old) <= np.median(new) <= max(old)
        out.append(f"  {which:4s} {it} iterations: this library {spread(new)} | the parent's {spread(old)} -> the new median {'lies within' if inside else 'is OUTSIDE'} the parent's spread")
    print("\n".join(out), flush=True)
    with open(out_path, "a") as fh:
        fh.write("\n".join(out) + "\n")


def append_stats(directory, out_path, top=10):
    found = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not found:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    with open(found[0], newline="") as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    lines = ["kernel trace of the 2-D case, lambda 1e-4 (one set-up, three solves): kernel, calls, total ms, average us, share"]
    for r in rows[:top]:
        lines.append(f"  {r['Name'][:90]:<90} {int(r['Calls']):>7} {float(r['TotalDurationNs']) / 1e6:>9.2f} {float(r['AverageNs']) / 1e3:>8.2f} {float(r['Percentage']):>6.2f} %")
    with open(out_path, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--stats":
        return append_stats(sys.argv[2], sys.argv[3])
    default_obs = os.path.join(ROOT, "profiles", "block_obs_amg_time.txt")
    if len(sys.argv) == 3 and sys.argv[1] == "--guard-child":
        return guard_child(sys.argv[2])
    if len(sys.argv) == 3 and sys.argv[1] == "--driver-guard-child":
        return driver_guard_child(sys.argv[2])
    if len(sys.argv) >= 3 and sys.argv[1] == "--driver-guard":
        return driver_guard_main(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "handle_driver_time.txt"),
                                 cases=tuple(sys.argv[4:]) or ("sq", "cube"))
    if len(sys.argv) >= 3 and sys.argv[1] == "--obs-guard":
        return guard_main(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else default_obs)
    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen

    if capi.load().fdapde_device_count() < 1:
        raise SystemExit("block_amg_time.py needs a HIP device; a CPU run says nothing about these times")
    if len(sys.argv) > 1 and sys.argv[1] == "--obs":
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        names = [a for a in sys.argv[2:] if a in OBS_INPUTS]
        paths = [a for a in sys.argv[2:] if a not in OBS_INPUTS]
        return obs_main(capi, meshgen, paths[0] if paths else default_obs, names or list(OBS_INPUTS))
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        c, n_nodes = space(capi, meshgen.unit_square(708))
        blocks, b, _ = smoothing_blocks(c, capi, n_nodes, 1e-4)
        c.block_compute(*blocks, symmetric=True)
        for _ in range(3):
            _, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG, rtol=1e-10, raise_on_noconv=False)
        print(f"trace run: {info.iters} iterations per solve, converged {info.converged}")
        c.close()
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "block_amg_time.txt")
    out = [f"tools/block_amg_time.py on {socket.gethostname()} (MI355X), {time.strftime('%Y-%m-%d %H:%M:%S')}", ""]
    for label, mesh in (("2-D P1, unit_square(708) (C2's size)", lambda: meshgen.unit_square(708)), ("3-D P1, unit_cube(118)", lambda: meshgen.unit_cube(118))):
        m = mesh()
        arms = {absorb: space(capi, m, absorb)[0] for absorb in (0, 1)}
        n_nodes = m[0].shape[0]
        del m
        out.append(f"{label}: {arms[0].sizes()['n_dofs']} DOFs, 2 n = {2 * arms[0].sizes()['n_dofs']}")
        for lam in (1e-4, 1e-2):
            at = len(out)
            case(capi, arms, n_nodes, lam, out)
            print("\n".join(out[at:]), flush=True)
        for c in arms.values():
            c.close()
        out.append("")
    text = "\n".join(out)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
