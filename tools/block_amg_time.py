#!/usr/bin/env python3
"""FDAPDE_SOLVER_BLOCK_AMG against the block handle's GMRES stage on the two sizes of DESIGN 14's table: nothing here is compared against a gate -- nobody
had measured this before.

  * 2-D P1, unit_square(708): 502 681 DOFs; 3-D P1, unit_cube(118): 1 685 159 DOFs; observations at half of the nodes, lambda 1e-4 and 1e-2, rtol 1e-10.
  * per case: the hierarchy's rows per level (2 n_l) and set-up time (first BLOCK_AMG solve - second), then the host clock around one solve (it ends in a
    stream synchronise) by FDAPDE_SOLVER_BLOCK_AMG under `amg_absorb` 0 and 1 (a context each) and by FDAPDE_SOLVER_GMRES in the same process, alternating,
    five times each -> median, smallest, largest, and the iterations of each.  GMRES(50) is the stage the handle had before, untouched: the baseline.
  * --trace: the 2-D case, lambda 1e-4, one set-up and three solves, nothing else -- what a `rocprofv3 --kernel-trace --stats -- python tools/block_amg_time.py
    --trace` run wraps (the script does not start the profiler itself); --stats DIR OUT appends the top kernels of that run's *kernel_stats.csv to OUT.

usage: block_amg_time.py [OUT]      (OUT defaults to profiles/block_amg_time.txt)
       block_amg_time.py --trace
       block_amg_time.py --stats DIR OUT"""
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
    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen

    if capi.load().fdapde_device_count() < 1:
        raise SystemExit("block_amg_time.py needs a HIP device; a CPU run says nothing about these times")
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
