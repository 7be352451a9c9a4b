#!/usr/bin/env python3
"""What solving the columns of a multilevel handle solve side by side buys (knob `amg_cols`): wall time per column of fdapde_lin_solve under FDAPDE_SOLVER_AMG
and of fdapde_block_solve under FDAPDE_SOLVER_BLOCK_AMG with n_rhs = 8, at `amg_cols` = 1, 2, 4, 8.

  * 3-D P1 on unit_cube(30 / 66 / 118): 29 791, 300 763 and 1 685 159 DOFs.  The scalar handle holds the stiffness matrix of -Lap + 1, the block handle the
    smoothing system with observations at half of the nodes, lambda 1e-2; eight standard-normal columns, rtol 1e-10.
  * the baseline is `amg_cols` = 1 in the same process on the same hierarchy: the knob does not rebuild it, and 1 is the column-by-column path.
  * per arm: the host clock around one solve of the eight columns (it ends in a stream synchronise), after a warm-up solve of every arm (the hierarchy built, every
    buffer allocated); the arms alternate, five rounds (--rounds) -> median, smallest, largest, divided by eight.  The iterations are the same in every arm (the
    columns' iterates are the same bits), so the ratio is the ratio of the work's cost.

usage: amg_cols_time.py [--sizes 30,66,118] [--rounds 5] [OUT]      (OUT defaults to profiles/amg_cols.txt; it is appended to size by size)"""
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARMS = (1, 2, 4, 8)
N_RHS = 8


def smoothing_blocks(c, capi, n_nodes, lam):
    """the four blocks on the pattern for R1 = stiff() of -laplacian (symmetric), R0 = mass(), Psi = the identity's rows at half of the nodes"""
    rp, ci = c.pattern_get()
    nd = len(rp) - 1
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    obs = np.sort(np.random.default_rng(0).choice(n_nodes, n_nodes // 2, replace=False))
    rows = np.repeat(np.arange(nd, dtype=np.int64), np.diff(rp))
    diag_slot = np.flatnonzero(ci == rows)
    a11 = np.zeros(len(ci))
    a11[diag_slot[obs]] = -1.0
    return (a11, lam * r1, lam * r1, lam * r0), nd


def measure(solve, tune, rounds):
    """solve(): one call on the eight columns -> info; -> {arm: (times in ms, iterations)}"""
    t, its = {a: [] for a in ARMS}, {}
    for a in ARMS:   # warm-up: every arm's buffers
        tune(a)
        solve()
    for _ in range(rounds):
        for a in ARMS:
            tune(a)
            t0 = time.perf_counter()
            info = solve()
            t[a].append(1e3 * (time.perf_counter() - t0))
            its[a] = (info.iters, info.converged)
    return t, its


def report(name, t, its, out):
    base = np.median(t[1]) / N_RHS
    for a in ARMS:
        per = np.array(t[a]) / N_RHS
        out.append(f"    {name} amg_cols {a}: {np.median(per):8.2f} ms per column (smallest {per.min():.2f}, largest {per.max():.2f}); {its[a][0]} iterations summed, "
                   f"converged {its[a][1]}; {np.median(per) / base:.2f} x amg_cols 1")


def main():
    args = sys.argv[1:]
    sizes, rounds = (30, 66, 118), 5
    while args and args[0].startswith("--"):
        if args[0] == "--sizes":
            sizes = tuple(int(s) for s in args[1].split(","))
        elif args[0] == "--rounds":
            rounds = max(5, int(args[1]))
        else:
            raise SystemExit(__doc__)
        args = args[2:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "amg_cols.txt")
    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen

    if capi.load().fdapde_device_count() < 1:
        raise SystemExit("amg_cols_time.py needs a HIP device; a CPU run says nothing about these times")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as fh:
        fh.write(f"tools/amg_cols_time.py on {socket.gethostname()} (MI355X), {time.strftime('%Y-%m-%d %H:%M:%S')}: n_rhs = {N_RHS}, rtol 1e-10, median of {rounds}\n")
    for nx in sizes:
        nodes, cells, bnd = meshgen.unit_cube(nx)
        c = capi.Context(0)
        c.mesh_upload(nodes, cells, bnd)
        nd = c.dofs_build(1)
        n_nodes = nodes.shape[0]
        del nodes, cells, bnd
        c.set_operator(-capi.laplacian() + capi.reaction(1.0))
        c.set_forcing(np.zeros(c.quadrature_nodes().shape[0]))
        c.init()
        out = [f"  3-D P1, unit_cube({nx}): {nd} DOFs"]
        tune = lambda a: c.tune("amg_cols", a)
        # the scalar handle
        c.lin_compute(capi.MAT_STIFF, symmetric=True)
        B = np.random.default_rng(7).standard_normal((nd, N_RHS))
        t, its = measure(lambda: c.lin_solve(B, method=capi.SOLVER_AMG, rtol=1e-10, raise_on_noconv=False)[1], tune, rounds)
        h = c.amg_hierarchy(capi.AMG_OF_HANDLE)
        out.append(f"    FDAPDE_SOLVER_AMG: rows per level {' / '.join(str(r) for r in h['rows'])}, absorbed {h['absorbed']}")
        report("fdapde_lin_solve  ", t, its, out)
        # the block handle
        c.set_operator(-capi.laplacian())
        c.init()
        blocks, _ = smoothing_blocks(c, capi, n_nodes, 1e-2)
        c.block_compute(*blocks, symmetric=True)
        B2 = np.random.default_rng(8).standard_normal((2 * nd, N_RHS))
        t, its = measure(lambda: c.block_solve(B2, method=capi.SOLVER_BLOCK_AMG, rtol=1e-10, raise_on_noconv=False)[1], tune, rounds)
        h = c.amg_hierarchy(capi.AMG_OF_BLOCK)
        out.append(f"    FDAPDE_SOLVER_BLOCK_AMG: rows per level {' / '.join(str(r) for r in h['rows'])}, absorbed {h['absorbed']}")
        report("fdapde_block_solve", t, its, out)
        c.close()
        print("\n".join(out), flush=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
