#!/usr/bin/env python3
"""1-D meshes at scale: street grids (meshgen.street_grid) of about 1 M and 8 M segments at P1 and P2, and an interval of 10^6 cells at P1.
Per case: fdapde_dofs_build wall time, the first fdapde_init and a warm one (t_assemble_ms: operator + forcing + mass), then -u'' + u = 1 with
zero Dirichlet data at the dead ends (the interval: its two ends) solved under FDAPDE_SOLVER_AUTO and under FDAPDE_SOLVER_AMG (rtol 1e-8,
maxit MAXIT): iterations, solve ms and us per iteration.  A solve that stops at MAXIT is reported as such (Jacobi-CG needs O(n) iterations on a
path graph).  The assembly kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (not written here).
usage: tools/network_time.py [MAXIT] [OUT]    (OUT default profiles/network_time.txt)"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdapde_loader import load_package
capi = load_package().capi
from fdapde_core_amd import meshgen

maxit = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "network_time.txt")
cases = [("grid 1M P1", 1, lambda: meshgen.street_grid(167, 167, k=20, seed=1, drop=0.1)),
         ("grid 1M P2", 2, lambda: meshgen.street_grid(167, 167, k=20, seed=1, drop=0.1)),
         ("grid 8M P1", 1, lambda: meshgen.street_grid(300, 300, k=50, seed=2, drop=0.1)),
         ("grid 8M P2", 2, lambda: meshgen.street_grid(300, 300, k=50, seed=2, drop=0.1)),
         ("interval 1M P1", 1, lambda: meshgen.interval(1_000_000))]
lines = [f"tools/network_time.py: one MI355X, -u'' + u = 1, zero Dirichlet data at the boundary nodes, rtol 1e-8, maxit {maxit}",
         f"{'case':<15} {'cells':>9} {'DOFs':>9} {'dofs_build ms':>13} {'init1 ms':>9} {'init ms':>8} | "
         f"{'AUTO it':>8} {'ms':>9} {'us/it':>7} | {'AMG it':>8} {'ms':>9} {'us/it':>7}"]
cache, notes = {}, []
for name, order, make in cases:
    key = name.split(" P")[0]
    if key not in cache:
        cache.clear()
        cache[key] = make()
    nodes, cells, bnd = cache[key]
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    t0 = time.perf_counter()
    nd = c.dofs_build(order)
    c.synchronize()
    t_dofs = 1e3 * (time.perf_counter() - t0)
    nq = order + 1
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.set_forcing(np.ones(nq * cells.shape[0]))
    c.set_dirichlet(np.zeros(nd))
    c.init()
    t_init1 = c.info().t_assemble_ms
    c.init()
    t_init = c.info().t_assemble_ms
    row = f"{name:<15} {cells.shape[0]:>9} {nd:>9} {t_dofs:>13.1f} {t_init1:>9.3f} {t_init:>8.3f} |"
    for meth in (capi.SOLVER_AUTO, capi.SOLVER_AMG):
        try:
            info = c.solve(method=meth, rtol=1e-8, maxit=maxit, raise_on_noconv=False)
        except capi.FdapdeError as e:   # (recorded, not hidden: the ladder shows which method refuses which system)
            row += f" {'refused':>8} {'-':>9} {'-':>7} |"
            notes.append(f"{name}, {'AUTO' if meth == capi.SOLVER_AUTO else 'AMG'}: {e}")
            continue
        it = f"{info.iters}{'' if info.converged == 1 else '*'}"
        row += f" {it:>8} {info.t_solve_ms:>9.2f} {1e3 * info.t_solve_ms / max(1, info.iters):>7.2f} |"
    lines.append(row.rstrip(" |"))
    print(lines[-1], flush=True)
    c.close()
lines.append("(* = stopped at maxit without reaching rtol; solve ms includes the method's own set-up -- AMG's hierarchy, PMG's coarse level --")
lines.append(" so us/it is solve ms / iterations, not the cost of one iteration alone; AUTO hands order-2 systems from 300 k DOFs to PMG)")
lines += ["refused: " + n for n in notes]
text = "\n".join(lines)
print(text, flush=True)
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write(text + "\n")
