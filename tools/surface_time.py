#!/usr/bin/env python3
"""Surface (Triangulation<2,3>) against planar meshes of the same size, alternated in one process: P1 on a level-8 icosahedral sphere
(655 362 nodes, 1 310 720 triangles, -Lap_S u + u = 3x) against unit_square(810) (1 312 200 triangles, -Lap u + u = 1); P2 on a level-7 sphere
(327 680 triangles, 655 362 DOFs) against unit_square(405) (328 050 triangles).  Per case: fdapde_init time (operator + forcing + mass, one sweep
where it fits), CG iterations and time per iteration (rtol 1e-8), M DOF/s of the solve.  Medians of REPS alternations.
Only the per-launch and per-iteration times compare like with like: the sphere is closed (no Dirichlet rows, f = 3x) and the square has zero
Dirichlet data and f = 1, so the iteration counts -- and with them the M DOF/s column -- differ by the problems, not by the geometry code.
usage: tools/surface_time.py [REPS] [OUT]    (OUT default profiles/surface_time.txt; run it under rocprofv3 --kernel-trace --stats for the kernels)"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdapde_loader import load_package
capi = load_package().capi
from fdapde_core_amd import meshgen

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "surface_time.txt")
cases = [("P1 sphere L8", 1, lambda: meshgen.unit_sphere_surface(8)), ("P1 plane nx810", 1, lambda: meshgen.unit_square(810)),
         ("P2 sphere L7", 2, lambda: meshgen.unit_sphere_surface(7)), ("P2 plane nx405", 2, lambda: meshgen.unit_square(405))]
meshes = {name: make() for name, _, make in cases}
res = {name: [] for name, _, _ in cases}
for r in range(reps):
    for name, order, _ in cases:
        nodes, cells, bnd = meshes[name]
        c = capi.Context(0)
        c.mesh_upload(nodes, cells, bnd)
        nd = c.dofs_build(order)
        qn = c.quadrature_nodes()
        c.set_operator(-capi.laplacian() + capi.reaction(1.0))
        c.set_forcing(3.0 * qn[:, 0] if nodes.shape[1] == 3 else np.ones(qn.shape[0]))
        if nodes.shape[1] == 2:
            c.set_dirichlet(np.zeros(nd))
        c.init()
        t_init = c.info().t_assemble_ms
        info = c.solve(method=capi.SOLVER_CG, rtol=1e-8)
        res[name].append((nd, cells.shape[0], t_init, info.iters, info.t_solve_ms))
        c.close()
lines = [f"tools/surface_time.py: medians of {reps} alternations (rtol 1e-8, Jacobi CG, one MI355X)",
         "(compare init ms and us/iter: the iteration counts, hence M DOF/s, belong to different problems -- closed sphere vs Dirichlet square)",
         f"{'case':<16} {'cells':>9} {'DOFs':>9} {'init ms':>8} {'iters':>6} {'solve ms':>9} {'us/iter':>8} {'M DOF/s':>8}"]
for name, _, _ in cases:
    a = np.array(res[name], dtype=float)
    nd, nc = int(a[0, 0]), int(a[0, 1])
    ti, it, ts = np.median(a[:, 2]), np.median(a[:, 3]), np.median(a[:, 4])
    lines.append(f"{name:<16} {nc:>9} {nd:>9} {ti:>8.3f} {int(it):>6} {ts:>9.2f} {1e3 * ts / it:>8.2f} {nd / ts / 1e3:>8.1f}")
text = "\n".join(lines)
print(text, flush=True)
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write(text + "\n")
