#!/usr/bin/env python3
"""Single-launch CG: blocks by recursive coordinate bisection (knob persist_partition 1) against contiguous chunks of the internal order
(knob 0) and the automatic choice (2), alternated on ONE context per system: iterations, microseconds per iteration of the launch (HIP events
around the dispatch), bytes the layout streams per iteration, the in-kernel phase stamps, and the wall time of the layout's construction
(fdapde_solver_prepare after the knob changed).  Sizes: C3 and the systems the choice must not slow down.
usage: persist_partition_ab.py [c3] [c2] [3d60] [3d105] [2d1400] [wide]   (default: all)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdapde_loader import load_package

capi = load_package().capi
from fdapde_core_amd import meshgen   # noqa: E402

CASES = {"c3": (3, 119), "c2": (2, 708), "3d60": (3, 60), "3d105": (3, 105), "2d1400": (2, 1400), "wide": (3, 132)}   # wide: 133^3 = 2.35 M DOFs


def run(name, dim, nx, reps=3):
    nodes, cells, bnd = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
    _, f = meshgen.manufactured(dim)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    c.set_operator(-capi.laplacian())
    c.set_forcing(f(c.quadrature_nodes()))
    c.set_dirichlet(np.zeros(nd))
    c.init()
    c.solve(rtol=1e-10)
    print(f"{name}: {dim}-D nx {nx}, {nd} DOFs", flush=True)
    for rep in range(reps):
        for knob in (0, 1) if rep < reps - 1 else (0, 1, 2):
            c.tune("persist_partition", knob)
            t0 = time.perf_counter()
            c.solver_prepare(True)
            c.synchronize()
            t_prep = 1e3 * (time.perf_counter() - t0)
            c.solve(rtol=1e-10)
            us = []
            for _ in range(3):
                i = c.solve(rtol=1e-10, time_spmv=32)
                us.append(1e3 * i.launch_ms / max(i.iters, 1))
            lay = c.solver_layout_kind(True)
            print(f"  partition={knob}: {i.iters} it  {min(us):.3f} / {sorted(us)[1]:.3f} / {max(us):.3f} us/it (min / median / max of 3)  "
                  f"{c.solver_layout(True)[2]:.0f} B/it  operator slowest {1e3 * i.spmv_avg_ms:.2f} mean {1e3 * i.spmv_mean_ms:.2f} "
                  f"allgather {1e3 * i.gather_avg_ms:.2f} update {1e3 * i.update_avg_ms:.2f} us  kind={lay['kind']} sym={lay['sym']} "
                  f"G={lay['workgroups']} R={lay['rows_per_thread']}  layout built in {t_prep:.1f} ms  persistent={i.persistent}", flush=True)
    c.close()


if __name__ == "__main__":
    for name in (sys.argv[1:] or list(CASES)):
        run(name, *CASES[name])
