"""FDAPDE_SOLVER_AMG (csrc/eng_amg.hip) against the path the open method takes today, case by case on one GPU: the hierarchy (levels, rows per level,
operator complexity), set-up ms (first solve minus second), solve ms and iterations, and the same system through FDAPDE_SOLVER_AUTO (or, for C5's P2 operator,
FDAPDE_SOLVER_PMG; for the handle, the handle's existing path per column).  Wall-clock host times around each call.  -> profiles/amg_probe.txt

    python tools/amg_probe.py [--cases all | c2,c3,...]

The hierarchy's line comes from FDAPDE_DEBUG_SETUP (stderr of the library, caught per call)."""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdapde_loader import load_package

load_package()
from fdapde_core_amd import capi, meshgen, workloads


class CaptureStderr:
    """the library's stderr lines of one call (file descriptor 2, not sys.stderr)"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def amg_line(text):
    m = re.findall(r"amg: (\d+) levels, rows ([\d / ]+), operator complexity ([\d.]+)", text)
    return f"{m[-1][0]} levels, rows {m[-1][1]}, op. complexity {m[-1][2]}" if m else "-"


def elliptic(name, dim, nx, order, op, compare=capi.SOLVER_AUTO):
    nodes, cells, bnd = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(order)
    del nodes, cells
    c.set_operator(op)
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.set_dirichlet(np.zeros(nd))
    c.init()
    os.environ["FDAPDE_DEBUG_SETUP"] = "1"
    try:
        with CaptureStderr() as cap:
            first, t_first = timed(lambda: c.solve(method=capi.SOLVER_AMG, raise_on_noconv=False))
    finally:
        del os.environ["FDAPDE_DEBUG_SETUP"]
    second, t_second = timed(lambda: c.solve(method=capi.SOLVER_AMG, raise_on_noconv=False))
    u = c.solution()
    c.solve(method=compare, raise_on_noconv=False)   # (warm: its own layouts, the two-level solver's coarse level)
    other, t_other = timed(lambda: c.solve(method=compare, raise_on_noconv=False))
    diff = np.linalg.norm(c.solution() - u) / max(np.linalg.norm(u), 1e-300)
    c.close()
    cmp_name = {capi.SOLVER_AUTO: "open method", capi.SOLVER_PMG: "PMG"}[compare]
    print(f"{name:<34} {nd:>9} | {amg_line(cap.text):<62} | set-up {t_first - t_second:8.1f} ms  solve {t_second:8.1f} ms  {second.iters:>4} it "
          f"{'ok' if second.converged else 'NO CONV'} | {cmp_name} (method {other.method_used}) {t_other:8.1f} ms {other.iters:>5} it "
          f"{'ok' if other.converged else 'NO CONV'} | rel. diff {diff:.1e}", flush=True)


def handle(nx, cols=8):
    nodes, cells, bnd = meshgen.unit_square(nx)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.set_forcing(np.ones(3 * cells.shape[0]))
    c.init()
    B = np.random.default_rng(3).standard_normal((nd, cols))
    c.lin_compute(capi.MAT_STIFF)
    (_, i1), t1 = timed(lambda: c.lin_solve(B[:, 0], method=capi.SOLVER_AMG))   # (builds the hierarchy)
    (_, ia), ta = timed(lambda: c.lin_solve(B, method=capi.SOLVER_AMG))
    c.lin_solve(B[:, 0])
    (_, ib), tb = timed(lambda: c.lin_solve(B))
    c.close()
    print(f"{'handle, 2-D P1 -Lap + 1':<34} {nd:>9} | set-up + 1st column {t1:8.2f} ms | AMG {ta / cols:7.3f} ms per column ({ia.iters / cols:.1f} it) | "
          f"existing handle path (method {ib.method_used}) {tb / cols:7.3f} ms per column", flush=True)


CASES = {
    "p1_2d_66k": lambda: elliptic("2-D P1 -Lap", 2, 256, 1, -capi.laplacian()),
    "p1_2d_263k": lambda: elliptic("2-D P1 -Lap", 2, 512, 1, -capi.laplacian()),
    "c2": lambda: elliptic("C2: 2-D P1 -Lap", 2, 708, 1, -capi.laplacian()),
    "p1_3d_275k": lambda: elliptic("3-D P1 -Lap", 3, 64, 1, -capi.laplacian()),
    "c3": lambda: elliptic("C3: 3-D P1 -Lap", 3, 119, 1, -capi.laplacian()),
    "large": lambda: elliptic("large_8p1M: 3-D P1 -Lap", 3, 200, 1, -capi.laplacian()),
    "handle": lambda: [handle(nx) for nx in (90, 128, 256)],
    # cell Peclet |b| h / 2 at h = 1 / 128
    "pe150": lambda: elliptic("2-D P1 -Lap + b.grad + 1, Pe 150", 2, 128, 1,
                              -capi.laplacian() + capi.advection(list(2.0 * 150 * 128 * np.array([1.0, 0.5]) / np.sqrt(1.25))) + capi.reaction(1.0)),
    "pe1000": lambda: elliptic("2-D P1 -Lap + b.grad + 1, Pe 1000", 2, 128, 1,
                               -capi.laplacian() + capi.advection(list(2.0 * 1000 * 128 * np.array([1.0, 0.5]) / np.sqrt(1.25))) + capi.reaction(1.0)),
    "c5_2m": lambda: elliptic("C5 operator, 3-D P2", 3, 64, 2, workloads.c5_operator(capi), compare=capi.SOLVER_PMG),
}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="all")
    a = ap.parse_args()
    names = list(CASES) if a.cases == "all" else a.cases.split(",")
    print("case                                    DOFs | hierarchy | FDAPDE_SOLVER_AMG (set-up = first solve - second) | today's path | |u_amg - u_other| / |u_amg|")
    for n in names:
        try:
            CASES[n]()
        except capi.FdapdeError as e:   # (a case the solver refuses is a result too)
            print(f"{n:<34} refused: {e}", flush=True)
