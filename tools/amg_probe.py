"""FDAPDE_SOLVER_AMG (csrc/eng_amg.hip) against the path the open method takes today, case by case on one GPU: the hierarchy (levels, rows per level,
operator complexity), set-up ms (first solve minus second), solve ms and iterations, and the same system through FDAPDE_SOLVER_AUTO (or, for C5's P2 operator,
FDAPDE_SOLVER_PMG; for the handle, the handle's existing path per column).  Wall-clock host times around each call.  -> profiles/amg_probe.txt

    python tools/amg_probe.py [--cases all | c2,c3,...] [--absorb 2 | 0,1 | ...]

--absorb: the values of the knob `amg_absorb` to run every elliptic case with, one context per value in the same process; the timed solves of the arms
alternate, five each (median, smallest, largest).  The hierarchy comes from fdapde_amg_hierarchy; the cost of the build `amg_absorb` 2 discards comes from the
FDAPDE_DEBUG_SETUP line (stderr of the library, caught per call)."""
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


ABSORB = [2]   # --absorb


def amg_line(h):
    return (f"{len(h['rows'])} levels, rows {' / '.join(str(r) for r in h['rows'])}, op. complexity {sum(h['nnz']) / h['nnz'][0]:.3f}, "
            f"absorbed {h['absorbed']}")


def elliptic(name, dim, nx, order, op, compare=capi.SOLVER_AUTO):
    nodes, cells, bnd = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
    arms = {}
    for absorb in ABSORB:
        c = capi.Context(0)
        c.mesh_upload(nodes, cells, bnd)
        nd = c.dofs_build(order)
        c.tune("amg_absorb", absorb)
        c.set_operator(op)
        c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
        c.set_dirichlet(np.zeros(nd))
        c.init()
        arms[absorb] = c
    del nodes, cells
    built, u = {}, None
    for absorb, c in arms.items():
        os.environ["FDAPDE_DEBUG_SETUP"] = "1"
        try:
            with CaptureStderr() as cap:
                first, t_first = timed(lambda: c.solve(method=capi.SOLVER_AMG, raise_on_noconv=False))
        except capi.FdapdeError as e:   # (a case the solver refuses is a result too)
            print(f"{name:<34} {nd:>9} | amg_absorb {absorb} | refused: {e}", flush=True)
            continue
        finally:
            del os.environ["FDAPDE_DEBUG_SETUP"]
        _, t_second = timed(lambda: c.solve(method=capi.SOLVER_AMG, raise_on_noconv=False))
        discarded = re.findall(r"discarded build ([\d.]+) ms", cap.text)
        built[absorb] = (c.amg_hierarchy(), t_first - t_second, float(discarded[-1]) if discarded else 0.0)
        u = c.solution()
    times, last = {absorb: [] for absorb in built}, {}
    for _ in range(5):   # the arms alternate
        for absorb in built:
            last[absorb], t = timed(lambda: arms[absorb].solve(method=capi.SOLVER_AMG, raise_on_noconv=False))
            times[absorb].append(t)
    c = next(iter(arms.values()))
    c.solve(method=compare, raise_on_noconv=False)   # (warm: its own layouts, the two-level solver's coarse level)
    other, t_other = timed(lambda: c.solve(method=compare, raise_on_noconv=False))
    diff = np.linalg.norm(c.solution() - u) / max(np.linalg.norm(u), 1e-300) if u is not None else float("nan")
    cmp_name = {capi.SOLVER_AUTO: "open method", capi.SOLVER_PMG: "PMG"}[compare]
    for absorb, (h, t_setup, discarded) in built.items():
        t, info = times[absorb], last[absorb]
        print(f"{name:<34} {nd:>9} | amg_absorb {absorb} | {amg_line(h):<76} | set-up {t_setup:8.1f} ms (of it the discarded build {discarded:6.1f})  "
              f"solve {np.median(t):8.1f} ms (smallest {min(t):.1f}, largest {max(t):.1f})  {info.iters:>4} it {'ok' if info.converged else 'NO CONV'}", flush=True)
    print(f"{name:<34} {nd:>9} | {cmp_name} (method {other.method_used}) {t_other:8.1f} ms {other.iters:>5} it {'ok' if other.converged else 'NO CONV'} | "
          f"rel. diff to the last multilevel arm {diff:.1e}", flush=True)
    for c in arms.values():
        c.close()


def handle(nx, cols=8):
    nodes, cells, bnd = meshgen.unit_square(nx)
    for absorb in ABSORB:   # (one arm after the other: every column is a solve of its own)
        c = capi.Context(0)
        c.mesh_upload(nodes, cells, bnd)
        nd = c.dofs_build(1)
        c.tune("amg_absorb", absorb)
        c.set_operator(-capi.laplacian() + capi.reaction(1.0))
        c.set_forcing(np.ones(3 * cells.shape[0]))
        c.init()
        B = np.random.default_rng(3).standard_normal((nd, cols))
        c.lin_compute(capi.MAT_STIFF)
        (_, i1), t1 = timed(lambda: c.lin_solve(B[:, 0], method=capi.SOLVER_AMG))   # (builds the hierarchy)
        (_, ia), ta = timed(lambda: c.lin_solve(B, method=capi.SOLVER_AMG))
        h = c.amg_hierarchy(capi.AMG_OF_HANDLE)
        c.lin_solve(B[:, 0])
        (_, ib), tb = timed(lambda: c.lin_solve(B))
        c.close()
        print(f"{'handle, 2-D P1 -Lap + 1':<34} {nd:>9} | amg_absorb {absorb} | {amg_line(h)} | set-up + 1st column {t1:8.2f} ms | AMG {ta / cols:7.3f} ms per column "
              f"({ia.iters / cols:.1f} it) | existing handle path (method {ib.method_used}) {tb / cols:7.3f} ms per column", flush=True)


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
    ap.add_argument("--absorb", default="2")
    a = ap.parse_args()
    ABSORB[:] = [int(v) for v in a.absorb.split(",")]
    names = list(CASES) if a.cases == "all" else a.cases.split(",")
    print("case                                    DOFs | knob | hierarchy | FDAPDE_SOLVER_AMG (set-up = first solve - second; five solves) -- then today's path and |u_amg - u_other| / |u_amg|")
    for n in names:
        try:
            CASES[n]()
        except capi.FdapdeError as e:   # (a case the solver refuses is a result too)
            print(f"{n:<34} refused: {e}", flush=True)
