#!/usr/bin/env python3
"""fdapde_project (nearest cell + closest point + basis values) on a level-8 sphere (1 310 720 triangles) with 10^6 points, next to
fdapde_eval_pointwise with 10^6 locations on unit_square(810) (1 312 200 triangles), the one comparable figure the project has.

Cases: points moved off the surface by N(0, (h / 2)^2) along the normal (measured locations); points uniform in the bounding box; the sphere's
centre alone (every cell equidistant to rounding: the whole grid is scanned by one lane).

Per case: the first call (builds the bin grid, loads the code object), then WARM + REPS calls of the C ABI, the last REPS timed: the whole call
by the host clock around it (it ends in a stream synchronise: check of the coordinates, upload, kernel, four downloads) and the kernel alone by
device events around the launch (FDAPDE_DEBUG_TIMING=1 makes the library print them on stderr, so the timed calls run in a child process whose
stderr is read here).  Medians, with the smallest and largest.  Nothing is compared against a gate: nobody had measured any of this.

usage: project_time.py [N_POINTS] [OUT]      (OUT defaults to profiles/project_time.txt)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_calls(call, warm, reps, label):
    t0 = time.perf_counter()
    call()
    first = time.perf_counter() - t0
    for _ in range(warm):
        call()
    print("@@MARK " + label, file=sys.stderr, flush=True)   # the kernel lines after this mark belong to the timed calls
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    print("@@END " + label, file=sys.stderr, flush=True)
    return dict(label=label, first_ms=1e3 * first, call_ms=[1e3 * t for t in ts])


def _emit(r):
    print("@@JSON " + json.dumps(r), file=sys.stderr, flush=True)   # (one line per finished case, on the stream the kernel times arrive on)


def child(n):
    import ctypes as C

    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen

    if capi.load().fdapde_device_count() < 1:
        raise SystemExit("project_time.py needs a HIP device; a CPU run says nothing about these times")
    rng = np.random.default_rng(7)
    nodes, cells, bnd = meshgen.unit_sphere_surface(8)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(1)
    e = nodes[cells[:, 1]] - nodes[cells[:, 0]]
    h = float(np.linalg.norm(e, axis=1).mean())
    pick = rng.integers(0, len(cells), n)
    lam = rng.dirichlet(np.ones(3), n)
    on = np.einsum("ij,ijk->ik", lam, nodes[cells[pick]])
    nrm = np.cross(nodes[cells[pick, 1]] - nodes[cells[pick, 0]], nodes[cells[pick, 2]] - nodes[cells[pick, 0]])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    near = on + rng.normal(0.0, 0.5 * h, n)[:, None] * nrm
    box = rng.uniform(nodes.min(axis=0), nodes.max(axis=0), (n, 3))
    nb = c.sizes()["n_basis"]

    def projector(ctx, pts):
        m = len(pts)
        flat = np.ascontiguousarray(pts.T).reshape(-1)
        cid, q, d, v = np.zeros(m, dtype=np.int32), np.zeros(pts.shape[1] * m), np.zeros(m), np.zeros((m, nb))
        return lambda: ctx._check(ctx.lib.fdapde_project(ctx._ctx, C.c_int64(m), capi._dp(flat), capi._ip(cid), capi._dp(q), capi._dp(d), capi._dp(v))), d

    def sphere_case(label, pts, warm, reps):
        call, d = projector(c, pts)
        r = _time_calls(call, warm, reps, label)
        r.update(n=len(pts), cells=int(len(cells)), h=h, mean_dist=float(d.mean()), max_dist=float(d.max()))
        _emit(r)

    sphere_case("near", near, 2, 7)
    sphere_case("centre", np.zeros((1, 3)), 2, 7)
    n2, cells2, bnd2 = meshgen.unit_square(810)
    c2 = capi.Context(0)
    c2.mesh_upload(n2, cells2, bnd2)
    c2.dofs_build(1)
    locs = rng.uniform(0.01, 0.99, (n, 2))
    flat = np.ascontiguousarray(locs.T).reshape(-1)
    cid, v = np.zeros(n, dtype=np.int32), np.zeros((n, 3))
    r = _time_calls(lambda: c2._check(c2.lib.fdapde_eval_pointwise(c2._ctx, C.c_int64(n), capi._dp(flat), capi._ip(cid), capi._dp(v))), 2, 7, "eval_pointwise")
    r.update(n=n, cells=int(len(cells2)), found=int((cid >= 0).sum()))
    _emit(r)
    call, d = projector(c2, locs)   # the same planar locations through fdapde_project (inside: q = p)
    r = _time_calls(call, 2, 7, "project_planar")
    r.update(n=n, cells=int(len(cells2)), max_dist=float(d.max()))
    _emit(r)
    c2.close()
    sphere_case("box", box, 1, 3)   # (last: by far the longest case)
    c.close()


def _med(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:.3f} ({v[0]:.3f} .. {v[-1]:.3f})"


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "project_time.txt")
    env = dict(os.environ, FDAPDE_DEBUG_TIMING="1")
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", str(n)], env=env, stderr=subprocess.PIPE, text=True)
    res, kern, cur = [], {}, None
    for ln in p.stderr:   # echoed as it arrives: a run that is cut short still shows the cases it finished
        sys.stderr.write(ln)
        sys.stderr.flush()
        ln = ln.rstrip("\n")
        if ln.startswith("@@MARK "):
            cur = ln[7:]
            kern[cur] = []
        elif ln.startswith("@@END "):
            cur = None
        elif ln.startswith("@@JSON "):
            res.append(json.loads(ln[7:]))
        elif cur is not None and ln.startswith("[timing] k_"):
            kern[cur].append(float(ln.split()[-2]))
    if p.wait() != 0:
        raise SystemExit(p.returncode)
    by = {r["label"]: r for r in res}
    lines = ["fdapde_project / fdapde_eval_pointwise: ms per call, median (min .. max) of the timed calls; kernel = device events around the launch,",
             "call = host clock around the C ABI call (coordinate check, upload, kernel, downloads, synchronise); first = the first call of the context", ""]
    for r in res:
        extra = ", ".join(f"{k} {r[k]:.4g}" if isinstance(r[k], float) else f"{k} {r[k]}" for k in r if k not in ("label", "first_ms", "call_ms"))
        lines.append(f"{r['label']:<15} kernel {_med(kern[r['label']]):<28} call {_med(r['call_ms']):<30} first {r['first_ms']:.1f}   [{extra}]")
    km = {k: sorted(v)[len(v) // 2] for k, v in kern.items()}
    cm = {k: sorted(by[k]["call_ms"])[len(by[k]["call_ms"]) // 2] for k in by}
    lines += ["", "ratios to fdapde_eval_pointwise on unit_square(810) (kernel / call):"]
    for k in ("near", "box", "project_planar"):
        lines.append(f"  {k:<15} {km[k] / km['eval_pointwise']:.2f} / {cm[k] / cm['eval_pointwise']:.2f}")
    lines.append(f"  centre (1 point, one lane scans the whole grid): kernel {km['centre']:.3f} ms, call {cm['centre']:.3f} ms")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
