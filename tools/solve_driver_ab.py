#!/usr/bin/env python3
"""Bit identity of the multi-launch solve driver (csrc/eng_solve.hip: solve_run, fdapde_solve_parabolic, fdapde_lin_solve) between two builds of the library
-> profiles/solve_driver_ab.txt

    FDAPDE_HIP_LIB=tools/bin/variants/libfdapde_hip_parent.so python tools/solve_driver_ab.py run parent.npz      (one process per library)
    python tools/solve_driver_ab.py run new.npz
    python tools/solve_driver_ab.py compare parent.npz new.npz

`run` solves the cases below and stores, per case, the solution(s), the return code and the status text, iters / relres / converged / method_used / persistent /
spmv_timed and fdapde_solver_trace; `compare` holds every array of the second file to the first with np.array_equal and ends with "<k> arrays differ".
Under rocprofv3 --kernel-trace --hip-trace the line "case <name>" on stdout and a fdapde_synchronize in front of every case cut the traces into cases.

elliptic   cube16 and sq24p2 (tests/krylov_systems.py) with non-zero Dirichlet data, persist 0, blocked 0 and 2: CG, single-reduction CG, BiCGStab (the `adv`
           systems), GMRES by name, the open method, fused CG at (cgf_lazy 0 / 1) x (use_graph 0 / 1 at check_every 2) -- each at maxit 7 (FDAPDE_ENOCONV)
           and converged; fused CG with time_spmv 4; cube16 without Dirichlet data; at the defaults the single launch (cube16), the one-workgroup front kernel
           (sq20, second solve) and the single-launch BiCGStab (cube16adv)
stages     -Lap - 300 on unit_cube(8): a CG breakdown, then BiCGStab; cell Peclet 1000 on unit_square(32) at dense_rows 0 (BiCGStab restarts, then the GMRES
           stage) and at the default dense_rows (the direct stage)
parabolic  6 steps with time-varying Dirichlet data: the Krylov steps, FDAPDE_SOLVER_AMG, FDAPDE_SOLVER_PMG on unit_square(20) P2, FDAPDE_SOLVER_DENSE at
           dense_fold 1 and 0, and M / dt + A indefinite (tests/test_gpu_indefinite.py): a CG breakdown inside a step
handle     sq60: 1, 3 and 11 columns at persist 0 (a batch of 8 plus the rest) and at the defaults (side by side, two workgroups per column); x aliasing b;
           the direct single column on unit_square(16), one workgroup (converged; maxit 7) and on -Lap - 150 on unit_square(24) handed over as symmetric
           (CG named: the breakdown reported; the open method: the retry as BiCGStab); the 3-D P2 mass matrix handed over as symmetric (the retry as
           BiCGStab behind the column forms); dense_after reached on the second call
The element-partitioned and row-distributed arms are not here: tests/test_gpu_dist.py and tests/test_gpu_partition.py are their check."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def record(out, c, name, rc, info, x):
    """one case: the arrays of the npz file and a line on stdout"""
    tr = c.solver_trace()
    text = c.lib.fdapde_last_error(c._ctx).decode()
    out[name + ".x"] = np.asarray(x)
    out[name + ".counts"] = np.array([rc, info.iters, info.converged, info.method_used, info.persistent, info.spmv_timed, tr["small_front"], tr["graph_replays"]],
                                     dtype=np.int64)
    out[name + ".relres"] = np.array([info.relres])
    out[name + ".text"] = np.array([text if rc else ""])
    print(f"     -> rc {rc} iterations {info.iters} converged {info.converged} method {info.method_used} persistent {info.persistent} timed {info.spmv_timed} "
          f"front {tr['small_front']} replays {tr['graph_replays']} relres {info.relres:.3e}{' [' + text + ']' if rc else ''}", flush=True)


def begin(c, name):
    c.synchronize()
    print(f"case {name}", flush=True)


def solve(out, c, capi, name, method=0, rtol=1e-9, maxit=0, check_every=0, time_spmv=0):
    begin(c, name)
    opt = capi.Options(method=method, maxit=maxit, rtol=rtol, assembly=0, check_every=check_every, time_spmv=time_spmv)
    info = capi.Info()
    rc = c.lib.fdapde_solve(c._ctx, C.byref(opt), C.byref(info))
    record(out, c, name, rc, info, c.solution() if rc in (capi.OK, capi.ENOCONV) else np.zeros(0))


def lin_solve(out, c, capi, name, B, method=0, rtol=1e-9, maxit=0, inplace=False):
    begin(c, name)
    buf = np.ascontiguousarray(np.asarray(B, dtype=float).reshape(B.shape[0], -1).T)   # (column-major n_dofs x n_rhs, as the ABI wants it)
    x = buf if inplace else np.zeros_like(buf)
    opt = capi.Options(method=method, maxit=maxit, rtol=rtol, assembly=0, check_every=0, time_spmv=0)
    info = capi.Info()
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = c.lib.fdapde_lin_solve(c._ctx, C.byref(opt), ptr(buf), buf.shape[0], ptr(x), C.byref(info))
    record(out, c, name, rc, info, x)
    return info


def parabolic(out, c, capi, name, times, u0, G, method=0, rtol=1e-10):
    begin(c, name)
    nd = u0.size
    g = np.ascontiguousarray(G.T).reshape(-1)
    sol = np.zeros(nd * times.size)
    opt = capi.Options(method=method, maxit=0, rtol=rtol, assembly=0, check_every=0, time_spmv=0)
    info = capi.Info()
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = c.lib.fdapde_solve_parabolic(c._ctx, C.byref(opt), int(times.size), C.c_double(times[1] - times[0]), ptr(np.ascontiguousarray(u0)), ptr(g), ptr(sol),
                                      C.byref(info))
    record(out, c, name, rc, info, sol)


def context(capi, mesh, order, op, forcing=None, dirichlet=True, **knobs):
    c = capi.Context(0)
    c.mesh_upload(*mesh)
    c.dofs_build(order)
    coords = c.dofs_get()[2]
    c.set_operator(op)
    qn = c.quadrature_nodes()
    c.set_forcing(forcing(qn) if forcing else np.cos(3.0 * qn[:, 0]) + qn[:, 1] + 0.5)
    if dirichlet:
        c.set_dirichlet(0.3 * np.cos(2.0 * coords[:, 0]) + coords[:, -1])
    c.init()
    for k, v in knobs.items():
        c.tune(k, v)
    return c, coords


def system(capi, meshgen, name, **kw):
    import krylov_systems as ks

    s = ks.spec_of(name)
    return context(capi, ks.mesh_of(meshgen, s), s["order"], ks.operator_of(capi, s), **kw)


def elliptic_cases(capi, meshgen, out):
    for name in ("cube16", "sq24p2"):
        for blocked in (0, 2):
            tag = f"ell.{name}.b{blocked}"
            c, _ = system(capi, meshgen, name, persist=0, blocked=blocked, dense_rows=0)
            for mname in ("CG", "CG_SR", "GMRES", "AUTO"):
                for maxit in (7, 0):
                    solve(out, c, capi, f"{tag}.{mname}.maxit{maxit}", method=getattr(capi, "SOLVER_" + mname), maxit=maxit)
            for lazy in (0, 1):
                for graph in (0, 1):
                    c.tune("cgf_lazy", lazy)
                    c.tune("use_graph", graph)
                    for maxit in (7, 0):
                        solve(out, c, capi, f"{tag}.CG_FUSED.lazy{lazy}.graph{graph}.maxit{maxit}", method=capi.SOLVER_CG_FUSED, maxit=maxit, check_every=2 if graph else 0)
            if name == "cube16" and blocked == 0:
                solve(out, c, capi, f"{tag}.CG_FUSED.time_spmv4", method=capi.SOLVER_CG_FUSED, time_spmv=4)
            c.close()
            c, _ = system(capi, meshgen, name + "adv", persist=0, blocked=blocked, dense_rows=0)
            for maxit in (7, 0):
                solve(out, c, capi, f"{tag}.BICGSTAB.maxit{maxit}", method=capi.SOLVER_BICGSTAB, maxit=maxit)
            c.close()
    c, _ = system(capi, meshgen, "cube16", dirichlet=False, persist=0, blocked=0)
    solve(out, c, capi, "ell.cube16.no_dirichlet")
    c.close()
    c, _ = system(capi, meshgen, "cube16")
    solve(out, c, capi, "ell.cube16.single_launch")
    c.close()
    c, _ = system(capi, meshgen, "sq20")
    solve(out, c, capi, "ell.sq20.first")   # (a context's first solve builds the layout's column table and leaves the front to the separate kernels)
    solve(out, c, capi, "ell.sq20.front")
    c.close()
    c, _ = system(capi, meshgen, "cube16adv")
    solve(out, c, capi, "ell.cube16adv.single_launch_bicgstab")
    c.close()


def stage_cases(capi, meshgen, out):
    _, f2 = meshgen.manufactured(2)
    _, f3 = meshgen.manufactured(3)
    c, _ = context(capi, meshgen.unit_cube(8), 1, -capi.laplacian() + capi.reaction(-300.0), forcing=f3)
    solve(out, c, capi, "stage.cg_breakdown", rtol=1e-10)
    c.close()
    d = np.array([1.0, 0.5])
    op = -capi.laplacian() + capi.advection((2.0 * 1000.0 * 32 / np.linalg.norm(d)) * d)   # cell Peclet number |b| h / 2 = 1000
    c, _ = context(capi, meshgen.unit_square(32), 1, op, forcing=f2, dense_rows=0)
    solve(out, c, capi, "stage.peclet1000.gmres", rtol=1e-10)
    c.close()
    c, _ = context(capi, meshgen.unit_square(32), 1, op, forcing=f2)
    solve(out, c, capi, "stage.peclet1000.direct", rtol=1e-10)
    c.close()


def stepper(capi, mesh, order, op, times, **knobs):
    c = capi.Context(0)
    c.mesh_upload(*mesh)
    c.dofs_build(order)
    coords = c.dofs_get()[2]
    qn = c.quadrature_nodes()
    c.set_operator(op)
    c.set_forcing(np.stack([np.sin(2.0 * qn[:, 0]) * (1.0 + t) for t in times], axis=1))
    c.init()
    for k, v in knobs.items():
        c.tune(k, v)
    u0 = np.cos(coords[:, 0]) * coords[:, 1]
    G = np.stack([0.1 * np.sin(coords[:, 0] + 3.0 * t) for t in times], axis=1)
    return c, u0, G


def parabolic_cases(capi, meshgen, out):
    times = np.linspace(0.0, 0.3, 7)   # 6 steps
    adr = capi.dt() - capi.laplacian() + capi.advection([1.0, -0.5])
    c, u0, G = stepper(capi, meshgen.unit_square(24), 1, adr, times, dense_rows=0)
    parabolic(out, c, capi, "par.krylov", times, u0, G)
    parabolic(out, c, capi, "par.amg", times, u0, G, method=capi.SOLVER_AMG)
    c.close()
    c, u0, G = stepper(capi, meshgen.unit_square(20), 2, adr, times, dense_rows=0)
    parabolic(out, c, capi, "par.pmg", times, u0, G, method=capi.SOLVER_PMG, rtol=1e-11)
    c.close()
    for fold in (1, 0):
        c, u0, G = stepper(capi, meshgen.unit_square(24), 1, adr, times, dense_fold=fold)
        parabolic(out, c, capi, f"par.dense.fold{fold}", times, u0, G, method=capi.SOLVER_DENSE)
        c.close()
    times = np.linspace(0.0, 0.12, 7)   # dt = 0.02: 50 M - 150 M + K is indefinite
    c, u0, G = stepper(capi, meshgen.unit_square(24), 1, capi.dt() - capi.laplacian() + capi.reaction(-150.0), times, dense_rows=0)
    parabolic(out, c, capi, "par.indefinite", times, u0, G, rtol=1e-11)
    c.close()


def handle_cases(capi, meshgen, out):
    import krylov_systems as ks

    for arm, knobs in (("persist0", dict(persist=0, dense_rows=0)), ("default", dict(dense_rows=0))):
        c, coords = context(capi, meshgen.unit_square(60), 1, -capi.laplacian() + capi.reaction(0.4), dirichlet=False, **knobs)
        c.lin_compute(capi.MAT_STIFF, symmetric=True)
        for cols in (1, 3, 11):
            lin_solve(out, c, capi, f"lin.{arm}.cols{cols}", ks.handle_rhs(coords, cols, 3))
        if arm == "default":
            lin_solve(out, c, capi, "lin.default.inplace", ks.handle_rhs(coords, 3, 4), inplace=True)
        c.close()
    # the 3-D P2 mass matrix is not positive definite (negative quadrature weight): CG breaks down, every column again with BiCGStab
    c, coords = context(capi, meshgen.unit_cube(5), 2, -capi.laplacian() + capi.reaction(1.0), dirichlet=False, dense_rows=0)
    c.lin_compute(capi.MAT_MASS, symmetric=True)
    lin_solve(out, c, capi, "lin.retry_as_bicgstab", ks.handle_rhs(coords, 3, 5), rtol=1e-10)
    c.close()
    # ONE column against a system of one workgroup (at most 2048 rows; no Dirichlet data): the direct single column (run_persist_direct) -- converged, out of
    # iterations, and on an indefinite matrix handed over as symmetric: the breakdown reported where CG was named, the retry as BiCGStab where the method is open
    c, coords = context(capi, meshgen.unit_square(16), 1, -capi.laplacian() + capi.reaction(0.4), dirichlet=False, dense_rows=0)
    c.lin_compute(capi.MAT_STIFF, symmetric=True)
    for name, maxit in (("lin.direct.cols1", 0), ("lin.direct.cols1.maxit7", 7)):
        info = lin_solve(out, c, capi, name, ks.handle_rhs(coords, 1, 8), maxit=maxit)
        assert info.persistent == 1 and info.t_solve_ms == 0.0, "the direct single column leaves t_solve_ms at 0: this case must run it"
    c.close()
    c, coords = context(capi, meshgen.unit_square(24), 1, -capi.laplacian() + capi.reaction(-150.0), dirichlet=False, dense_rows=0)
    c.lin_compute(capi.MAT_STIFF, symmetric=True)
    info = lin_solve(out, c, capi, "lin.direct.breakdown.cg_named", ks.handle_rhs(coords, 1, 9), method=capi.SOLVER_CG_FUSED, rtol=1e-10)
    assert info.persistent == 1 and info.t_solve_ms == 0.0 and info.converged == 0
    lin_solve(out, c, capi, "lin.direct.breakdown.retry", ks.handle_rhs(coords, 1, 9), rtol=1e-10)
    c.close()
    # rent or buy: the first call's columns are Krylov runs (multi-launch: several times the 0.25 ms that half an inversion of 289 rows costs), the second call inverts
    c, coords = context(capi, meshgen.unit_square(16), 1, -capi.laplacian() + capi.reaction(0.4), dirichlet=False, persist=0, dense_after=2)
    c.lin_compute(capi.MAT_STIFF, symmetric=True)
    lin_solve(out, c, capi, "lin.dense_after.first", ks.handle_rhs(coords, 3, 6))
    lin_solve(out, c, capi, "lin.dense_after.second", ks.handle_rhs(coords, 3, 7))
    c.close()


def run(path):
    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen

    if capi.load().fdapde_device_count() < 1:
        raise SystemExit("solve_driver_ab.py needs a HIP device")
    print(f"library: {capi.LIB_PATH}", flush=True)
    out = {}
    elliptic_cases(capi, meshgen, out)
    stage_cases(capi, meshgen, out)
    parabolic_cases(capi, meshgen, out)
    handle_cases(capi, meshgen, out)
    np.savez(path, **out)
    print(f"{len(out) // 4} cases -> {path}", flush=True)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    differ = 0
    for k in sorted(set(a.files) | set(b.files)):
        same = k in a.files and k in b.files and np.array_equal(a[k], b[k])
        differ += 0 if same else 1
        if not same or k.endswith(".x"):
            shape = "x".join(str(s) for s in a[k].shape) if k in a.files else "-"
            print(f"{k:<58} {shape:>10} {'array_equal' if same else 'DIFFERS'}")
    print(f"{len(set(a.files) | set(b.files))} arrays compared, {differ} arrays differ")
    return differ


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    else:
        raise SystemExit(__doc__)
