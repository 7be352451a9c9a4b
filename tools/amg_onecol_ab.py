#!/usr/bin/env python3
"""Bit identity of the multilevel and two-level solvers between two builds of the library: the single-column path as the one-column instantiation of the column
kernels (csrc/eng_amg.hip, csrc/kernels_block.h) and of the flexible GMRES (fgmres_outer, csrc/eng_pmg.hip) against a parent commit's hand-written single-column
forms.  -> section 1 of profiles/amg_onecol_ab.txt and of profiles/fgmres_onecol_ab.txt

    FDAPDE_HIP_LIB=tools/bin/variants/libfdapde_hip_parent.so python tools/amg_onecol_ab.py run parent.npz      (one process per library)
    python tools/amg_onecol_ab.py run new.npz
    python tools/amg_onecol_ab.py compare parent.npz new.npz

`run` solves the cases below and stores, per case, the iteration count, relres and the solution vectors; `compare` holds every array of the second file to the
first with np.array_equal and ends with "<k> arrays differ".

  scalar2d      fdapde_solve, FDAPDE_SOLVER_AMG: unit_square(32) P1 -Lap with Dirichlet data, amg_coarse_rows 256
  scalar3d      fdapde_solve: unit_cube(16) P1 -Lap + 2 with Dirichlet data, amg_absorb 1
  handle        fdapde_lin_solve: the stiffness matrix of -Lap + 2 on unit_square(48), 11 columns at amg_cols 1 and 8 (8 + 2 + 1)
  handle_adr    ... of -Lap + b.grad + 1 handed over as non-symmetric (GCR corrections)
  handle_dense  ... on unit_square(12): 169 DOFs, the hierarchy is the dense level alone
  block         fdapde_block_solve, FDAPDE_SOLVER_BLOCK_AMG: the smoothing system of unit_square(32), lambda 1e-4, 11 columns at amg_cols 1 and 8
  parabolic     fdapde_solve_parabolic stepping with FDAPDE_SOLVER_AMG: unit_square(48) P1, 12 steps with Dirichlet data
  pmg.*         fdapde_solve, FDAPDE_SOLVER_PMG: unit_cube(9) P2, C5's operator with Dirichlet data -- at the default knobs, pmg_restart 5 (restarts),
                pmg_smooth 0 (the additive form), pmg_blocked 0 and 1, and pmg_smooth 0 with pmg_blocked 0 (the x update without dinv)
  pmg_indefinite, pmg_budget12   ... by name where the coarse level does not help (tests/test_gpu_pmg.py): -Lap - 300 on unit_cube(8), FDAPDE_ENOCONV at maxit; -Lap +
                b.grad + 1 on unit_square(60) with pmg_inner_maxit 12
  pmg_stop, pmg_stop2d   ... -Lap - 300 on unit_cube(8) with pmg_inner_maxit 3 and on unit_square(60): four coarse solves in a row get nowhere, the preconditioner raises
                `stop`, the iterate keeps the vectors of the cycle so far -- FDAPDE_ENOCONV, "the coarse level's solves do not converge"
  pmg_parabolic fdapde_solve_parabolic stepping with FDAPDE_SOLVER_PMG: unit_square(20) P2, 6 steps with Dirichlet data (warm starts)
amg_setup_check 1 and amg_coarse_rows 256 throughout the multilevel cases, as the tests: every hierarchy but handle_dense's has three levels."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def context(capi, meshgen, dim, nx, coarse_rows=256, **knobs):
    nodes, cells, bnd = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    c.tune("amg_setup_check", 1)
    c.tune("amg_coarse_rows", coarse_rows)
    for k, v in knobs.items():
        c.tune(k, v)
    return c, nd, nodes.shape[0]


def solve_case(capi, meshgen, out, name, dim, nx, op, **kw):
    c, nd, _ = context(capi, meshgen, dim, nx, **kw)
    coords = c.dofs_get()[2]
    c.set_operator(op)
    qn = c.quadrature_nodes()
    c.set_forcing(1.0 + np.sin(3.0 * qn[:, 0]) * qn[:, 1])
    c.set_dirichlet(0.3 * np.cos(2.0 * coords[:, 0]) + coords[:, -1])
    c.init()
    info = c.solve(method=capi.SOLVER_AMG, rtol=1e-11)
    record(out, name, info, c.solution(), c.amg_hierarchy())
    c.close()


def record(out, name, info, x, h):
    out[name + ".counts"] = np.array([info.iters, info.converged], dtype=np.int64)
    out[name + ".relres"] = np.array([info.relres])
    out[name + ".x"] = np.asarray(x)
    print(f"{name:<22} rows {h['rows'] if h else '(the stepper keeps its hierarchy to itself)'} iterations {info.iters} converged {info.converged} relres {info.relres:.3e}", flush=True)


def columns(n, n_rhs=11):
    """columns that stop at different iterations: a unit vector, zeros, one scaled by 1e-150, the rest standard normal"""
    B = np.random.default_rng(7).standard_normal((n, n_rhs))
    B[:, 1] = 0.0
    B[n // 2, 1] = 1.0
    B[:, 2] = 0.0
    B[:, 3] *= 1e-150
    return B


def handle_case(capi, meshgen, out, name, nx, op, symmetric):
    c, nd, _ = context(capi, meshgen, 2, nx)
    c.set_operator(op)
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    c.lin_compute(capi.MAT_STIFF, symmetric=symmetric)
    B = columns(nd)
    for arm, cols in (("cols1", 1), ("cols8", 8), ("cols1_again", 1)):   # (the last arm: column by column after batches on the same hierarchy)
        c.tune("amg_cols", cols)
        X, info = c.lin_solve(B, method=capi.SOLVER_AMG, rtol=1e-10, raise_on_noconv=False)
        record(out, f"{name}.{arm}", info, X, c.amg_hierarchy(capi.AMG_OF_HANDLE))
    c.close()


def block_case(capi, meshgen, out):
    from amg_cols_time import smoothing_blocks

    c, nd, n_nodes = context(capi, meshgen, 2, 32)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    blocks, _ = smoothing_blocks(c, capi, n_nodes, 1e-4)
    c.block_compute(*blocks, symmetric=True)
    B = columns(2 * nd)
    for arm, cols in (("cols1", 1), ("cols8", 8), ("cols1_again", 1)):
        c.tune("amg_cols", cols)
        X, info = c.block_solve(B, method=capi.SOLVER_BLOCK_AMG, rtol=1e-10, raise_on_noconv=False)
        record(out, f"block.{arm}", info, X, c.amg_hierarchy(capi.AMG_OF_BLOCK))
    c.close()


def parabolic_case(capi, meshgen, out):
    c, nd, _ = context(capi, meshgen, 2, 48)
    coords = c.dofs_get()[2]
    c.set_operator(-capi.laplacian() + capi.advection([1.0, 0.5]) + capi.dt())
    times = np.linspace(0.0, 0.6, 12)
    qn = c.quadrature_nodes()
    c.set_forcing(np.stack([np.sin(2.0 * qn[:, 0]) * (1.0 + t) for t in times], axis=1))
    c.init()
    u0 = np.sin(np.pi * coords[:, 0]) * np.sin(np.pi * coords[:, 1])
    g = np.stack([0.1 * t * coords[:, 0] for t in times], axis=1)
    U, info = c.solve_parabolic(times, u0, dirichlet=g, method=capi.SOLVER_AMG, rtol=1e-12)
    record(out, "parabolic", info, U, None)
    c.close()


def record_pmg(out, name, info, x):
    out[name + ".counts"] = np.array([info.iters, info.converged, info.method_used], dtype=np.int64)
    out[name + ".relres"] = np.array([info.relres])
    out[name + ".x"] = np.asarray(x)
    print(f"{name:<22} iterations {info.iters} converged {info.converged} method {info.method_used} relres {info.relres:.3e}", flush=True)


def pmg_context(capi, meshgen, dim, nx, op, zero=False, **knobs):
    nodes, cells, bnd = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(2)
    c.tune("pmg_setup_check", 1)
    coords = c.dofs_get()[2]
    c.set_operator(op)
    qn = c.quadrature_nodes()
    c.set_forcing(1.0 + np.sin(3.0 * qn[:, 0]) * qn[:, 1])
    c.set_dirichlet(np.zeros(coords.shape[0]) if zero else 0.3 * np.cos(2.0 * coords[:, 0]) + coords[:, -1])
    c.init()
    for k, v in knobs.items():
        c.tune(k, v)
    return c


def pmg_cases(capi, meshgen, workloads, out):
    arms = (("default", {}), ("restart5", {"pmg_restart": 5}), ("smooth0", {"pmg_smooth": 0}), ("blocked0", {"pmg_blocked": 0}), ("blocked1", {"pmg_blocked": 1}),
            ("smooth0_blocked0", {"pmg_smooth": 0, "pmg_blocked": 0}))
    for arm, knobs in arms:   # (a context per arm: no knob of one arm reaches the next)
        c = pmg_context(capi, meshgen, 3, 9, workloads.c5_operator(capi), **knobs)
        info = c.solve(method=capi.SOLVER_PMG, rtol=1e-11, raise_on_noconv=False)
        record_pmg(out, f"pmg.{arm}", info, c.solution())
        c.close()
    # where the coarse level does not help (tests/test_gpu_pmg.py: the indefinite operator by name, a coarse budget of 12): pmg_indefinite ends at maxit, pmg_budget12
    # converges; pmg_stop and pmg_stop2d end with "the coarse level's solves do not converge" after 11 and 24 iterations -- the preconditioner raised `stop`
    adr, indef = -capi.laplacian() + capi.advection([2.0, 1.0]) + capi.reaction(1.0), -capi.laplacian() + capi.reaction(-300.0)
    for name, args, kw, maxit in (("pmg_indefinite", (3, 8, indef), {}, 400), ("pmg_budget12", (2, 60, adr), {"zero": True, "pmg_inner_maxit": 12}, 300),
                                  ("pmg_stop", (3, 8, indef), {"pmg_inner_maxit": 3}, 100), ("pmg_stop2d", (2, 60, indef), {}, 100)):
        c = pmg_context(capi, meshgen, *args, **kw)
        info = c.solve(method=capi.SOLVER_PMG, rtol=1e-10 if "zero" in kw else 1e-11, maxit=maxit, raise_on_noconv=False)
        record_pmg(out, name, info, c.solution())
        print(f"{'':<22} status text: {c.lib.fdapde_last_error(c._ctx).decode()}", flush=True)
        c.close()


def pmg_parabolic_case(capi, meshgen, out):
    nodes, cells, bnd = meshgen.unit_square(20)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(2)
    coords = c.dofs_get()[2]
    qn = c.quadrature_nodes()
    c.set_operator(capi.dt() - capi.laplacian() + capi.advection([1.0, -0.5]))
    c.tune("dense_rows", 0)
    times = np.linspace(0.0, 0.2, 7)
    c.set_forcing(np.stack([np.sin(2.0 * qn[:, 0]) * (1.0 + t) for t in times], axis=1))
    c.init()
    u0 = np.cos(coords[:, 0]) * coords[:, 1]
    G = np.stack([0.1 * np.sin(coords[:, 0] + 3.0 * t) for t in times], axis=1)
    U, info = c.solve_parabolic(times, u0, G, method=capi.SOLVER_PMG, rtol=1e-11)
    record_pmg(out, "pmg_parabolic", info, U)
    c.close()


def run(path):
    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen, workloads

    if capi.load().fdapde_device_count() < 1:
        raise SystemExit("amg_onecol_ab.py needs a HIP device")
    print(f"library: {capi.LIB_PATH}", flush=True)
    out = {}
    solve_case(capi, meshgen, out, "scalar2d", 2, 32, -capi.laplacian())
    solve_case(capi, meshgen, out, "scalar3d", 3, 16, -capi.laplacian() + capi.reaction(2.0), amg_absorb=1)
    handle_case(capi, meshgen, out, "handle", 48, -capi.laplacian() + capi.reaction(2.0), True)
    handle_case(capi, meshgen, out, "handle_adr", 48, -capi.laplacian() + capi.advection([3.0, -1.5]) + capi.reaction(1.0), False)
    handle_case(capi, meshgen, out, "handle_dense", 12, -capi.laplacian() + capi.reaction(2.0), True)
    block_case(capi, meshgen, out)
    parabolic_case(capi, meshgen, out)
    pmg_cases(capi, meshgen, workloads, out)
    pmg_parabolic_case(capi, meshgen, out)
    np.savez(path, **out)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    differ = 0
    for k in sorted(set(a.files) | set(b.files)):
        same = k in a.files and k in b.files and np.array_equal(a[k], b[k])
        differ += 0 if same else 1
        shape = "x".join(str(s) for s in a[k].shape) if k in a.files else "-"
        print(f"{k:<28} {shape:>10} {'array_equal' if same else 'DIFFERS'}")
    print(f"{differ} arrays differ")
    return differ


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    else:
        raise SystemExit(__doc__)
