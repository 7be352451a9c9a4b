#!/usr/bin/env python3
"""Bit identity of the multilevel solvers between two builds of the library: the single-column path as the one-column instantiation of the column kernels
(csrc/eng_amg.hip, csrc/kernels_block.h) against the parent commit's hand-written single-column kernels.  -> section 1 of profiles/amg_onecol_ab.txt

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
amg_setup_check 1 and amg_coarse_rows 256 throughout, as the tests: every hierarchy but handle_dense's has three levels."""
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


def run(path):
    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen

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
