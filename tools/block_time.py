#!/usr/bin/env python3
"""The 2 x 2 block handle on sizes a user would run: nothing here is compared against a gate -- no earlier number exists for this operator.

  * k_block_spmv (the Krylov stage's operator on D^-1 A): HIP events around REPS launches behind three warm-up launches (fdapde_block_bench_spmv), repeated
    five times -> median, smallest, largest; bytes per launch from the model 36 nnz + 4 (n + 1) + 32 n, and that over the 8 TB/s HBM peak.  Beside it: FOUR
    launches of the scalar SpMV kernel on the same pattern (fdapde_bench_spmv x 4, fused dot partials included: the launch inside CG) -- the only way the
    parent of this change could apply four blocks.  Sizes: C2's (unit_square(708): 502 681 DOFs) and a 3-D P1 space of 1 685 159 DOFs (unit_cube(118)).
  * one smoothing solve (observations at half of the nodes, lambda 1e-4, rtol 1e-10, at most 2 000 iterations of GMRES(50)) at those sizes: iterations and
    the host clock around the call (it ends in a stream synchronise).
  * the dense stage at 2 n = 578 and 2 178 (unit_square_16 / _32): the inversion, then the host clock around calls of one column and of 64.

usage: block_time.py [OUT]      (OUT defaults to profiles/block_time.txt)"""
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
LAMBDA = 1e-4


def smoothing_blocks(c, capi, n_nodes):
    """the four blocks on the pattern for R1 = stiff() of -laplacian (symmetric: R1^T = R1), R0 = mass(), Psi = the identity's rows at half of the nodes"""
    rp, ci = c.pattern_get()
    nd = len(rp) - 1
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    obs = np.sort(np.random.default_rng(0).choice(n_nodes, n_nodes // 2, replace=False))
    rows = np.repeat(np.arange(nd, dtype=np.int64), np.diff(rp))
    diag_slot = np.flatnonzero(ci == rows)
    assert len(diag_slot) == nd
    a11 = np.zeros(len(ci))
    a11[diag_slot[obs]] = -1.0
    rng = np.random.default_rng(1)
    b = np.zeros(2 * nd)
    b[obs] = -rng.standard_normal(len(obs))
    b[nd:] = LAMBDA * 0.1 * rng.standard_normal(nd)
    return (a11, LAMBDA * r1, LAMBDA * r1, LAMBDA * r0), b, nd, len(ci)


def space(capi, mesh):
    nodes, cells, bnd = mesh
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(1)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.zeros(c.quadrature_nodes().shape[0]))
    c.init()
    return c, nodes.shape[0]


def spread(v):
    return f"{np.median(v):.4f} ms (smallest {min(v):.4f}, largest {max(v):.4f})"


def large(capi, label, mesh, out):
    c, n_nodes = space(capi, mesh)
    blocks, b, nd, nnz = smoothing_blocks(c, capi, n_nodes)
    c.block_compute(*blocks, symmetric=True)
    blk, sca = [], []
    by_blk = by_sca = 0.0
    for _ in range(5):   # the two alternate inside one process
        ms, by_blk = c.block_bench_spmv(200)
        blk.append(ms)
        ms, by_sca = c.bench_spmv(200)
        sca.append(4.0 * ms)
    med = float(np.median(blk))
    out.append(f"{label}: {nd} DOFs, {nnz} pattern entries")
    out.append(f"  k_block_spmv                     {spread(blk)}; {by_blk / 1e6:.1f} MB per launch by the model -> {by_blk / (med * 1e-3) / 1e12:.2f} TB/s, "
               f"{100 * by_blk / (med * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")
    out.append(f"  4 x the scalar SpMV launch       {spread(sca)}; 4 x {by_sca / 1e6:.1f} MB by its model")
    t0 = time.perf_counter()
    x, info = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000, raise_on_noconv=False)
    wall = time.perf_counter() - t0
    out.append(f"  smoothing solve, lambda {LAMBDA:g}:    GMRES(50) iterations {info.iters}, converged {info.converged}, relres {info.relres:.2e}, {1e3 * wall:.1f} ms "
               f"({1e3 * wall / max(info.iters, 1):.3f} ms per iteration)")
    c.close()


def dense(capi, workloads, name, out):
    c, n_nodes = space(capi, workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", name)))
    blocks, b, nd, _ = smoothing_blocks(c, capi, n_nodes)
    c.block_compute(*blocks, symmetric=True)
    t0 = time.perf_counter()
    c.block_solve(b, method=capi.SOLVER_DENSE)
    first = time.perf_counter() - t0
    B = np.random.default_rng(2).standard_normal((2 * nd, 64))
    one, many = [], []
    for _ in range(5):
        c.block_solve(b, method=capi.SOLVER_DENSE), c.block_solve(B, method=capi.SOLVER_DENSE)
    for _ in range(50):
        t0 = time.perf_counter()
        c.block_solve(b, method=capi.SOLVER_DENSE)
        one.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        c.block_solve(B, method=capi.SOLVER_DENSE)
        many.append(1e3 * (time.perf_counter() - t0) / 64)
    x, info = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000, raise_on_noconv=False)
    t0 = time.perf_counter()
    x, info = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000, raise_on_noconv=False)
    gm = 1e3 * (time.perf_counter() - t0)
    out.append(f"{name}: 2 n = {2 * nd}: first dense call (inversion + one column) {1e3 * first:.2f} ms; per column, one per call {spread(one)}; "
               f"per column, 64 per call {spread(many)}; the same column by GMRES(50): {info.iters} iterations, {gm:.2f} ms")
    c.close()


def main():
    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen, workloads

    if capi.load().fdapde_device_count() < 1:
        raise SystemExit("block_time.py needs a HIP device; a CPU run says nothing about these times")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "block_time.txt")
    out = [f"tools/block_time.py on {socket.gethostname()} (MI355X), {time.strftime('%Y-%m-%d %H:%M:%S')}", ""]
    large(capi, "2-D P1, unit_square(708) (C2's size)", meshgen.unit_square(708), out)
    large(capi, "3-D P1, unit_cube(118)", meshgen.unit_cube(118), out)
    out.append("")
    dense(capi, workloads, "unit_square_16", out)
    dense(capi, workloads, "unit_square_32", out)
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
