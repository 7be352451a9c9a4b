#!/usr/bin/env python3
"""The Kronecker-sum handle on sizes a user would run: nothing here is compared against a gate -- no earlier number exists for this operator.

The space-time separable smoothing system of tests/kron_ref.py (observations at half of the nodes, lambda = lambda_T = 1e-4, m = q / 2 time nodes, four
distinct spatial factors) on a 2-D P1 mesh of about 0.5 M DOFs (unit_square(708)) and a 3-D P1 mesh of about 0.2 M DOFs (unit_cube(58)), q in {2, 10, 16, 32}:

  * the Krylov stage's operator D^-1 A (fdapde_kron_bench_spmv: HIP events around REPS applications behind three warm-up ones), five times each with D^-1
    fused into the epilogue of k_kron_spmv and with k_kron_dinv_apply as a launch of its own, alternating inside one process -> median, smallest,
    largest; bytes by the model 8 n_S nnz + 4 nnz + 4 (n + 1) + 16 q n + 8 q^2 n, and that over the 8 TB/s HBM peak;
  * as yardstick the same product A x (without D^-1) through torch.sparse_csr on the explicit matrix, on the same device with the same event timing;
    its bytes are 12 per stored entry + 16 q n;
  * one solve by GMRES(50) (rtol 1e-10, at most 1 000 iterations): iterations and the host clock around the call (it ends in a stream synchronise).

D^-1 takes 8 q^2 n bytes: 4.1 GB at q = 32 on the 2-D mesh, above the default budget (kron_dinv_mb = 2048), which this tool raises to 8192 and says so.

usage: kron_time.py [OUT]      (OUT defaults to profiles/kron_time.txt)"""
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12
LAMBDA = 1e-4
REPS = 100
QS = (2, 10, 16, 32)


def spread(v):
    return f"{np.median(v):.4f} ms (smallest {min(v):.4f}, largest {max(v):.4f})"


def explicit_on_device(torch, terms, rp, ci, n, q, dev="cuda:0"):
    """the explicit matrix as a torch.sparse_csr tensor on the device, built there: row r n + i holds, for every s with some T_k[r, s] != 0 (ascending), the
    entries of row i of the pattern at columns s n + j with value sum_k T_k[r, s] S_k[i, j]"""
    T = torch.tensor(np.stack([t for t, _ in terms]), device=dev)            # (K, q, q)
    S = torch.tensor(np.stack([s for _, s in terms]), device=dev)            # (K, nnz)
    rowptr = torch.tensor(rp.astype(np.int64), device=dev)
    col = torch.tensor(ci.astype(np.int64), device=dev)
    nnz = col.numel()
    length = rowptr[1:] - rowptr[:-1]
    row_of = torch.repeat_interleave(torch.arange(n, device=dev), length)
    within = torch.arange(nnz, device=dev) - rowptr[row_of]
    mask = (T != 0).any(dim=0)                                               # (q, q)
    cnt = mask.sum(dim=1)
    total = int(cnt.sum().item()) * nnz
    cols = torch.empty(total, dtype=torch.int64, device=dev)
    vals = torch.empty(total, dtype=torch.float64, device=dev)
    crow = torch.zeros(q * n + 1, dtype=torch.int64, device=dev)
    base = 0
    for r in range(q):
        ss = torch.nonzero(mask[r]).reshape(-1).tolist()
        c = len(ss)
        crow[r * n + 1:(r + 1) * n + 1] = base + (rowptr[1:] * c)
        for si, s in enumerate(ss):
            pos = base + rowptr[row_of] * c + si * length[row_of] + within
            cols[pos] = col + s * n
            vals[pos] = (T[:, r, s].reshape(-1, 1) * S).sum(dim=0)
        base += c * nnz
    return torch.sparse_csr_tensor(crow, cols, vals, size=(q * n, q * n)), total


def torch_product(torch, A, nq):
    x = torch.ones(nq, dtype=torch.float64, device="cuda:0")
    for _ in range(3):
        y = A @ x
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            y = A @ x
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / REPS)
    del y
    return out


def one_mesh(capi, torch, kr, br, label, mesh, out, table):
    nodes, cells, bnd = mesh
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.zeros(c.quadrature_nodes().shape[0]))
    c.init()
    rp, ci = c.pattern_get()
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    obs = br.observed_nodes(nodes.shape[0])
    out.append(f"{label}: {nd} DOFs, {len(ci)} pattern entries")
    for q in QS:
        m = q // 2
        terms = kr.spacetime_terms(rp, ci, r1, r0, obs, LAMBDA, LAMBDA, m)
        b = kr.spacetime_rhs(obs, LAMBDA, nd, m)
        need_mb = 8.0 * q * q * nd / 1048576.0
        raised = need_mb > 2048
        c.tune("kron_dinv_mb", 8192 if raised else 2048)
        c.kron_compute(terms, symmetric=True)
        fused, apart = [], []
        by = 0.0
        for _ in range(5):   # the two alternate inside one process
            c.tune("kron_fuse", 1)
            ms, by = c.kron_bench_spmv(REPS)
            fused.append(ms)
            c.tune("kron_fuse", 0)
            ms, by = c.kron_bench_spmv(REPS)
            apart.append(ms)
        c.tune("kron_fuse", 1)
        med_f, med_a = float(np.median(fused)), float(np.median(apart))
        best = min(med_f, med_a)
        out.append(f"  q = {q:2d} (m = {m}, n_S = 4, q n = {q * nd}){', kron_dinv_mb raised to 8192 (D^-1 takes %.0f MiB)' % need_mb if raised else ''}")
        out.append(f"    D^-1 A, D^-1 fused in            {spread(fused)}; {by / 1e6:.1f} MB by the model -> {by / (med_f * 1e-3) / 1e12:.2f} TB/s, "
                   f"{100 * by / (med_f * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")
        out.append(f"    D^-1 A, k_kron_dinv_apply apart  {spread(apart)}; -> {by / (med_a * 1e-3) / 1e12:.2f} TB/s, {100 * by / (med_a * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s "
                   f"(model bytes as above; the second launch also writes and reads y once more: + {16 * q * nd / 1e6:.1f} MB)")
        t_med, t_txt, t_by = float("nan"), "not measured", 0.0
        try:
            A, stored = explicit_on_device(torch, terms, rp, ci, nd, q)
            tt = torch_product(torch, A, q * nd)
            t_med, t_by = float(np.median(tt)), 12.0 * stored + 16.0 * q * nd
            t_txt = f"{spread(tt)}; {stored} stored entries, {t_by / 1e6:.1f} MB by its model -> {t_by / (t_med * 1e-3) / 1e12:.2f} TB/s"
            del A
            torch.cuda.empty_cache()
        except Exception as e:   # (a yardstick that cannot run is reported, not replaced)
            t_txt = f"not measured: {type(e).__name__}: {str(e).splitlines()[0][:160]}"
        out.append(f"    A x through torch.sparse_csr      {t_txt}")
        t0 = time.perf_counter()
        x, info = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=1000, raise_on_noconv=False)
        wall = time.perf_counter() - t0
        out.append(f"    solve by GMRES(50)                iterations {info.iters}, converged {info.converged}, relres {info.relres:.2e}, {1e3 * wall:.1f} ms "
                   f"({1e3 * wall / max(info.iters, 1):.3f} ms per iteration)")
        table.append((label.split(",")[0], q, q * nd, by / 1e6, med_f, med_a, 100 * by / (best * 1e-3) / HBM_PEAK, t_med, info.iters, info.converged, 1e3 * wall))
    c.close()


def main():
    import torch   # (before the library: torch brings its own HIP runtime and finds no device once another copy has been initialised)

    if torch.cuda.is_available():
        torch.zeros(1, device="cuda:0")
    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen

    if capi.load().fdapde_device_count() < 1:
        raise SystemExit("kron_time.py needs a HIP device; a CPU run says nothing about these times")
    import block_ref as br
    import kron_ref as kr

    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kron_time.txt")
    out = [f"tools/kron_time.py on {socket.gethostname()} (MI355X), {time.strftime('%Y-%m-%d %H:%M:%S')}", ""]
    table = []
    one_mesh(capi, torch, kr, br, "2-D P1, unit_square(708)", meshgen.unit_square(708), out, table)
    out.append("")
    one_mesh(capi, torch, kr, br, "3-D P1, unit_cube(58)", meshgen.unit_cube(58), out, table)
    out += ["", "| mesh | q | q n | MB by the model | D^-1 A fused, ms | D^-1 A two launches, ms | faster one, % of 8 TB/s | torch.sparse_csr A x, ms | GMRES(50) iterations | converged | solve, ms |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    for row in table:
        out.append("| {} | {} | {} | {:.1f} | {:.4f} | {:.4f} | {:.1f} | {:.4f} | {} | {} | {:.1f} |".format(*row))
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
