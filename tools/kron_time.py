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

usage: kron_time.py [OUT]      (OUT defaults to profiles/kron_time.txt)

FDAPDE_SOLVER_KRON_AMG against the GMRES stage as it was (the multilevel stage) on the same eight rows:

  kron_time.py --amg PARENT_LIB [OUT] [MESH ...]     (OUT defaults to profiles/kron_amg_time.txt; MESH: 2d, 3d; both by default)

PARENT_LIB is libfdapde_hip.so built from the parent commit.  Every measurement is one fresh process (`--amg-child`) that sets one mesh up, and for every
q computes the handle, solves once to warm up (the first FDAPDE_SOLVER_KRON_AMG solve also builds the hierarchy, whose set-up time and rows per level
it reports) and then times ONE solve by the host clock (the call ends in a stream synchronise).  Five rounds; in every round this tree's library solving
by FDAPDE_SOLVER_KRON_AMG and the parent's solving by FDAPDE_SOLVER_GMRES alternate -> median, smallest and largest of five.

The factored data term of fdapde_kron_set_obs:

  kron_time.py --driver-guard PARENT_LIB [OUT [2d|3d ...]]     (appends to profiles/handle_driver_time.txt): the handle's solve path against the parent commit's -- one
      FDAPDE_SOLVER_GMRES and one FDAPDE_SOLVER_KRON_AMG solve of --amg's systems at q = 2 and 10 on both meshes, five windows per process, the two libraries
      alternating twice; the gate: this library's median is at most the largest of the parent's windows.
  kron_time.py --obs [OUT] [--parent-lib PATH] [a | a2d | a3d] [b] [c]     (OUT defaults to profiles/kron_obs_time.txt; the parts to run, all by default;
  a2d / a3d: part (a) on one of its two meshes)

Every measurement is a process of its own (`--obs-child`), HIP events around 100 operator applications behind 3 warm-ups (fdapde_kron_bench_spmv), the
median of five windows with the smallest and the largest.  The handle is the four pattern terms of the space-time smoothing system (q = 2 m), the term
Phi = [H, 0] with the hat functions of the m time nodes at p = m random instants, about 30 % of the observations missing.
  (a) the Krylov stage's operator with the term live under kron_obs_form 0 (the rule), 1 (narrow) and 2 (wide), and without a term: areal Psi over 32 x 32
      tiles and pointwise Psi of 10^6 random locations on the 2-D mesh (unit_square(708)), areal Psi over 8^3 tiles on the 3-D mesh (unit_cube(118)),
      q = 2, 10, 16: time, bytes by the model of fdapde_kron_bench_spmv, rate;
  (b) the price of factoring: the pointwise design with all observations present (Phi = NULL, p = m) against the five-term handle with I_m (x) G,
      G = fdapde_gram_pointwise's values on the pattern: per operator application and per GMRES(50) solve (2-D mesh, q = 10);
  (c) the guard: the operator of the five-term handle with NO term live, this library and the parent commit's (PATH: its libfdapde_hip.so) alternating --
      the new median against the spread of the parent's five windows."""
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


MESHES = {"2d": ("2-D P1, unit_square(708)", "unit_square", 708), "3d": ("3-D P1, unit_cube(58)", "unit_cube", 58)}


def amg_child(mesh_key, method_name):
    """one fresh process: a mesh, every q, one warm-up and one timed solve each -> a JSON line per q"""
    import json

    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen
    import block_ref as br
    import kron_ref as kr

    _, gen, nx = MESHES[mesh_key]
    nodes, cells, bnd = getattr(meshgen, gen)(nx)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.zeros(c.quadrature_nodes().shape[0]))
    c.init()
    rp, ci = c.pattern_get()
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    obs = br.observed_nodes(nodes.shape[0])
    gram = br.gram_selection_values(rp, ci, obs, nd)
    r1t = br.transpose_values(rp, ci, r1, nd)
    amg = method_name == "KRON_AMG"
    method = capi.SOLVER_KRON_AMG if amg else capi.SOLVER_GMRES
    for q in QS:
        m = q // 2
        Mt, Pt = kr.time_mass(m), kr.time_penalty(m)
        terms = [(kr._in_block(-np.eye(m), m, 0, 0), gram), (kr._in_block(-LAMBDA * Pt, m, 0, 0), r0), (kr._in_block(LAMBDA * Mt, m, 0, 1), r1t),
                 (kr._in_block(LAMBDA * Mt, m, 1, 0), r1), (kr._in_block(LAMBDA * Mt, m, 1, 1), r0)]   # (kron_ref.spacetime_terms, the gram matrix built once)
        b = kr.spacetime_rhs(obs, LAMBDA, nd, m)
        c.tune("kron_dinv_mb", 16384)   # (q = 32 in 2-D: 4.1 GB at level 0, and the multilevel stage counts every level's)
        c.kron_compute(terms, symmetric=True)
        maxit = 200 if amg else 1000
        row = dict(mesh=mesh_key, q=q, rows=q * nd, method=method_name)
        try:
            c.kron_solve(b, method=method, rtol=1e-10, maxit=maxit, raise_on_noconv=False)   # warm-up (and the set-up)
            t0 = time.perf_counter()
            x, info = c.kron_solve(b, method=method, rtol=1e-10, maxit=maxit, raise_on_noconv=False)
            row.update(wall_ms=1e3 * (time.perf_counter() - t0), iters=info.iters, converged=info.converged, relres=info.relres)
            if amg:
                h = c.kron_amg_hierarchy()
                row.update(setup_ms=h["setup_ms"], levels=h["rows"], absorbed=h["absorbed"])
        except capi.FdapdeError as e:   # (a refusal is recorded as such)
            row.update(refused=str(e)[:200])
        print("ROW " + json.dumps(row), flush=True)
    c.close()


def driver_guard_child(mesh_key):
    """one fresh process: a mesh, q = 2 and 10, five FDAPDE_SOLVER_GMRES and five FDAPDE_SOLVER_KRON_AMG solves each behind two warm-ups -> one GUARD_RESULT line"""
    import json

    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen
    import block_ref as br
    import kron_ref as kr

    _, gen, nx = MESHES[mesh_key]
    nodes, cells, bnd = getattr(meshgen, gen)(nx)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.zeros(c.quadrature_nodes().shape[0]))
    c.init()
    rp, ci = c.pattern_get()
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    obs = br.observed_nodes(nodes.shape[0])
    gram = br.gram_selection_values(rp, ci, obs, nd)
    r1t = br.transpose_values(rp, ci, r1, nd)
    res = {"lib": capi.LIB_PATH}
    for q in (2, 10):
        m = q // 2
        Mt, Pt = kr.time_mass(m), kr.time_penalty(m)
        terms = [(kr._in_block(-np.eye(m), m, 0, 0), gram), (kr._in_block(-LAMBDA * Pt, m, 0, 0), r0), (kr._in_block(LAMBDA * Mt, m, 0, 1), r1t),
                 (kr._in_block(LAMBDA * Mt, m, 1, 0), r1), (kr._in_block(LAMBDA * Mt, m, 1, 1), r0)]   # (as amg_child)
        b = kr.spacetime_rhs(obs, LAMBDA, nd, m)
        c.kron_compute(terms, symmetric=True)
        for name, method, maxit in (("GMRES", capi.SOLVER_GMRES, 1000), ("KRON_AMG", capi.SOLVER_KRON_AMG, 200)):
            solve = lambda: c.kron_solve(b, method=method, rtol=1e-10, maxit=maxit, raise_on_noconv=False)
            solve(), solve()
            times = []
            for _ in range(5):
                t0 = time.perf_counter()
                _, info = solve()
                times.append(1e3 * (time.perf_counter() - t0))
            res[f"q {q:2d} {name}"] = {"ms": times, "iters": int(info.iters)}
    c.close()
    print("GUARD_RESULT " + json.dumps(res))


def amg_main(parent_lib, out_path, meshes):
    import json
    import subprocess

    def child(mesh_key, method_name, lib):
        env = dict(os.environ)
        if lib:
            env["FDAPDE_HIP_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--amg-child", mesh_key, method_name], capture_output=True, text=True, env=env, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"a measuring process failed ({mesh_key}, {method_name}): rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return [json.loads(line[4:]) for line in r.stdout.splitlines() if line.startswith("ROW ")]

    out = [f"tools/kron_time.py --amg on {socket.gethostname()} (MI355X), {time.strftime('%Y-%m-%d %H:%M:%S')}",
           "space-time smoothing system, lambda = lambda_T = 1e-4, rtol 1e-10; five rounds, every figure from a fresh process (one warm-up solve, one timed solve);",
           "KRON_AMG: this tree's library, FDAPDE_SOLVER_KRON_AMG (maxit 200); GMRES: the PARENT commit's library, FDAPDE_SOLVER_GMRES (maxit 1000), alternating", ""]
    table = []
    for mk in meshes:
        got = {"KRON_AMG": {}, "GMRES": {}}
        for rnd in range(5):
            for name, lib in (("KRON_AMG", None), ("GMRES", parent_lib)):
                for row in child(mk, name, lib):
                    got[name].setdefault(row["q"], []).append(row)
            print(f"{mk}: round {rnd + 1} of 5 done", flush=True)
        out.append(f"{MESHES[mk][0]}")
        for q in QS:
            a, g = got["KRON_AMG"][q], got["GMRES"][q]
            out.append(f"  q = {q:2d}, q n = {a[0]['rows']}")
            if "refused" in a[0]:
                out.append(f"    KRON_AMG refused: {a[0]['refused']}")
                continue
            ta, tg = [r["wall_ms"] for r in a], [r["wall_ms"] for r in g]
            ts = [r["setup_ms"] for r in a]
            out.append(f"    KRON_AMG  {a[0]['iters']} iterations, converged {a[0]['converged']}, relres {a[0]['relres']:.2e} (unscaled), solve {spread(ta)}; "
                       f"set-up {spread(ts)}, absorbed {a[0]['absorbed']}, {len(a[0]['levels'])} levels, rows {' / '.join(str(r) for r in a[0]['levels'])}")
            out.append(f"    GMRES     {g[0]['iters']} iterations, converged {g[0]['converged']}, relres {g[0]['relres']:.2e} (D^-1-scaled), solve {spread(tg)}")
            ratio = float(np.median(ta) / np.median(tg))
            out.append(f"    KRON_AMG / GMRES  {ratio:.2f} x the time, {a[0]['iters'] / max(g[0]['iters'], 1):.2f} x the iterations -> {'wins' if ratio < 1 else 'loses'}")
            table.append((MESHES[mk][0].split(",")[0], q, a[0]["rows"], " / ".join(str(r) for r in a[0]["levels"]), float(np.median(ts)), a[0]["iters"], float(np.median(ta)),
                          min(ta), max(ta), g[0]["iters"], float(np.median(tg)), min(tg), max(tg), ratio))
        out.append("")
    out += ["| mesh | q | q n | rows per level | set-up, ms | KRON_AMG iterations | KRON_AMG solve, ms (smallest, largest) | GMRES iterations | GMRES solve, ms (smallest, largest) | time ratio |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for r in table:
        out.append("| {} | {} | {} | {} | {:.1f} | {} | {:.1f} ({:.1f}, {:.1f}) | {} | {:.1f} ({:.1f}, {:.1f}) | {:.2f} |".format(*r))
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


# ---- --obs: the factored data term (fdapde_kron_set_obs) ---------------------------------------------------------------------------------------------
OBS_MESHES = {"sq": ("2-D P1, unit_square(708)", "unit_square", 708), "cube": ("3-D P1, unit_cube(118)", "unit_cube", 118)}
OBS_QS = (2, 10, 16)


def obs_child(argv):
    """--obs-child KIND MESH Q FORM: KIND areal | pointwise (the operator with a term), none (the four-term handle alone), op_term | op_five (all observations
    present: factored / on the pattern), solve_term | solve_five (one GMRES solve of those), guard (the five-term handle of kron_ref.spacetime_terms)"""
    import json

    from fdapde_loader import load_package

    capi = load_package().capi
    from fdapde_core_amd import meshgen
    import block_ref as br
    import block_time as bt
    import kron_obs_ref as ko
    import kron_ref as kr

    kind, which, q, form = argv[0], argv[1], int(argv[2]), int(argv[3])
    m = q // 2
    _, gen, nx = OBS_MESHES[which]
    mesh = getattr(meshgen, gen)(nx)
    c, n_nodes = bt.space(capi, mesh)
    rp, ci = c.pattern_get()
    nd = len(rp) - 1
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    r1t = br.transpose_values(rp, ci, r1, nd)
    Mt, Pt = kr.time_mass(m), kr.time_penalty(m)
    four = [(kr._in_block(-LAMBDA * Pt, m, 0, 0), r0), (kr._in_block(LAMBDA * Mt, m, 0, 1), r1t), (kr._in_block(LAMBDA * Mt, m, 1, 0), r1),
            (kr._in_block(LAMBDA * Mt, m, 1, 1), r0)]
    res = {"kind": kind, "mesh": which, "q": q, "n_dofs": nd, "pattern_nnz": len(ci)}
    need_mb = 8.0 * q * q * nd / 1048576.0
    if need_mb > 2048:
        c.tune("kron_dinv_mb", 8192)
        res["dinv_mb"] = need_mb
    rng = np.random.default_rng(5)
    psi = None
    if kind == "areal":
        psi = bt._tiles_psi(c, mesh, 32 if which == "sq" else 8)
    elif kind in ("pointwise", "op_term", "op_five", "solve_term", "solve_five"):
        psi, cells, vals = bt._pointwise_psi(c, mesh, 1000000)
    if psi is not None:
        res.update(n_obs=psi.shape[0], nnz=int(psi.nnz), longest_row=int(np.diff(psi.indptr).max()), longest_col=int(np.bincount(psi.indices, minlength=nd).max()))
    t0 = time.perf_counter()
    if kind == "guard":
        obs = br.observed_nodes(n_nodes)
        c.kron_compute([(kr._in_block(-np.eye(m), m, 0, 0), br.gram_selection_values(rp, ci, obs, nd))] + four, symmetric=True)
    elif kind in ("op_five", "solve_five"):
        c.kron_compute([(kr._in_block(-np.eye(m), m, 0, 0), c.gram_pointwise(cells, vals))] + four, symmetric=True)
    else:
        c.kron_compute(four, symmetric=True)
        if kind in ("areal", "pointwise"):
            times = np.sort(rng.uniform(0, 1, m))
            W = (rng.uniform(size=(m, psi.shape[0])) >= 0.3).astype(float)
            c.tune("kron_obs_form", form)
            c.kron_set_obs(psi, Phi=np.hstack([ko.hats(m, times), np.zeros((m, m))]), weights=W, scale=-1.0)
        elif kind in ("op_term", "solve_term"):
            c.kron_set_obs(psi, Phi=None, weights=np.ones((m, psi.shape[0])), scale=-1.0)
        if kind != "none":
            info = c.kron_obs_info()
            res.update(p=info["p"], form_rows=info["form_rows"], form_cols=info["form_cols"])
    res["setup_ms"] = 1e3 * (time.perf_counter() - t0)
    if kind in ("solve_term", "solve_five"):
        z = rng.standard_normal(m * psi.shape[0])
        b = np.concatenate([-np.concatenate([psi.T @ z[r * psi.shape[0]:(r + 1) * psi.shape[0]] for r in range(m)]), LAMBDA * 0.1 * rng.standard_normal(m * nd)])
        c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=1000, raise_on_noconv=False)   # (warm-up: the work buffers)
        t0 = time.perf_counter()
        x, info = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=1000, raise_on_noconv=False)
        res.update(solve_ms=1e3 * (time.perf_counter() - t0), iters=info.iters, converged=info.converged, relres=info.relres)
    else:
        win, by = [], 0.0
        for _ in range(5):
            ms, by = c.kron_bench_spmv(REPS)
            win.append(ms)
        res.update(windows_ms=win, bytes=by)
    c.close()
    print("OBS_RESULT " + json.dumps(res))


def obs_main(out_path, parent_lib, parts):
    import json
    import subprocess

    def child(kind, which, q, form=0, lib=None):
        env = dict(os.environ)
        if lib:
            env["FDAPDE_HIP_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--obs-child", kind, which, str(q), str(form)], capture_output=True, text=True, env=env, timeout=600)
        for line in r.stdout.splitlines():
            if line.startswith("OBS_RESULT "):
                print(line, file=sys.stderr, flush=True)   # (progress)
                return json.loads(line[len("OBS_RESULT "):])
        raise SystemExit(f"child {kind} {which} {q} {form} failed (rc {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")

    def op_line(r):
        med = float(np.median(r["windows_ms"]))
        return f"{spread(r['windows_ms'])}; {r['bytes'] / 1e6:.1f} MB by the model -> {r['bytes'] / (med * 1e-3) / 1e12:.2f} TB/s"

    out = [f"tools/kron_time.py --obs on {socket.gethostname()} (MI355X), {time.strftime('%Y-%m-%d %H:%M:%S')}",
           f"HIP events around {REPS} operator applications behind 3 warm-ups, five windows (median, smallest, largest), every line a process of its own", ""]

    def flush():
        text = "\n".join(out) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)
        return text

    if "a" in parts or "a2d" in parts or "a3d" in parts:
        out.append("(a) the Krylov stage's operator with a data term live: k_kron_spmv (D^-1 fused in) + k_kron_obs_gather + k_kron_obs_scatter; p = m = q / 2")
        for which, kinds in (("sq", ("areal", "pointwise")), ("cube", ("areal",))):
            if "a" not in parts and ("a2d" if which == "sq" else "a3d") not in parts:
                continue
            for q in OBS_QS:
                base = child("none", which, q)
                out.append(f"{OBS_MESHES[which][0]}: {base['n_dofs']} DOFs, {base['pattern_nnz']} pattern entries, q = {q}; without a term {op_line(base)}")
                for kind in kinds:
                    got = {}
                    for form in (0, 1, 2):
                        r = got[form] = child(kind, which, q, form)
                        out.append(f"  {kind:9s} Psi {r['n_obs']} x {r['n_dofs']}, {r['nnz']} entries, longest row {r['longest_row']} / column {r['longest_col']}; kron_obs_form {form} -> "
                                   f"{r['form_rows']} / {r['form_cols']}: {op_line(r)}")
                        flush()
                    med = {f: float(np.median(got[f]["windows_ms"])) for f in got}
                    best = min(med, key=med.get)
                    same = (got[best]["form_rows"], got[best]["form_cols"]) == (got[0]["form_rows"], got[0]["form_cols"])
                    out.append(f"  -> fastest: kron_obs_form {best} ({med[best]:.4f} ms); the rule's choice {got[0]['form_rows']} / {got[0]['form_cols']} ({med[0]:.4f} ms) "
                               f"{'is that setting' if best == 0 or same else 'is NOT the fastest'}")
        out.append("")
    if "b" in parts:
        out.append("(b) the price of factoring (2-D mesh, 10^6 random locations, every observation present, q = 10): the term factored (Phi = NULL, p = m) against the "
                   "five-term handle with I_m (x) G, G = fdapde_gram_pointwise's values")
        for kind, label in (("op_term", "operator, factored"), ("op_five", "operator, on the pattern")):
            r = child(kind, "sq", 10)
            out.append(f"  {label:28s} {op_line(r)}; set-up {r['setup_ms']:.1f} ms")
            flush()
        for kind, label in (("solve_term", "GMRES(50) solve, factored"), ("solve_five", "GMRES(50) solve, on the pattern")):
            r = child(kind, "sq", 10)
            out.append(f"  {label:32s} iterations {r['iters']}, converged {r['converged']}, relres {r['relres']:.2e}, {r['solve_ms']:.1f} ms "
                       f"({r['solve_ms'] / max(r['iters'], 1):.3f} ms per iteration); set-up {r['setup_ms']:.1f} ms")
            flush()
        out.append("")
    if "c" in parts:
        out.append("(c) the guard: fdapde_kron_bench_spmv of the five-term handle with NO term live, this library and the parent commit's alternating")
        if parent_lib:
            for which, q in (("sq", 2), ("sq", 10), ("sq", 16), ("cube", 10)):
                new, old = child("guard", which, q), child("guard", which, q, lib=parent_lib)
                med = float(np.median(new["windows_ms"]))
                inside = min(old["windows_ms"]) <= med <= max(old["windows_ms"])
                out.append(f"  {which:4s} q = {q:2d}: this library {spread(new['windows_ms'])} | the parent's {spread(old['windows_ms'])} -> the new median "
                           f"{'lies within' if inside else 'is OUTSIDE'} the parent's spread")
                flush()
        else:
            out.append("  (no --parent-lib given: not measured)")
    print(flush())


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--obs-child":
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        return obs_child(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--obs":
        rest = sys.argv[2:]
        parent = None
        if "--parent-lib" in rest:
            i = rest.index("--parent-lib")
            parent = os.path.abspath(rest[i + 1])
            del rest[i:i + 2]
        known = ("a", "a2d", "a3d", "b", "c")
        parts = [a for a in rest if a in known] or ["a", "b", "c"]
        paths = [a for a in rest if a not in known]
        return obs_main(paths[0] if paths else os.path.join(ROOT, "profiles", "kron_obs_time.txt"), parent, parts)
    if len(sys.argv) == 3 and sys.argv[1] == "--driver-guard-child":
        return driver_guard_child(sys.argv[2])
    if len(sys.argv) >= 3 and sys.argv[1] == "--driver-guard":   # (the alternation and the gate are block_amg_time.py's)
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import block_amg_time

        return block_amg_time.driver_guard_main(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "handle_driver_time.txt"),
                                                tool=__file__, cases=tuple(sys.argv[4:]) or ("2d", "3d"), what="fdapde_kron_solve, the space-time system of --amg (lambda = lambda_T = 1e-4), q = 2 and 10")
    if len(sys.argv) > 1 and sys.argv[1] == "--amg-child":
        return amg_child(sys.argv[2], sys.argv[3])
    if len(sys.argv) > 1 and sys.argv[1] == "--amg":
        if len(sys.argv) < 3:
            raise SystemExit("usage: kron_time.py --amg PARENT_LIB [OUT] [MESH ...]")
        rest = sys.argv[3:]
        out_path = rest[0] if rest and rest[0] not in MESHES else os.path.join(ROOT, "profiles", "kron_amg_time.txt")
        meshes = [a for a in rest if a in MESHES] or list(MESHES)
        return amg_main(os.path.abspath(sys.argv[2]), out_path, meshes)
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
