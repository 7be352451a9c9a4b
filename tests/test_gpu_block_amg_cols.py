"""The columns of fdapde_block_solve under FDAPDE_SOLVER_BLOCK_AMG side by side (knob `amg_cols`; the k_bamg_* kernels at Q = 2, 4, 8 columns and k_block_spmv_cols of
csrc/kernels_block.h, block_amg_batch of csrc/eng_block_amg.hip, fgmres_outer of csrc/eng_pmg.hip at that width), against the column-by-column path (`amg_cols` = 1) on
the same hierarchy: np.array_equal per column at the k-th iterate (`rtol = 1e-30, maxit = k`, k = 1, 2, 5) and at convergence.

Cases a, d, e, g, h of block_iter_ref.AMG_CASES, blocks built as tests/test_gpu_block_iterates.py builds them: both lane widths, absorption (e), a correction that
is the dense level alone (g), `gmres_m` = 3 so that the batch restarts inside the run (h).  Columns: A times a low-frequency vector, a unit vector at an interior
DOF, zeros, one scaled by 1e-150, the smoothing system's own right-hand side, the rest standard normal; n_rhs = 11 goes as 8 + 2 + 1, n_rhs = 7 under
`amg_cols` = 4 as 4 + 2 + 1.  One more case, a-dense: case a under `amg_coarse_rows` = 1024, so that the hierarchy is the dense level alone and the
preconditioner the inverse -- a column's Krylov space is exhausted at once, the recurrence and the true residual (rtol 1e-30) disagree, and the batch hands the
column back to block_amg_run's warm start; the trace must say so.

At convergence every column is also held to scipy's SuperLU on sp.bmat of the blocks (the reference of tests/test_gpu_block_amg.py), relative to the column's
own direct solution, at that file's ladder bar 1e-6."""
import numpy as np
import pytest

import block_iter_ref as ir
import block_ref as br

pytestmark = pytest.mark.gpu
# name -> (system of block_iter_ref.AMG_CASES, knobs on top of the system's own)
CASES = {"a": ("a", {}), "d": ("d", {}), "e": ("e", {}), "g": ("g", {}), "h": ("h", {}), "a-dense": ("a", dict(amg_coarse_rows=1024))}
LU_BAR = 1e-6   # test_gpu_block_amg.py::test_ladder's bound on |x - x_lu| / |x_lu|
SHAPES = [(11, 8), (7, 4)]   # (n_rhs, amg_cols)
RTOL = 1e-10


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi, meshgen


_live = {}


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _live.values():
        s["c"].close()
    _live.clear()


def _system(env, name):
    capi, meshgen = env
    if name not in _live:
        mesh, order, lam, advection, knobs = ir.AMG_CASES[CASES[name][0]][:5]
        knobs = {**knobs, **CASES[name][1]}
        nodes, cells, bnd = getattr(meshgen, mesh[0])(mesh[1])
        c = capi.Context(0)
        c.mesh_upload(nodes, cells, bnd)
        nd = c.dofs_build(order)
        c.tune("amg_coarse_rows", ir.AMG_COARSE_ROWS)
        c.tune("amg_setup_check", 1)
        for k_, v_ in knobs.items():
            c.tune(k_, v_)
        c.set_operator(-capi.laplacian())
        c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
        c.init()
        _, _, coords = c.dofs_get()
        rp, ci = c.pattern_get()
        rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
        obs = br.observed_nodes(nodes.shape[0])
        blocks = br.smoothing_blocks(rp, ci, c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS), obs, lam, nd)
        c.block_compute(*blocks, symmetric=not advection)
        A = br.bmat(rp, ci, blocks, nd)
        B = np.random.default_rng(7).standard_normal((2 * nd, 11))
        low = np.prod(np.cos(np.pi * coords), axis=1)
        B[:, 0] = A @ np.concatenate([low, 0.5 * low])
        B[:, 1] = ir.unit_rhs(nd, ir.interior_dof(rp, nd))
        B[:, 2] = 0.0
        B[:, 3] *= 1e-150
        B[:, 4] = br.smoothing_rhs(obs, lam, nd)
        import scipy.sparse.linalg as spl

        _live[name] = dict(c=c, A=A, n=nd, B=B, knobs=knobs, lu=spl.splu(A.tocsc()))
    return _live[name]


def _solve(capi, c, B, cols, **kw):
    c.tune("amg_cols", cols)
    return c.block_solve(B, method=capi.SOLVER_BLOCK_AMG, raise_on_noconv=False, **kw)


def test_trace_counts_batches_and_single_columns(env):
    """n_rhs = 11 under the default `amg_cols`: 2 batches, 10 batched columns, 1 single column; `amg_cols` = 1: 0 / 0 / 11; fdapde_block_compute drops the
    hierarchy: FDAPDE_ENOTINIT until the next solve builds it, whose trace starts at zero"""
    capi, _ = env
    s = _system(env, "a")
    c = s["c"]
    _, info = c.block_solve(s["B"], method=capi.SOLVER_BLOCK_AMG)   # (the default: no tune call)
    assert info.converged == 1 and info.method_used == capi.SOLVER_BLOCK_AMG
    assert c.amg_cols_trace(capi.AMG_OF_BLOCK) == dict(batches=2, batched_cols=10, single_cols=1)
    mesh, order, lam, advection = ir.AMG_CASES["a"][:4]
    rp, ci = c.pattern_get()
    nodes_n = s["n"]   # (order 1: the DOFs are the nodes)
    blocks = br.smoothing_blocks(np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS),
                                 br.observed_nodes(nodes_n), lam, s["n"])
    c.block_compute(*blocks, symmetric=True)
    with pytest.raises(capi.FdapdeError) as e:
        c.amg_cols_trace(capi.AMG_OF_BLOCK)
    assert e.value.status == capi.ENOTINIT
    _solve(capi, c, s["B"], 1)
    assert c.amg_cols_trace(capi.AMG_OF_BLOCK) == dict(batches=0, batched_cols=0, single_cols=11)
    c.tune("amg_cols", 8)


def _first_difference(X, R):
    return [(j, int(np.flatnonzero(X[:, j] != R[:, j])[0]), float(np.abs(X[:, j] - R[:, j]).max())) for j in range(X.shape[1]) if not np.array_equal(X[:, j], R[:, j])]


def _converged_bar(capi, s, B, X, info):
    """converged, relres <= rtol, per column the residual recomputed by numpy <= 10 rtol of the column's norm and the error against SuperLU <= LU_BAR of the
    column's own direct solution (the zero column: exactly zero, asserted by the caller)"""
    assert info.converged == 1 and info.relres <= RTOL and info.method_used == capi.SOLVER_BLOCK_AMG
    worst = 0.0
    for j in range(B.shape[1]):
        bn = np.linalg.norm(B[:, j])
        assert np.linalg.norm(B[:, j] - s["A"] @ X[:, j]) <= 10 * RTOL * bn, j
        if bn == 0.0:
            continue
        xr = s["lu"].solve(B[:, j])
        err = np.linalg.norm(X[:, j] - xr) / np.linalg.norm(xr)
        worst = max(worst, err)
        print(f"  column {j}: |x - x_lu| / |x_lu| = {err:.2e}")
        assert err <= LU_BAR, (j, err)
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}cols_by{q}" for n, q in SHAPES])
@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_as_column_by_column(env, name, shape):
    """every column np.array_equal between `amg_cols` = 8 / 4 and 1 on the same hierarchy at the k-th iterate and at convergence, the summed iterations and relres
    equal, the zero column exactly zero.  At convergence the bar of tests/test_gpu_block_amg.py that needs no restatement: converged, relres <= rtol, and per
    column the unscaled residual recomputed by numpy against sp.bmat of the blocks <= 10 rtol of the column's own norm"""
    capi, _ = env
    s = _system(env, name)
    c, (n_rhs, cols) = s["c"], shape
    B = s["B"][:, :n_rhs]
    _solve(capi, c, B[:, :1], 1, rtol=1e-30, maxit=1)   # (the hierarchy exists from here on)
    h = c.amg_hierarchy(capi.AMG_OF_BLOCK)
    if name == "e":
        assert h["absorbed"] == 1 and max(int(np.bincount(c.amg_aggregates(capi.AMG_OF_BLOCK, l)).max()) for l in range(len(h["rows"]) - 1)) > 4
    if name == "g":
        assert len(h["rows"]) == 2, "the correction is the dense level alone"
    if name == "h":
        assert s["knobs"]["gmres_m"] == 3, "k = 5 restarts inside the run"
    if name == "a-dense":
        assert len(h["rows"]) == 1, "the hierarchy is the dense level alone"
    t0 = c.amg_cols_trace(capi.AMG_OF_BLOCK)
    for k in (1, 2, 5, None):
        kw = dict(rtol=1e-30, maxit=k) if k else dict(rtol=RTOL)
        X, info = _solve(capi, c, B, cols, **kw)
        R, ref = _solve(capi, c, B, 1, **kw)
        assert c.amg_hierarchy(capi.AMG_OF_BLOCK) == h, "the knob does not rebuild the hierarchy"
        print(f"block {name} n_rhs {n_rhs} amg_cols {cols} k {k}: iterations {info.iters} / {ref.iters}, relres {info.relres:.3e} / {ref.relres:.3e}")
        assert _first_difference(X, R) == [], (name, k, "(column, first row, max |difference|)", _first_difference(X, R))
        assert info.iters == ref.iters and info.relres == ref.relres and info.converged == ref.converged
        assert not X[:, 2].any(), "the zero column is exactly zero"
        if k and name == "a-dense":   # (the preconditioner is the inverse: a column may be done before k)
            assert info.iters <= k * (n_rhs - 1)
        elif k:
            assert info.iters == k * (n_rhs - 1) and info.converged == 0   # (the zero column takes no iteration)
        elif name != "h":
            _converged_bar(capi, s, B, X, info)
    # columns a batch handed back to block_amg_run's warm start: what single_cols counts beyond the tail columns and the column-by-column runs
    t1 = c.amg_cols_trace(capi.AMG_OF_BLOCK)
    handed = t1["single_cols"] - t0["single_cols"] - 4 * (1 + n_rhs)
    print(f"block {name} n_rhs {n_rhs} amg_cols {cols}: {handed} column(s) handed back to the single-column path")
    assert t1["batches"] - t0["batches"] == 8 and t1["batched_cols"] - t0["batched_cols"] == 4 * (n_rhs - 1) and handed >= 0
    if name == "a-dense":
        assert handed >= 1, "the warm start of block_amg_run ran, and its columns carry the column-by-column run's bits (above)"
    if name == "h":
        # restarted after three vectors the outer iteration stalls on the rough columns, in both runs alike (above: the same bits after 200 iterations, converged
        # == 0 in both).  The restart is what h is for; held to the bar of the other cases it runs with the default restart length on the same hierarchy
        assert info.converged == 0 and ref.converged == 0
        c.tune("gmres_m", 50)
        X, info = _solve(capi, c, B, cols, rtol=RTOL)
        R, ref = _solve(capi, c, B, 1, rtol=RTOL)
        c.tune("gmres_m", 3)
        assert c.amg_hierarchy(capi.AMG_OF_BLOCK) == h
        assert _first_difference(X, R) == [] and info.iters == ref.iters and info.relres == ref.relres
        _converged_bar(capi, s, B, X, info)
    c.tune("amg_cols", 8)


def test_in_place_with_8_columns(env):
    capi, _ = env
    s = _system(env, "a")
    c = s["c"]
    R, _ = _solve(capi, c, s["B"][:, :8], 1, rtol=RTOL)
    c.tune("amg_cols", 8)
    bx = np.asfortranarray(s["B"][:, :8].copy())
    info = c.block_solve_inplace(bx, method=capi.SOLVER_BLOCK_AMG, rtol=RTOL)
    assert info.converged == 1 and np.array_equal(bx, R)
