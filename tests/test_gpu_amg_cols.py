"""The columns of fdapde_lin_solve under FDAPDE_SOLVER_AMG side by side (knob `amg_cols`; csrc/eng_amg.hip: the cycle kernels at Q = 2, 4, 8 columns, amg_cycle; csrc/eng_pmg.hip:
fgmres_outer at that width), against the column-by-column path (`amg_cols` = 1: the same kernels at Q = 1) on the same hierarchy.

With the hierarchy fixed the k-th iterate of a column is ONE vector, and every cycle kernel orders a column's sums in the same way at every width: a batch
must hand out the column-by-column run's BITS -- np.array_equal per column at `rtol = 1e-30, maxit = k` (k = 1, 2, 5) and at convergence.  Right-hand sides of
different difficulty stop at different iterations: a smooth column, a unit vector, a column of zeros, a column scaled by 1e-150, random columns; n_rhs = 11 goes as
8 + 2 + 1, n_rhs = 7 under `amg_cols` = 4 as 4 + 2 + 1.  `amg_coarse_rows` = 256 and `amg_setup_check` = 1 throughout, as tests/test_gpu_amg.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# name -> (dimension, nx, order, operator, symmetric, knobs)
SYSTEMS = {
    "p1_2d_sym": (2, 48, 1, "reaction", True, {}),        # 2 401 DOFs, narrow rows; flexible-CG corrections
    "p1_2d_adr": (2, 48, 1, "adr", False, {}),            # -Lap + b.grad + 1 handed over as non-symmetric: GCR corrections
    "p1_3d": (3, 12, 1, "reaction", True, dict(amg_absorb=1)),   # 2 197 DOFs, rows longer than one team pass, aggregates of more than four rows
    "p2_2d": (2, 20, 2, "reaction", True, {}),            # 1 681 DOFs, long and short rows on one level
    "dense": (2, 12, 1, "reaction", True, {}),            # 169 DOFs: the hierarchy is the dense level alone
}
SHAPES = [(11, 8), (7, 4)]   # (n_rhs, amg_cols)


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


def _rhs(A, coords, bd, n_rhs):
    """the columns of the issue: smooth, unit vector at an interior DOF, zeros, one scaled by 1e-150, the rest standard normal"""
    n = A.shape[0]
    rng = np.random.default_rng(7)
    B = rng.standard_normal((n, n_rhs))
    low = np.prod(np.cos(np.pi * coords), axis=1)
    B[:, 0] = A @ low
    interior = np.flatnonzero(bd == 0)
    B[:, 1] = 0.0
    B[interior[len(interior) // 2], 1] = 1.0
    B[:, 2] = 0.0
    B[:, 3] *= 1e-150
    return B


def _system(env, name):
    import scipy.sparse as sp

    capi, meshgen = env
    if name not in _live:
        dim, nx, order, kind, sym, knobs = SYSTEMS[name]
        nodes, cells, bnd = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
        c = capi.Context(0)
        c.mesh_upload(nodes, cells, bnd)
        nd = c.dofs_build(order)
        c.tune("amg_coarse_rows", 256)
        c.tune("amg_setup_check", 1)
        for k_, v_ in knobs.items():
            c.tune(k_, v_)
        _, bd, coords = c.dofs_get()
        op = -capi.laplacian() + capi.reaction(2.0)
        if kind == "adr":
            op = -capi.laplacian() + capi.advection([3.0, -1.5]) + capi.reaction(1.0)
        c.set_operator(op)
        c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
        c.init()
        rp, ci = c.pattern_get()
        A = sp.csr_matrix((c.matrix_values(capi.MAT_STIFF), ci, rp), shape=(nd, nd))
        c.lin_compute(values=A.data, symmetric=sym)
        _live[name] = dict(c=c, A=A, n=nd, sym=sym, B=_rhs(A, coords, np.asarray(bd), 11))
    return _live[name]


def _solve(capi, c, B, cols, **kw):
    c.tune("amg_cols", cols)
    return c.lin_solve(B, method=capi.SOLVER_AMG, raise_on_noconv=False, **kw)


def test_trace_counts_batches_and_single_columns(env):
    """n_rhs = 11 under the default `amg_cols`: 2 batches, 10 batched columns, 1 single column; under `amg_cols` = 1: 0 / 0 / 11.  fdapde_lin_compute builds the
    hierarchy again and the trace restarts at zero; before the first solve there is no hierarchy to ask (FDAPDE_ENOTINIT), fdapde_solve's own is
    FDAPDE_EUNSUPPORTED"""
    capi, _ = env
    s = _system(env, "p1_2d_sym")
    c = s["c"]
    c.lin_compute(values=s["A"].data, symmetric=True)
    with pytest.raises(capi.FdapdeError) as e:
        c.amg_cols_trace(capi.AMG_OF_HANDLE)
    assert e.value.status == capi.ENOTINIT
    with pytest.raises(capi.FdapdeError) as e:
        c.amg_cols_trace(capi.AMG_OF_SOLVE)
    assert e.value.status == capi.EUNSUPPORTED
    _, info = c.lin_solve(s["B"], method=capi.SOLVER_AMG)   # (the default: no tune call)
    assert info.converged == 1 and info.method_used == capi.SOLVER_AMG
    assert c.amg_cols_trace(capi.AMG_OF_HANDLE) == dict(batches=2, batched_cols=10, single_cols=1)
    c.lin_compute(values=s["A"].data, symmetric=True)
    _solve(capi, c, s["B"], 1)
    assert c.amg_cols_trace(capi.AMG_OF_HANDLE) == dict(batches=0, batched_cols=0, single_cols=11)
    _solve(capi, c, s["B"][:, :7], 4)   # 4 + 2 + 1, counted on top
    assert c.amg_cols_trace(capi.AMG_OF_HANDLE) == dict(batches=2, batched_cols=6, single_cols=12)
    for bad in (0, 3, 16):
        with pytest.raises(capi.FdapdeError):
            c.tune("amg_cols", bad)
    c.tune("amg_cols", 8)


def _first_difference(X, R):
    return [(j, int(np.flatnonzero(X[:, j] != R[:, j])[0]), float(np.abs(X[:, j] - R[:, j]).max())) for j in range(X.shape[1]) if not np.array_equal(X[:, j], R[:, j])]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}cols_by{q}" for n, q in SHAPES])
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_same_bits_as_column_by_column(env, name, shape):
    """every column np.array_equal between `amg_cols` = 8 / 4 and 1 on the same hierarchy at the k-th iterate (k = 1, 2, 5) and at convergence; the summed
    iterations and relres equal; the zero column exactly zero; and at convergence every column within 1e-8 of SuperLU's (the 1e-150 column relative to its own
    norm: every bound here is relative to the column's reference)"""
    import scipy.sparse.linalg as spl

    capi, _ = env
    s = _system(env, name)
    c, (n_rhs, cols) = s["c"], shape
    B = s["B"][:, :n_rhs]
    _solve(capi, c, B[:, :1], 1, rtol=1e-30, maxit=1)   # (the hierarchy exists from here on)
    h = c.amg_hierarchy(capi.AMG_OF_HANDLE)
    if name == "dense":
        assert len(h["rows"]) == 1, "the hierarchy is the dense level alone"
    else:
        assert len(h["rows"]) >= 3, h["rows"]
    if name == "p1_3d":
        # some aggregate has more than four members: read from the level-0 map itself.  (The row counts say the same here -- the handle's matrix has no
        # Dirichlet rows, so every level-0 row belongs to an aggregate, and fewer than n / 4 of them means one has more than four members.)
        agg = c.amg_aggregates(capi.AMG_OF_HANDLE, 0)
        assert agg.shape == (h["rows"][0],) and agg.min() == 0 and agg.max() == h["rows"][1] - 1 and np.bincount(agg).max() > 4
        assert h["absorbed"] == 1 and 4 * h["rows"][1] < h["rows"][0], h["rows"]
    t0 = c.amg_cols_trace(capi.AMG_OF_HANDLE)
    for k in (1, 2, 5, None):
        kw = dict(rtol=1e-30, maxit=k) if k else dict(rtol=1e-10)
        X, info = _solve(capi, c, B, cols, **kw)
        R, ref = _solve(capi, c, B, 1, **kw)
        assert c.amg_hierarchy(capi.AMG_OF_HANDLE) == h, "the knob does not rebuild the hierarchy"
        print(f"{name} n_rhs {n_rhs} amg_cols {cols} k {k}: iterations {info.iters} / {ref.iters}, relres {info.relres:.3e} / {ref.relres:.3e}")
        assert _first_difference(X, R) == [], (name, k, "(column, first row, max |difference|)", _first_difference(X, R))
        assert info.iters == ref.iters and info.relres == ref.relres and info.converged == ref.converged
        assert not X[:, 2].any(), "the zero column is exactly zero"
        if k and name == "dense":   # (the preconditioner is the inverse: a column's Krylov space may be exhausted before k, and the single-column path takes it back)
            assert info.iters <= k * (n_rhs - 1)
        elif k:
            assert info.iters == k * (n_rhs - 1) and info.converged == 0   # (the zero column takes no iteration)
        else:
            assert info.converged == 1
            lu = spl.splu(s["A"].tocsc())
            for j in range(n_rhs):
                xr = lu.solve(B[:, j])
                assert np.linalg.norm(X[:, j] - xr) <= 1e-8 * np.linalg.norm(xr), j
    t1 = c.amg_cols_trace(capi.AMG_OF_HANDLE)
    assert t1["batches"] - t0["batches"] == 8 and t1["batched_cols"] - t0["batched_cols"] == 4 * (n_rhs - 1), (t0, t1)
    # columns a batch handed back to amg_run's warm start: what single_cols counts beyond the tail columns and the column-by-column runs
    handed = t1["single_cols"] - t0["single_cols"] - 4 * (1 + n_rhs)
    print(f"{name} n_rhs {n_rhs} amg_cols {cols}: {handed} column(s) handed back to the single-column path")
    assert handed >= 0
    if name == "dense":   # (the inverse exhausts a column's Krylov space at once; rtol 1e-30 never agrees: the hand-back ran, and the bits above are its)
        assert handed >= 1
    c.tune("amg_cols", 8)


def test_a_column_that_does_not_converge(env):
    """the advection system with maxit = the median of the columns' own iteration counts (read from `amg_cols` = 1 runs here): FDAPDE_ENOCONV, converged == 0; the
    columns that needed fewer iterations carry their converged bits, the others the maxit-th iterate of the column-by-column run"""
    capi, _ = env
    s = _system(env, "p1_2d_adr")
    c, B = s["c"], s["B"]
    full, counts = [], []
    for j in range(B.shape[1]):
        x, info = _solve(capi, c, B[:, j], 1, rtol=1e-10)
        assert info.converged == 1
        full.append(x), counts.append(info.iters)
    maxit = int(np.median([k for k in counts if k > 0]))
    assert min(k for k in counts if k > 0) < maxit < max(counts), ("the columns stop at different iterations", counts)
    R, ref = _solve(capi, c, B, 1, rtol=1e-10, maxit=maxit)
    c.tune("amg_cols", 8)
    opt = capi.Options(method=capi.SOLVER_AMG, maxit=maxit, rtol=1e-10, assembly=0, check_every=0, time_spmv=0)
    inf = capi.Info()
    flat = np.ascontiguousarray(B.T).reshape(-1)
    out = np.zeros_like(flat)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert c.lib.fdapde_lin_solve(c._ctx, C.byref(opt), dp(flat), B.shape[1], dp(out), C.byref(inf)) == capi.ENOCONV
    assert "maxit reached in at least one column" in c.lib.fdapde_last_error(c._ctx).decode()
    X = out.reshape(B.shape[1], B.shape[0]).T
    assert inf.converged == 0 and ref.converged == 0 and inf.iters == ref.iters and inf.relres == ref.relres
    print(f"iterations per column {counts}, maxit {maxit}")
    for j, k in enumerate(counts):
        assert np.array_equal(X[:, j], R[:, j]), j
        if k <= maxit:
            assert np.array_equal(X[:, j], full[j]), (j, "a column that converged within maxit carries its converged bits")
        else:
            assert not np.array_equal(X[:, j], full[j]), j


def test_sequence_and_state(env):
    """an in-place call with 8 columns; fdapde_lin_compute with new values: the next batch solves the new matrix and the trace restarts; a clone carries `amg_cols`"""
    import scipy.sparse.linalg as spl

    capi, _ = env
    s = _system(env, "p1_2d_sym")
    c, A, B = s["c"], s["A"], s["B"]
    c.tune("amg_cols", 8)
    R, _ = _solve(capi, c, B[:, :8], 1, rtol=1e-10)
    c.tune("amg_cols", 8)
    buf = np.ascontiguousarray(B[:, :8].T).reshape(-1).copy()
    opt = capi.Options(method=capi.SOLVER_AMG, maxit=0, rtol=1e-10, assembly=0, check_every=0, time_spmv=0)
    inf = capi.Info()
    ptr = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert c.lib.fdapde_lin_solve(c._ctx, C.byref(opt), ptr, 8, ptr, C.byref(inf)) == capi.OK
    assert np.array_equal(buf.reshape(8, -1).T, R), "x overlapping b: the batch read its columns before it wrote them"
    # new values on the same pattern
    A2 = A.copy()
    rows = np.repeat(np.arange(s["n"]), np.diff(A.indptr))
    A2.data = A.data * (1.0 + 0.3 * ((rows % 3 == 0) & (A.indices % 3 == 0)))
    c.lin_compute(values=A2.data, symmetric=True)
    X2, info2 = c.lin_solve(B[:, :8], method=capi.SOLVER_AMG)
    assert c.amg_cols_trace(capi.AMG_OF_HANDLE) == dict(batches=1, batched_cols=8, single_cols=0)
    lu2 = spl.splu(A2.tocsc())
    for j in range(8):
        xr = lu2.solve(B[:, j])
        assert np.linalg.norm(X2[:, j] - xr) <= 1e-8 * np.linalg.norm(xr), j
    # a clone carries the knob: 11 columns under amg_cols = 4 go as 4 + 4 + 2 + 1
    c.tune("amg_cols", 4)
    d = c.clone()
    Xd, _ = d.lin_solve(B, method=capi.SOLVER_AMG)
    assert d.amg_cols_trace(capi.AMG_OF_HANDLE) == dict(batches=3, batched_cols=10, single_cols=1)
    for j in range(B.shape[1]):   # (the clone builds its own hierarchy, under its own set-up knobs: its columns are held to the direct solve, not to the source's bits)
        xr = lu2.solve(B[:, j])
        assert np.linalg.norm(Xd[:, j] - xr) <= 1e-8 * np.linalg.norm(xr), j
    d.close()
    c.lin_compute(values=A.data, symmetric=True)
    c.tune("amg_cols", 8)


def test_multi_device_context_is_refused(env):
    capi, meshgen = env
    nodes, cells, bnd = meshgen.unit_square(16)
    c = capi.Context(devices=[0, 0])
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    c.lin_compute()   # (the handle itself serves multi-device contexts ...)
    c.tune("amg_cols", 8)
    with pytest.raises(capi.FdapdeError) as e:   # (... the multilevel method does not: the 8-column solve is what is refused)
        c.lin_solve(np.ones((nd, 8)), method=capi.SOLVER_AMG)
    assert e.value.status == capi.EUNSUPPORTED and "FDAPDE_SOLVER_AMG" in str(e.value)
    with pytest.raises(capi.FdapdeError) as e:
        c.amg_cols_trace(capi.AMG_OF_HANDLE)
    assert e.value.status == capi.ENOTINIT
    c.close()
