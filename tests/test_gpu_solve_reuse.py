"""fdapde_solve keeps the Jacobi-scaled system (scale, scaled copy, filled solver layout) across solves of an unchanged matrix (knob solve_reuse,
counter fdapde_solve_reuse_count; csrc/eng_solve.hip solve_prepare, fdapde_ctx::Prepared).  What is kept is bit for bit what a full prepare would
write again, so every solve must give the bits of a context that prepares in full every time (solve_reuse 0) -- on every branch of the prepare --,
and whatever can change the system between two solves must make the next solve prepare in full: compared bit for bit with a fresh context that makes
the same calls without the history (and with solve_reuse 0).  The oracle's solution for a changed forcing is matched after reuse within the bars of tests/test_gpu_parity.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-8   # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen

    assert capi.load().fdapde_device_count() >= 1
    return capi, meshgen


_meshes = {}


def _mesh(meshgen, dim, nx):
    if (dim, nx) not in _meshes:
        _meshes[(dim, nx)] = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
    return _meshes[(dim, nx)]


def _context(capi, meshgen, dim, nx, order, op=None, knobs=(), cols=1):
    """mesh, space, operator, forcing (cols columns), Dirichlet data 0.25 x on the boundary DOFs; no fdapde_init yet"""
    nodes, cells, bnd = _mesh(meshgen, dim, nx)
    _, f = meshgen.manufactured(dim)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(order)
    _, _, coords = c.dofs_get()
    for key, value in knobs:
        c.tune(key, value)
    c.set_operator(op if op is not None else -capi.laplacian())
    fq = f(c.quadrature_nodes())
    c.set_forcing(fq if cols == 1 else np.stack([(1.0 + 0.5 * k) * fq for k in range(cols)], axis=1))
    c.set_dirichlet(0.25 * coords[:, 0])
    return c, coords


def _solve(c, **kw):
    i = c.solve(rtol=1e-10, raise_on_noconv=False, **kw)
    return (i.iters, i.relres, i.converged, i.method_used, i.persistent), c.solution()


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), (what, "solution bits differ", float(np.abs(a[1] - b[1]).max()))


# (dim, nx, order, advection, persist, single launch expected, hits expected): the smallest shapes that reach each branch of the prepare
SHAPES = [
    pytest.param(2, 60, 1, False, 1, 1, True, id="2d-nx60-P1-deferred-flag"),           # 3 721 DOFs: the flag is not waited for, no front kernel
    pytest.param(3, 30, 1, False, 1, 1, True, id="3d-nx30-P1-resident"),                 # 29 workgroups, blocks resident
    pytest.param(3, 12, 2, False, 1, 1, True, id="3d-nx12-P2-streaming"),                # 26 workgroups, blocks stream
    pytest.param(3, 64, 1, False, 1, 1, True, id="3d-nx64-P1-symmetric-storage"),        # 256 workgroups, 302 iterations
    pytest.param(2, 60, 1, True, 1, 1, True, id="2d-nx60-advection-single-launch-bicgstab"),
    pytest.param(3, 30, 1, False, 0, 0, True, id="3d-nx30-P1-persist0-compact-pattern"),  # multi-launch CG on the compact CSR pattern
    pytest.param(2, 16, 1, False, 1, 1, False, id="2d-nx16-P1-front-kernel"),            # 289 DOFs: k_small_front scales and fills, nothing is reused
]


@pytest.mark.parametrize("dim,nx,order,advection,persist,launch,hits", SHAPES)
def test_same_bits_with_and_without_reuse(env, dim, nx, order, advection, persist, launch, hits):
    capi, meshgen = env
    op = (-capi.laplacian() + capi.advection(np.array([1.0, 0.5, 0.25][:dim]))) if advection else None
    runs, counts = {}, {}
    for reuse in (1, 0):
        c, coords = _context(capi, meshgen, dim, nx, order, op=op, knobs=(("persist", persist), ("solve_reuse", reuse)))
        out, cnt = [], []
        c.init()
        out.append(_solve(c)), cnt.append(c.solve_reuse_count())
        c.init()
        out.append(_solve(c)), cnt.append(c.solve_reuse_count())
        c.set_dirichlet(0.25 * coords[:, 0] + 0.5 + coords[:, 1] ** 2)   # other values on the same DOFs
        out.append(_solve(c)), cnt.append(c.solve_reuse_count())
        runs[reuse], counts[reuse] = out, cnt
        c.close()
    print([o[0] for o in runs[1]], counts)
    for k in range(3):
        _same(runs[1][k], runs[0][k], f"solve {k}")
        assert runs[1][k][0][2] == 1 and runs[1][k][0][4] == launch, runs[1][k][0]
    if advection:
        assert runs[1][0][0][3] == capi.SOLVER_BICGSTAB
    assert not np.array_equal(runs[1][2][1], runs[1][1][1]), "the third solve has other Dirichlet values"
    assert counts[1] == ([0, 1, 2] if hits else [0, 0, 0]), counts
    assert counts[0] == [0, 0, 0], counts


def _reaction_op(capi, cr=1.0):
    return -capi.laplacian() + capi.reaction(cr)   # (positive definite without Dirichlet data as well)


def _with_one_hit(capi, meshgen, dim, nx, order, cols=1, knobs=()):
    c, coords = _context(capi, meshgen, dim, nx, order, op=_reaction_op(capi), cols=cols, knobs=knobs)
    c.init()
    _solve(c)
    c.init()
    _solve(c)
    assert c.solve_reuse_count() == 1
    return c, coords


def _fresh(capi, meshgen, dim, nx, order, cols=1, knobs=(), init=True):
    c, coords = _context(capi, meshgen, dim, nx, order, op=_reaction_op(capi), cols=cols, knobs=knobs)
    if init:
        c.init()
    return c, coords


def _missed(c, before):
    assert c.solve_reuse_count() == before, "the solve after this call must prepare in full"


def _forget_set_operator(capi, c, coords, history):
    c.set_operator(_reaction_op(capi, 3.0))
    c.init()
    return [_solve(c)]


def _forget_assemble(capi, c, coords, history):
    c.assemble_operator(capi.MAT_STIFF, _reaction_op(capi, 3.0))
    return [_solve(c)]


def _forget_other_assembly(capi, c, coords, history):
    c.init(assembly=capi.ASSEMBLY_COLOURED)
    return [_solve(c)]


def _forget_dirichlet_off_and_on(capi, c, coords, history):
    c.set_dirichlet(None)
    out = [_solve(c)]
    if history:
        _missed(c, 1)
    c.set_dirichlet(0.25 * coords[:, 0])
    return out + [_solve(c)]


def _forget_parabolic(capi, c, coords, history):
    c.solve_parabolic(np.array([0.0, 0.01, 0.02]), np.zeros(coords.shape[0]))
    return [_solve(c)]


def _forget_lin(capi, c, coords, history):
    c.lin_compute(capi.MAT_MASS, symmetric=True)
    c.lin_solve(np.ones(coords.shape[0]))
    return [_solve(c)]


def _forget_named(method):
    def go(capi, c, coords, history):
        i = c.solve(method=getattr(capi, method), rtol=1e-10)
        assert i.converged == 1 and i.method_used == getattr(capi, method)
        return [_solve(c)]
    return go


def _forget_knob(key, value):
    def go(capi, c, coords, history):
        c.tune(key, value)
        return [_solve(c)]
    return go


def _forget_indefinite(capi, c, coords, history):
    c.set_operator(-capi.laplacian() + capi.reaction(-100.0))   # symmetric, indefinite: the CG stage breaks down
    c.init()
    first = _solve(c)
    if history:
        _missed(c, 1)
    second = _solve(c)
    cg = (capi.SOLVER_CG, capi.SOLVER_CG_SR, capi.SOLVER_CG_FUSED)
    assert first[0][3] not in cg and second[0][3] == first[0][3] and second[0][0] == first[0][0], (first[0], second[0])
    return [first, second]


FORGET = [
    pytest.param(3, 12, 1, 1, _forget_set_operator, id="set_operator-and-init"),
    pytest.param(3, 12, 1, 1, _forget_assemble, id="assemble-stiffness"),
    pytest.param(3, 12, 1, 1, _forget_other_assembly, id="init-coloured-assembly"),
    pytest.param(3, 12, 1, 1, _forget_dirichlet_off_and_on, id="dirichlet-off-and-on"),
    pytest.param(3, 12, 1, 3, _forget_parabolic, id="parabolic-solve-between"),
    pytest.param(3, 12, 1, 1, _forget_lin, id="lin-compute-and-solve-between"),
    pytest.param(2, 24, 2, 1, _forget_named("SOLVER_PMG"), id="solve-by-name-pmg"),
    pytest.param(2, 24, 2, 1, _forget_named("SOLVER_AMG"), id="solve-by-name-amg"),
    pytest.param(2, 24, 2, 1, _forget_named("SOLVER_DENSE"), id="solve-by-name-dense"),
    pytest.param(3, 12, 1, 1, _forget_knob("persist_partition", 0), id="knob-persist_partition"),
    pytest.param(3, 12, 1, 1, _forget_knob("persist", 0), id="knob-persist"),
    pytest.param(2, 60, 1, 1, _forget_indefinite, id="indefinite-cg-breakdown"),
]


@pytest.mark.parametrize("dim,nx,order,cols,action", FORGET)
def test_every_way_of_forgetting(env, dim, nx, order, cols, action):
    capi, meshgen = env
    c, coords = _with_one_hit(capi, meshgen, dim, nx, order, cols=cols)
    got = action(capi, c, coords, True)
    if action not in (_forget_dirichlet_off_and_on, _forget_indefinite):   # (they count their first solve themselves; their second one follows another full prepare)
        _missed(c, 1)
    f, fcoords = _fresh(capi, meshgen, dim, nx, order, cols=cols, knobs=(("solve_reuse", 0),))   # (... and never reuses anything itself)
    want = action(capi, f, fcoords, False)
    assert f.solve_reuse_count() == 0
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        _same(a, b, f"solve {k} after the call")
    c.close(), f.close()


def test_a_clone_prepares_its_first_solve_in_full(env):
    capi, meshgen = env
    c, coords = _with_one_hit(capi, meshgen, 3, 12, 1)
    d = c.clone()
    got = _solve(d)
    assert d.solve_reuse_count() == 0
    f, _ = _fresh(capi, meshgen, 3, 12, 1, knobs=(("solve_reuse", 0),))
    _same(got, _solve(f), "the clone's first solve")
    again = _solve(d)   # ... and keeps a record of its own from then on
    assert d.solve_reuse_count() == 1
    _same(again, got, "the clone's second solve")
    c.close(), d.close(), f.close()


def test_parity_with_the_oracle_after_reuse(env, oracle):
    capi, meshgen = env
    nodes, cells, bnd = _mesh(meshgen, 3, 30)
    m = oracle.Mesh(np.ascontiguousarray(nodes, dtype=float), np.ascontiguousarray(cells, dtype=np.int32), np.ascontiguousarray(bnd, dtype=np.uint8))
    c, coords = _context(capi, meshgen, 3, 30, 1)
    g = 0.25 * coords[:, 0]
    c.init()
    _solve(c)
    c.init()
    _solve(c)
    fq = np.cos(3.0 * c.quadrature_nodes()).prod(axis=1) + 2.0   # another forcing: the matrix keeps its epoch, the load vector is new
    c.set_forcing(fq)
    c.init()
    info, u = _solve(c)
    assert c.solve_reuse_count() == 2 and info[2] == 1 and info[1] <= 1e-10
    ref = oracle.pde_init_solve(m, 1, -oracle.laplacian(), forcing_q=fq, dirichlet=g, direct=True)
    err = np.linalg.norm(u - ref.solution) / np.linalg.norm(ref.solution)
    print(f"after two reuses: |u - u_oracle| / |u_oracle| = {err:.3e}")
    assert err <= SOL_TOL
    c.close()
