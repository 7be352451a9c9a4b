"""FDAPDE_SOLVER_AMG (csrc/eng_amg.hip): flexible GMRES around a K-cycle over an aggregation hierarchy built from the matrix alone, against scipy's SuperLU on
the reference's own row-zeroed system (fem_solver_base.h:142-155), on the parabolic stepper's implicit Euler system and on the factor-once handle's matrix.
Every problem switches `amg_setup_check` on: the device-built aggregates and coarse matrices are compared bit for bit with host loops."""
import os
import subprocess
import tempfile
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen

    assert capi.load().fdapde_device_count() >= 1
    return capi, meshgen


def _csr(c, capi, nd, which=None):
    import scipy.sparse as sp

    rp, ci = c.pattern_get()
    return sp.csr_matrix((c.matrix_values(capi.MAT_STIFF if which is None else which), ci, rp), shape=(nd, nd))


def _ctx(capi, meshgen, dim, nx, order):
    nodes, cells, bnd = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(order)
    c.tune("amg_setup_check", 1)
    return c, nd


def _problem(capi, meshgen, dim, nx, order, op, dirichlet, coarse_rows=None):
    c, nd = _ctx(capi, meshgen, dim, nx, order)
    if coarse_rows:
        c.tune("amg_coarse_rows", coarse_rows)
    _, bd, coords = c.dofs_get()
    c.set_operator(op)
    qn = c.quadrature_nodes()
    c.set_forcing(1.0 + np.sin(3.0 * qn[:, 0]) * qn[:, 1])
    if dirichlet == "zero":
        c.set_dirichlet(np.zeros(nd))
    elif dirichlet == "data":
        c.set_dirichlet(0.3 * np.cos(2.0 * coords[:, 0]) + coords[:, -1])
    c.init()
    return c, nd, bd, coords


def _op(capi, dim, kind):
    b = [3.0, -1.5] if dim == 2 else [1.0, 0.5, 0.25]
    K = np.array([[2.0, 0.3], [0.3, 1.0]]) if dim == 2 else np.array([[2.0, 0.3, 0.0], [0.3, 1.0, 0.1], [0.0, 0.1, 1.5]])
    return {"reaction": -capi.laplacian() + capi.reaction(2.0), "tensor": -capi.diffusion(K) + capi.reaction(0.5),
            "adr": -capi.laplacian() + capi.advection(b) + capi.reaction(1.0), "lap": -capi.laplacian()}[kind]


@pytest.mark.parametrize("dim,nx,order,kind,dirichlet", [
    (2, 48, 1, "reaction", "zero"), (2, 40, 1, "tensor", "data"), (2, 48, 1, "adr", "data"), (2, 40, 1, "adr", "none"),
    (2, 20, 2, "reaction", "data"), (2, 20, 2, "adr", "zero"),
    (3, 12, 1, "reaction", "data"), (3, 12, 1, "adr", "zero"), (3, 12, 1, "tensor", "none"),
    (3, 6, 2, "reaction", "zero"), (3, 6, 2, "adr", "data")])
def test_against_lu(env, dim, nx, order, kind, dirichlet):
    """2-D / 3-D, P1 / P2, -Lap + c, a diffusion tensor, -Lap + b.grad + c; zero, non-zero and no Dirichlet data: the LU solution of the row-zeroed system.
    A coarse limit of 256 rows gives every problem here several levels."""
    import scipy.sparse.linalg as spl

    capi, meshgen = env
    c, nd, _, _ = _problem(capi, meshgen, dim, nx, order, _op(capi, dim, kind), dirichlet, coarse_rows=256)
    info = c.solve(method=capi.SOLVER_AMG, rtol=1e-11)
    assert info.method_used == capi.SOLVER_AMG and info.converged == 1 and info.relres <= 1e-11
    assert info.persistent == 0 and info.iters <= 60, info.iters
    u = c.solution()
    ref = spl.spsolve(_csr(c, capi, nd).tocsc(), c.force())
    assert np.linalg.norm(u - ref) <= 1e-8 * np.linalg.norm(ref)
    again = c.solve(method=capi.SOLVER_AMG, rtol=1e-11)   # (the hierarchy is kept: the same iterations, the same bits)
    assert again.iters == info.iters and np.array_equal(c.solution(), u)
    c.close()


def test_small_system_is_one_dense_level(env):
    """a system below `amg_coarse_rows`: the hierarchy is the dense inverse alone, one outer iteration"""
    import scipy.sparse.linalg as spl

    capi, meshgen = env
    c, nd, _, _ = _problem(capi, meshgen, 2, 16, 1, _op(capi, 2, "adr"), "data")
    info = c.solve(method=capi.SOLVER_AMG)
    assert info.method_used == capi.SOLVER_AMG and info.converged == 1 and info.iters <= 2
    ref = spl.spsolve(_csr(c, capi, nd).tocsc(), c.force())
    assert np.linalg.norm(c.solution() - ref) <= 1e-8 * np.linalg.norm(ref)
    c.close()


def _ladder(capi, meshgen, dim, sizes):
    its = []
    for nx in sizes:   # (a coarse limit of 256 rows: the smallest sizes get a hierarchy too -- at the default 1 024, unit_cube(8) is one dense level, one iteration)
        c, nd, _, _ = _problem(capi, meshgen, dim, nx, 1, -capi.laplacian(), "zero", coarse_rows=256)
        info = c.solve(method=capi.SOLVER_AMG, rtol=1e-10)
        assert info.method_used == capi.SOLVER_AMG and info.converged == 1
        its.append(info.iters)
        c.close()
    return its


def test_iterations_do_not_grow_with_the_mesh_2d(env):
    capi, meshgen = env
    its = _ladder(capi, meshgen, 2, (32, 64, 128, 256, 512))
    print("2-D P1 -Lap, nx 32 .. 512:", its)
    assert max(its) <= 30 and its[-1] <= 1.5 * its[0] + 2, its


def test_iterations_do_not_grow_with_the_mesh_3d(env):
    capi, meshgen = env
    its = _ladder(capi, meshgen, 3, (8, 16, 32, 64))
    print("3-D P1 -Lap, nx 8 .. 64:", its)
    assert max(its) <= 30 and its[-1] <= 1.5 * its[0] + 2, its


@pytest.mark.parametrize("which", ["stiff", "mass"])
def test_handle(env, which):
    """lin_compute on a P1 stiffness / mass matrix, five columns against SuperLU; a second lin_compute with other values is the new matrix's (the
    hierarchy was built again); an in-place solve (x overlapping b)"""
    import scipy.sparse.linalg as spl

    capi, meshgen = env
    c, nd, _, _ = _problem(capi, meshgen, 2, 64, 1, _op(capi, 2, "reaction"), "none", coarse_rows=256)
    A = _csr(c, capi, nd, capi.MAT_STIFF if which == "stiff" else capi.MAT_MASS)
    rng = np.random.default_rng(7)
    B = rng.standard_normal((nd, 5))
    c.lin_compute(values=A.data, symmetric=True)
    X, info = c.lin_solve(B, method=capi.SOLVER_AMG)
    assert info.method_used == capi.SOLVER_AMG and info.converged == 1
    lu = spl.splu(A.tocsc())
    ref = lu.solve(B)
    for j in range(5):
        assert np.linalg.norm(X[:, j] - ref[:, j]) <= 1e-8 * np.linalg.norm(ref[:, j])
    A2 = A.copy()   # the entries among every third DOF scaled by 1.3: symmetric and positive definite again, the same pattern slots
    rows = np.repeat(np.arange(nd), np.diff(A.indptr))
    A2.data = A.data * (1.0 + 0.3 * ((rows % 3 == 0) & (A.indices % 3 == 0)))
    c.lin_compute(values=A2.data, symmetric=True)
    X2, info2 = c.lin_solve(B[:, :2], method=capi.SOLVER_AMG)
    ref2 = spl.spsolve(A2.tocsc(), B[:, :2])
    for j in range(2):
        assert np.linalg.norm(X2[:, j] - ref2[:, j]) <= 1e-8 * np.linalg.norm(ref2[:, j])
    # in place: x and b the same buffer
    import ctypes as C

    lib = capi.load()
    buf = np.ascontiguousarray(B[:, 0]).copy()
    opt = capi.Options(method=capi.SOLVER_AMG, maxit=0, rtol=1e-10, assembly=0, check_every=0, time_spmv=0)
    inf = capi.Info()
    ptr = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.fdapde_lin_solve(c._ctx, C.byref(opt), ptr, 1, ptr, C.byref(inf)) == capi.OK
    assert np.linalg.norm(buf - ref2[:, 0]) <= 1e-8 * np.linalg.norm(ref2[:, 0])
    c.close()


def test_stepper_against_lu_stepping(env):
    """fdapde_solve_parabolic by name, 2-D P1, 12 steps with Dirichlet data: every column against SuperLU stepping of the same implicit Euler system"""
    import scipy.sparse.linalg as spl

    capi, meshgen = env
    c, nd = _ctx(capi, meshgen, 2, 48, 1)
    c.tune("amg_coarse_rows", 256)
    _, bd, coords = c.dofs_get()
    c.set_operator(-capi.laplacian() + capi.advection([1.0, 0.5]) + capi.dt())
    times = np.linspace(0.0, 0.6, 12)
    qn = c.quadrature_nodes()
    c.set_forcing(np.stack([np.sin(2.0 * qn[:, 0]) * (1.0 + t) for t in times], axis=1))
    c.init()
    u0 = np.sin(np.pi * coords[:, 0]) * np.sin(np.pi * coords[:, 1])
    g = np.stack([0.1 * t * coords[:, 0] for t in times], axis=1)
    U, info = c.solve_parabolic(times, u0, dirichlet=g, method=capi.SOLVER_AMG, rtol=1e-12)
    assert info.method_used == capi.SOLVER_AMG and info.converged == 1
    dt = times[1] - times[0]
    A = _csr(c, capi, nd, capi.MAT_STIFF)
    M = _csr(c, capi, nd, capi.MAT_MASS)
    K = (M / dt + A).tolil()
    b_rows = np.flatnonzero(bd)
    for i in b_rows:
        K.rows[i], K.data[i] = [int(i)], [1.0]
    lu = spl.splu(K.tocsc())
    F = c.force(len(times)).reshape(len(times), nd).T   # (column after column)
    u = u0.copy()
    for i in range(len(times) - 1):
        rhs = M @ u / dt + F[:, i + 1]
        rhs[b_rows] = g[b_rows, i + 1]
        u = lu.solve(rhs)
        assert np.linalg.norm(U[:, i + 1] - u) <= 1e-8 * np.linalg.norm(u), i
    c.close()


def test_new_operator_rebuilds_the_hierarchy(env):
    import scipy.sparse.linalg as spl

    capi, meshgen = env
    c, nd, _, _ = _problem(capi, meshgen, 3, 12, 1, _op(capi, 3, "reaction"), "data", coarse_rows=256)
    c.solve(method=capi.SOLVER_AMG)
    c.set_operator(-capi.laplacian() + capi.advection([2.0, 0.0, -1.0]) + capi.reaction(5.0))
    c.init()
    info = c.solve(method=capi.SOLVER_AMG)
    assert info.converged == 1
    ref = spl.spsolve(_csr(c, capi, nd).tocsc(), c.force())
    assert np.linalg.norm(c.solution() - ref) <= 1e-8 * np.linalg.norm(ref)
    c.close()


def test_determinism_fresh_contexts_and_clone(env):
    capi, meshgen = env
    out = []
    for _ in range(2):
        c, nd, _, _ = _problem(capi, meshgen, 2, 96, 1, _op(capi, 2, "adr"), "data")
        info = c.solve(method=capi.SOLVER_AMG)
        out.append((info.iters, c.solution()))
        if len(out) == 1:
            d = c.clone()
            di = d.solve(method=capi.SOLVER_AMG)
            assert di.method_used == capi.SOLVER_AMG and di.iters == info.iters and np.array_equal(d.solution(), out[0][1])
            d.close()
        c.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])


def test_pure_neumann_is_refused(env):
    """-Lap with no Dirichlet data and a forcing outside the range: no answer, FDAPDE_ENOCONV"""
    capi, meshgen = env
    c, nd = _ctx(capi, meshgen, 2, 64, 1)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    info = c.solve(method=capi.SOLVER_AMG, raise_on_noconv=False)
    assert info.converged == 0
    with pytest.raises(capi.FdapdeError) as e:
        c.solve(method=capi.SOLVER_AMG)
    assert e.value.status == capi.ENOCONV
    assert str(e.value) == (f"[status {capi.ENOCONV}] FDAPDE_SOLVER_AMG: the coarsest level is singular to working precision "
                            "(a pure Neumann problem has no unique solution)")
    c.close()


def test_multi_device_context_is_refused_at_once(env):
    capi, meshgen = env
    nodes, cells, bnd = meshgen.unit_square(16)
    c = capi.Context(devices=[0, 0])
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(1)
    c.set_operator(-capi.laplacian())
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.set_dirichlet(np.zeros(c.sizes()["n_dofs"]))
    c.init()
    t0 = time.monotonic()
    with pytest.raises(capi.FdapdeError) as e:
        c.solve(method=capi.SOLVER_AMG)
    assert time.monotonic() - t0 < 5.0
    assert "FDAPDE_SOLVER_AMG" in str(e.value)
    c.close()


def test_randomised_against_superlu(env):
    """40 seeded problems: order, dimension, operator terms, coefficient fields, Dirichlet masks; the worst error and the most iterations recorded"""
    import scipy.sparse.linalg as spl

    capi, meshgen = env
    worst, most = 0.0, 0
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        dim = int(rng.integers(2, 4))
        order = int(rng.integers(1, 3))
        nx = int(rng.integers(14, 40)) if dim == 2 else int(rng.integers(5, 10))
        if order == 2:
            nx = max(4, nx // 2)
        c, nd = _ctx(capi, meshgen, dim, nx, order)
        c.tune("amg_coarse_rows", int(rng.choice([64, 256, 1024])))
        _, bd, coords = c.dofs_get()
        mask = rng.random()
        part = (bd != 0) if mask < 0.4 else ((bd != 0) & (coords[:, 0] < 0.5)) if mask < 0.7 else np.zeros(nd, dtype=bool)
        if mask >= 0.4 and part.any():   # Dirichlet data on a part of the boundary only
            c.dofs_set_boundary(part.astype(np.uint8))
        qn = c.quadrature_nodes()
        op = -capi.laplacian() if rng.random() < 0.5 else -capi.diffusion_field(np.tile(np.eye(dim).reshape(-1), (qn.shape[0], 1)) * (1.0 + 0.5 * np.sin(3.0 * qn[:, :1])))
        if rng.random() < 0.5:
            op = op + capi.advection(list(rng.uniform(-3.0, 3.0, dim)))
        reaction = rng.random() < 0.6
        if reaction:
            op = op + (capi.reaction(float(rng.uniform(0.1, 3.0))) if rng.random() < 0.5 else capi.reaction_field(1.0 + qn[:, 0] ** 2))
        if not (reaction or part.any()):   # (no Dirichlet data, no reaction: singular -- test_pure_neumann_is_refused)
            c.close()
            continue
        c.set_operator(op)
        c.set_forcing(rng.uniform(-1.0, 1.0) + np.cos(2.0 * qn[:, 1]))
        if part.any():
            c.set_dirichlet(np.where(part, np.sin(coords[:, 1]), 0.0))
        c.init()
        info = c.solve(method=capi.SOLVER_AMG, rtol=1e-11)
        assert info.method_used == capi.SOLVER_AMG and info.converged == 1, seed
        ref = spl.spsolve(_csr(c, capi, nd).tocsc(), c.force())
        err = np.linalg.norm(c.solution() - ref) / np.linalg.norm(ref)
        worst, most = max(worst, err), max(most, info.iters)
        assert err <= 1e-8, (seed, err)
        c.close()
    print(f"randomised: worst relative error {worst:.2e}, most iterations {most}")


_CPP = r"""
#include <cmath>
#include <cstdio>
#include "fdapde_amd/pde.h"
#include "fdapde_amd/io.h"
using namespace fdapde::amd;
int main(int argc, char** argv) {
    MeshLoader<2, 2> m(argv[1], "unit_square_32");
    auto L = -laplacian<FEM_HIP>() + reaction<FEM_HIP>(2.0);
    PDE<Triangulation<2, 2>, decltype(L), DMatrix<double>, FEM_HIP, fem_order<1>> pde_(m.mesh, L);
    pde_.init();
    auto invA = pde_.make_solver();
    invA.solver_options().method = FDAPDE_SOLVER_AMG;
    invA.compute(pde_.stiff(), true);
    DMatrix<double> X(pde_.n_dofs(), 2);
    for (int64_t i = 0; i < X.rows(); ++i)
        for (int j = 0; j < 2; ++j) X(i, j) = std::sin(0.01 * i * (j + 1)) + j;
    DMatrix<double> B = pde_.stiff() * X;
    DMatrix<double> Y = invA.solve(B);
    fdapde_info info;
    fdapde_info_get(pde_.context(), &info);
    double worst = 0;
    for (int64_t i = 0; i < X.rows(); ++i)
        for (int j = 0; j < 2; ++j) worst = std::fmax(worst, std::fabs(X(i, j) - Y(i, j)));
    std::printf("method %d worst %.3e\n", info.method_used, worst);
    return (info.method_used == FDAPDE_SOLVER_AMG && worst < 1e-7) ? 0 : 1;
}
"""


def test_cpp_facade_names_amg_for_the_handle(env):
    capi, _ = env
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "amg.cpp"), os.path.join(d, "amg")
        open(src, "w").write(_CPP)
        lib = os.path.join(ROOT, "fdapde-core_amd", "lib")
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-I" + os.path.join(ROOT, "include"), src, "-L" + lib, "-lfdapde_hip", "-Wl,-rpath," + lib,
                               "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o", exe])
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "mesh")], capture_output=True, text=True, timeout=300)
        print(r.stdout)
        assert r.returncode == 0, r.stdout + r.stderr
