"""The export stores of the single-launch CG (kernels_persist.h: every workgroup publishes the entries of p its neighbours import at the top
of each iteration) in the forms that have neighbours -- plain storage resident or streaming, symmetric storage streaming -- on systems of
many workgroups: the same iteration count as the multi-launch path, the same solution to rounding, the same bits from launch to launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, meshgen

    assert capi.load().fdapde_device_count() >= 1
    return capi, meshgen


def _problem(capi, meshgen, dim, nx, order):
    nodes, cells, bnd = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
    _, f = meshgen.manufactured(dim)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(order)
    _, _, coords = c.dofs_get()
    c.set_operator(-capi.laplacian())
    c.set_forcing(f(c.quadrature_nodes()))
    c.set_dirichlet(0.25 * coords[:, 0])
    c.init()
    return c


@pytest.mark.parametrize("dim,nx,order,sym", [
    (3, 30, 1, 0),     # plain storage
    (3, 12, 2, 0),     # P2 rows
    (3, 64, 1, 0),     # plain blocks stream
    (3, 105, 1, 1),    # symmetric blocks stream, 16 rows per thread (C3's form)
    (2, 1000, 1, 1),   # symmetric blocks stream, 8 rows per thread
])
def test_exported_entries_reach_every_neighbour(env, dim, nx, order, sym):
    capi, meshgen = env
    c = _problem(capi, meshgen, dim, nx, order)
    c.tune("persist", 0)
    i_ml = c.solve(rtol=1e-10)
    u_ml = c.solution()
    assert i_ml.persistent == 0 and i_ml.converged == 1
    c.tune("persist", 1)
    c.tune("persist_sym", sym)
    i1 = c.solve(rtol=1e-10)
    u1 = c.solution()
    lk = c.solver_layout_kind(True)
    assert i1.persistent == 1 and i1.converged == 1 and i1.relres <= 1e-10
    assert lk["kind"] in (2, 3) and lk["sym"] == sym and lk["workgroups"] > 1, lk
    assert abs(i1.iters - i_ml.iters) <= max(1, i_ml.iters // 200), (i1.iters, i_ml.iters)
    assert np.linalg.norm(u1 - u_ml) <= 1e-9 * np.linalg.norm(u_ml)
    for _ in range(2):
        i2 = c.solve(rtol=1e-10)
        assert i2.persistent == 1 and i2.iters == i1.iters and np.array_equal(c.solution(), u1)
    c.close()
