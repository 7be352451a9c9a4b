"""Blocks of the single-launch CG by coordinate bisection (knob persist_partition 1; csrc/host_bisect.cpp, csrc/dev_persist.hip) against the
contiguous chunks of the internal order (knob 0) and the automatic choice (knob 2, the default): the same system, the same recurrence, another
assignment of rows to workgroups -- so both converge, in the same number of iterations (+-1: the dot products are summed in another order),
to the same solution as the multi-launch path within the bars of tests/test_gpu_persist.py, bit for bit the same from launch to launch; the
automatic choice never streams more bytes than the chunks; and the device builder's bisection layout equals the host builder's array for
array (FDAPDE_SETUP_CHECK), also where the coordinates are degenerate along an axis (surfaces, networks)."""
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


def _problem(capi, meshgen, dim, nx, order, dirichlet=True):
    nodes, cells, bnd = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
    _, f = meshgen.manufactured(dim)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd if dirichlet else np.zeros_like(bnd))
    nd = c.dofs_build(order)
    _, _, coords = c.dofs_get()
    c.set_operator(-capi.laplacian() + (capi.reaction(0.0) if dirichlet else capi.reaction(1.0)))
    c.set_forcing(f(c.quadrature_nodes()))
    c.set_dirichlet(0.25 * coords[:, 0] if dirichlet else None)
    c.init()
    return c, nd


@pytest.mark.parametrize("dim,nx,order,dirichlet", [
    (2, 60, 1, True),      # 3 721 DOFs: two workgroups, host-built layouts
    (2, 60, 2, True),      # P2 rows
    (2, 150, 1, False),    # no Dirichlet DOF: every row interior
    (3, 30, 1, True),      # 3-D rows, device-built from here on
    (3, 12, 2, True),      # 3-D P2 rows (up to 64 entries)
    (2, 708, 1, True),     # C2: one workgroup per CU, blocks resident
    (3, 64, 1, True),      # symmetric blocks resident
    (2, 1000, 1, True),    # symmetric storage, 8 rows per thread, blocks stream
    (3, 105, 1, True),     # 16 rows per thread, blocks stream (C3's form)
])
def test_bisection_blocks_match_chunks_and_the_multi_launch_path(env, dim, nx, order, dirichlet):
    capi, meshgen = env
    c, nd = _problem(capi, meshgen, dim, nx, order, dirichlet)
    c.tune("persist", 0)
    i_ref = c.solve(rtol=1e-10)
    u_ref = c.solution()
    assert i_ref.persistent == 0 and i_ref.converged == 1
    c.tune("persist", 1)
    iters, nbytes, kinds, parts = {}, {}, {}, {}
    for knob in (0, 1, 2):
        c.tune("persist_partition", knob)
        i1 = c.solve(rtol=1e-10)
        u1 = c.solution()
        assert i1.persistent == 1, "the system qualifies: the single-launch path must have run"
        assert i1.converged == 1 and i1.relres <= 1e-10
        assert abs(i1.iters - i_ref.iters) <= max(1, i_ref.iters // 200), (knob, i1.iters, i_ref.iters)
        assert np.linalg.norm(u1 - u_ref) <= 1e-9 * np.linalg.norm(u_ref), knob
        i2 = c.solve(rtol=1e-10)   # a second launch on the same layout: identical bits
        assert i2.iters == i1.iters and np.array_equal(c.solution(), u1), knob
        iters[knob], nbytes[knob], kinds[knob] = i1.iters, c.solver_layout(dirichlet)[2], c.solver_layout_kind(dirichlet)
        parts[knob] = c.solver_layout_partition(dirichlet)
    print(f"{dim}-D nx {nx} P{order}: iterations {iters}, streamed bytes {nbytes}, partition {parts}, layouts {kinds}")
    assert parts[0] == 0, "knob 0: chunks of the internal order"
    assert parts[1] == 1 or (nbytes[1] == nbytes[0] and kinds[1] == kinds[0]), "knob 1: bisection blocks, or -- where they do not fit -- the chunk layout as it was"
    assert parts[2] == (1 if parts[1] == 1 and nbytes[1] < nbytes[0] else 0), "knob 2: bisection exactly where it fits and moves fewer bytes"
    assert abs(iters[1] - iters[0]) <= 1, iters
    assert nbytes[2] <= nbytes[0], nbytes
    assert kinds[1]["workgroups"] == kinds[0]["workgroups"]
    assert nbytes[2] == min(nbytes[0], nbytes[1]), nbytes   # the automatic choice: bisection exactly where it moves fewer bytes
    assert kinds[2] == (kinds[1] if nbytes[1] < nbytes[0] else kinds[0])
    c.close()


def _check_layouts(c, capsys):
    c.tune("persist_partition", 1)
    c.solver_prepare(True)     # raises FdapdeError(EHIP) on the first mismatch, details on stderr
    c.solver_prepare(False)
    err = capsys.readouterr().err
    print("\n".join(l for l in err.splitlines() if l.startswith("persist check")))
    assert "MISMATCH" not in err
    assert err.count("persist check slot_dof ") == 4, "per boundary variant: the chunk layout and the bisection layout, each against the host builder's"
    return err.count("bis_perm : ok")


@pytest.mark.parametrize("dim,nx,order", [(2, 300, 1), (2, 1000, 1), (3, 24, 2), (3, 64, 1), (3, 119, 1)])   # the last one: C3
def test_device_built_bisection_equals_the_host_builders(env, dim, nx, order, monkeypatch, capfd):
    capi, meshgen = env
    monkeypatch.setenv("FDAPDE_SETUP_CHECK", "1")
    nodes, cells, bnd = meshgen.unit_square(nx) if dim == 2 else meshgen.unit_cube(nx)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(order)
    assert _check_layouts(c, capfd) == 2, "both boundary variants must have built (and compared) a bisection layout on the device"
    assert c.solver_layout_partition(True) == 1 and c.solver_layout_partition(False) == 1, "knob 1 on these systems: the bisection layout is the one in use"
    _, f = meshgen.manufactured(dim)
    c.set_operator(-capi.laplacian())
    c.set_forcing(f(c.quadrature_nodes()))
    c.set_dirichlet(np.zeros(nd))
    c.init()
    assert c.solve(rtol=1e-10).converged == 1
    c.close()


@pytest.mark.parametrize("which,order", [("surface", 1), ("surface", 2), ("network", 1), ("network", 2)])
def test_bisection_where_the_coordinates_are_degenerate(env, which, order, monkeypatch, capfd):
    """a height field (hardly any extent along one axis) and a street network (1-D cells in the plane): the partition is still a permutation with
    no empty block -- the layout builders refuse anything else --, the device's equals the host's, and the solve through it converges to the
    multi-launch path's solution"""
    capi, meshgen = env
    monkeypatch.setenv("FDAPDE_SETUP_CHECK", "1")
    if which == "surface":
        nodes, cells, bnd = meshgen.height_field_surface(200, amplitude=0.01)
    else:
        nodes, cells, bnd = meshgen.street_grid(60, 50, k=8, seed=3, drop=0.1)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(order)
    assert nd > 32768, "large enough for the device builder"
    assert _check_layouts(c, capfd) == 2   # (built and compared for both variants; knob 1 keeps the chunks where the bisection layout needs more rows per
    print(f"{which} P{order}: partition in use {c.solver_layout_partition(True)} / {c.solver_layout_partition(False)}")   # thread or leaves the LDS: printed)
    monkeypatch.delenv("FDAPDE_SETUP_CHECK")
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.set_dirichlet(np.zeros(nd))
    c.init()
    c.tune("persist", 0)
    i0 = c.solve(rtol=1e-10)
    u0 = c.solution()
    c.tune("persist", 1)
    i1 = c.solve(rtol=1e-10)
    assert i1.persistent == 1 and i1.converged == 1 and abs(i1.iters - i0.iters) <= max(1, i0.iters // 200)
    assert np.linalg.norm(c.solution() - u0) <= 1e-9 * np.linalg.norm(u0)
    assert c.solver_layout_kind(True)["workgroups"] >= 2
    c.close()


def test_full_size_system_keeps_its_iteration_count(env):
    """C3 (119^3 x 6 tetrahedra, 1.728 M DOFs): 503 +- 1 iterations with either partition, identical bits from launch to launch, and the
    automatic choice streams no more than the chunks"""
    capi, meshgen = env
    nodes, cells, bnd = meshgen.unit_cube(119)
    _, f = meshgen.manufactured(3)
    c = capi.Context(0)
    c.mesh_upload(nodes, cells, bnd)
    nd = c.dofs_build(1)
    c.set_operator(-capi.laplacian())
    c.set_forcing(f(c.quadrature_nodes()))
    c.set_dirichlet(np.zeros(nd))
    c.init()
    out = {}
    for knob in (0, 1, 2):
        c.tune("persist_partition", knob)
        i1 = c.solve(rtol=1e-10)
        u1 = c.solution()
        assert i1.persistent == 1 and i1.converged == 1
        i2 = c.solve(rtol=1e-10)
        assert i2.iters == i1.iters and np.array_equal(c.solution(), u1)
        assert c.solver_layout_partition(True) == (0 if knob == 0 else 1)
        out[knob] = (i1.iters, c.solver_layout(True)[2], 1e3 * i2.launch_ms / i2.iters, u1)
    print("C3: " + "  ".join(f"partition={k}: {v[0]} it, {v[1]:.0f} B/it, {v[2]:.2f} us/it" for k, v in out.items()))
    assert abs(out[0][0] - out[1][0]) <= 1 and abs(out[0][0] - 503) <= 1 and abs(out[1][0] - 503) <= 1
    assert out[2][1] <= out[0][1]
    assert np.linalg.norm(out[1][3] - out[0][3]) <= 1e-8 * np.linalg.norm(out[0][3])
    c.close()
