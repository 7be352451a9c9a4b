"""CPU-side checks: the C-ABI library loads and exports every declared symbol; the host-side index work
(DOF numbering, boundary sets, DOF coordinates, CSR pattern) is bit-exact against the oracle; compute entry points
refuse to run without a device (no CPU fallback)."""
import os
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def capi():
    from fdapde_loader import load_package

    return load_package().capi


def test_library_exports_every_declared_symbol(capi):
    lib = capi.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fdapde_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(fdapde_[a-z_0-9]+)\s*\(", header)))
    assert declared, "no declarations parsed"
    assert sorted(capi.SYMBOLS) == declared
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.fdapde_abi_version() == 5


FIXTURES = ["unit_square_16", "unit_square_32", "unit_square_64", "unit_square", "c_shaped", "quasi_circle", "unit_sphere"]


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("order", [1, 2])
def test_numbering_and_pattern_bit_exact(capi, oracle, mesh_loader, name, order):
    m = mesh_loader(name)
    ctx = capi.Context(device=None)
    ctx.mesh_upload(m.nodes, m.cells, m.boundary)
    nd = ctx.dofs_build(order)
    dofs, bnd, coords = ctx.dofs_get()
    od, ob, ond, one = oracle.enumerate_dofs(m, order)
    assert nd == ond and ctx.sizes()["n_edges"] == one
    assert np.array_equal(dofs, od) and np.array_equal(bnd, ob)
    assert np.array_equal(coords, oracle.dofs_coords(m, order, od, ond))
    A = oracle.assemble_operator(m, order, od, ond, -oracle.laplacian())
    rp, ci = ctx.pattern_get()
    assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colidx)
    ctx.close()


def test_compute_fails_loudly_without_device(capi, mesh_loader):
    m = mesh_loader("unit_square_16")
    ctx = capi.Context(device=None)
    ctx.mesh_upload(m.nodes, m.cells, m.boundary)
    ctx.dofs_build(1)
    ctx.set_operator(-capi.laplacian())
    for call in (ctx.init, ctx.solve, ctx.solution, ctx.quadrature_nodes, lambda: ctx.matrix_values(0)):
        with pytest.raises(capi.FdapdeError) as e:
            call()
        assert e.value.status == capi.ENODEVICE
    ctx.close()


def test_argument_validation(capi, mesh_loader):
    m = mesh_loader("unit_square_16")
    ctx = capi.Context(device=None)
    bad = m.cells.copy()
    bad[0, 0] = m.n_nodes + 5
    with pytest.raises(capi.FdapdeError) as e:
        ctx.mesh_upload(m.nodes, bad, m.boundary)
    assert e.value.status == capi.EINVAL
    ctx.mesh_upload(m.nodes, m.cells, m.boundary)
    with pytest.raises(capi.FdapdeError) as e:
        ctx.dofs_build(3)   # LagrangianBasis::enumerate_dofs requires Order <= 2 (lagrangian_basis.h:94)
    assert e.value.status == capi.EUNSUPPORTED
    with pytest.raises(capi.FdapdeError) as e:
        ctx.set_operator(-capi.laplacian())   # before dofs_build
    assert e.value.status == capi.ENOTINIT
    ctx.close()


def test_unreferenced_node_is_rejected(capi):
    """a node no cell references gives an empty matrix row; the reference's SparseLU would fail (success = false)"""
    nodes = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [5.0, 5.0]])
    cells = np.array([[0, 1, 2]], dtype=np.int32)
    ctx = capi.Context(device=None)
    ctx.mesh_upload(nodes, cells, np.ones(4, dtype=np.uint8))
    with pytest.raises(capi.FdapdeError) as e:
        ctx.dofs_build(1)
    assert e.value.status == capi.EINVAL
    ctx.close()


@pytest.mark.parametrize("order", [1, 2])
def test_minimal_meshes(capi, oracle, order):
    """one triangle, one tetrahedron, two tetrahedra sharing a face: numbering and pattern as the oracle's"""
    tri = (np.array([[0.0, 0.0], [1.0, 0.2], [0.1, 0.9]]), np.array([[0, 1, 2]], dtype=np.int32))
    tet = (np.array([[0.0, 0, 0], [1.0, 0.1, 0], [0, 1.0, 0.2], [0.1, 0.2, 1.0]]), np.array([[0, 1, 2, 3]], dtype=np.int32))
    two = (np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 1.0, 1.0]]), np.array([[0, 1, 2, 3], [4, 2, 1, 3]], dtype=np.int32))
    for nodes, cells in (tri, tet, two):
        m = oracle.Mesh(nodes, cells, np.ones(nodes.shape[0], dtype=np.uint8))
        ctx = capi.Context(device=None)
        ctx.mesh_upload(m.nodes, m.cells, m.boundary)
        nd = ctx.dofs_build(order)
        od, ob, ond, _ = oracle.enumerate_dofs(m, order)
        dofs, bnd, coords = ctx.dofs_get()
        assert nd == ond and np.array_equal(dofs, od) and np.array_equal(bnd, ob)
        A = oracle.assemble_operator(m, order, od, ond, -oracle.laplacian())
        rp, ci = ctx.pattern_get()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colidx)
        ctx.close()


def test_boundary_mask_override(capi, oracle):
    """fdapde_dofs_set_boundary replaces basis_.boundary_dofs() (used by element-partitioned ranks and for Dirichlet data on
    part of the boundary); host-only contexts accept it too"""
    m = oracle.load_mesh(os.path.join(os.path.dirname(__file__), "golden", "mesh", "unit_square_16"))
    ctx = capi.Context(device=None)
    ctx.mesh_upload(m.nodes, m.cells, m.boundary)
    nd = ctx.dofs_build(2)
    _, bnd, coords = ctx.dofs_get()
    new = (bnd.astype(bool) & (coords[:, 0] < 0.5)).astype(np.uint8)      # Dirichlet on the left half of the boundary only
    ctx.dofs_set_boundary(new)
    _, got, _ = ctx.dofs_get()
    assert np.array_equal(got, new) and got.sum() < bnd.sum()
    with pytest.raises(AssertionError):
        ctx.dofs_set_boundary(new[:-1])
    ctx.close()


@pytest.mark.parametrize("dim,nx", [(3, 22), (2, 150)])
def test_order2_numbering_at_multithreaded_sizes(capi, oracle, dim, nx):
    """The set-up enumerates edges with all host threads once a mesh has a few 10^4 cells (buckets by the smaller node, relaxed
    atomic scatter, per-bucket sorts); DOF table, boundary DOFs and DOF coordinates must still equal the reference's serial
    first-seen enumeration (lagrangian_basis.h:105-133, triangulation.h:150-193,348-377) bit for bit."""
    from fdapde_core_amd import meshgen

    nodes, cells, bnd = meshgen.unit_cube(nx) if dim == 3 else meshgen.unit_square(nx)
    m = oracle.Mesh(nodes, cells, bnd)
    dofs, b, nd, _ = oracle.enumerate_dofs(m, 2)
    coords = oracle.dofs_coords(m, 2, dofs, nd)
    c = capi.Context(device=None)
    c.mesh_upload(nodes, cells, bnd)
    assert c.dofs_build(2) == nd
    d2, b2, co2 = c.dofs_get()
    assert np.array_equal(d2, dofs)
    assert np.array_equal(np.asarray(b2).astype(bool), np.asarray(b).astype(bool))
    assert np.array_equal(co2, coords)
    rp, ci = c.pattern_get()
    A = oracle.assemble_operator(m, 2, dofs, nd, oracle.reaction(1.0))
    assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colidx)


def test_committed_counter_passes_name_their_workload():
    """bench.py quotes roofline.traffic from profiles/spmv_pmc.json only for the workload the passes were collected on: the file must say which
    (nx, iterations of the single launch) -- a summary copied over without these keys silently turns `traffic` into null"""
    import json
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pj = json.load(open(os.path.join(root, "profiles", "spmv_pmc.json")))
    assert pj.get("nx") == 119 and int(pj.get("persist_iterations", 0)) > 0
    assert pj.get("persist_hbm_bytes_per_solve", 0) > 0 and pj.get("hbm_bytes_per_launch", 0) > 0
    c5 = json.load(open(os.path.join(root, "profiles", "r3_c5_spmv_pmc.json")))
    assert c5.get("hbm_bytes_per_launch", 0) > 0


def test_multi_gpu_acceptance_predictions_are_monotone():
    """dist.predict_c3: the row-distributed form must be predicted faster with more GPUs and faster than the element-partitioned
    exchange at every N; the "wrong above" threshold sits at twice the prediction"""
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import dist

    last = None
    for world in (2, 4, 8):
        r, p = dist.predict_c3(world, "rowdist"), dist.predict_c3(world, "peers")
        assert r["us_per_iteration"] < p["us_per_iteration"] and r["dof_per_s"] > p["dof_per_s"]
        assert abs(r["wrong_above_us"] - 2 * r["us_per_iteration"]) < 0.11
        assert r["rows_per_rank"] == 1643032 // world
        if last is not None:
            assert r["us_per_iteration"] < last["us_per_iteration"] and r["dof_per_s"] > last["dof_per_s"]
        last = r
    assert 100e6 < dist.predict_c3(2, "rowdist")["dof_per_s"] < 400e6


def test_parity_check_fails_the_bench_when_a_bar_is_missed():
    """the comparison itself: a perturbed entry / a different pattern must be reported as not ok"""
    import numpy as np

    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import bench
    from oracle import oracle as o

    m = o.load_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16"))
    dofs, bnd, nd, _ = o.enumerate_dofs(m, 1)
    A = o.assemble_operator(m, 1, dofs, nd, -o.laplacian())
    Mm = o.assemble_operator(m, 1, dofs, nd, o.reaction(1.0))
    rhs = o.assemble_forcing(m, 1, dofs, nd, np.ones(3 * m.n_cells))
    u = np.linspace(1.0, 2.0, nd)
    gpu = {"u": u.copy(), "rowptr": A.rowptr.copy(), "colidx": A.colidx.copy(), "dofs": dofs.copy(), "boundary": bnd.copy(), "stiff": A.values.copy(),
           "mass": Mm.values.copy(), "force": rhs.copy()}
    assert bench.parity_against_oracle(gpu, dofs, bnd, A, Mm, rhs, u, "self")["ok"] is True
    bad = dict(gpu, stiff=gpu["stiff"].copy())
    bad["stiff"][7] += 1e-9
    assert bench.parity_against_oracle(bad, dofs, bnd, A, Mm, rhs, u, "self")["ok"] is False
    bad = dict(gpu, colidx=gpu["colidx"].copy())
    bad["colidx"][3] += 1
    r = bench.parity_against_oracle(bad, dofs, bnd, A, Mm, rhs, u, "self")
    assert r["ok"] is False and r["pattern_equal"] is False
    bad = dict(gpu, u=u * (1 + 1e-6))
    assert bench.parity_against_oracle(bad, dofs, bnd, A, Mm, rhs, u, "self")["ok"] is False


def test_bench_output_dump_is_float64_and_a_fixed_sample_of_large_outputs(tmp_path):
    """bench.py --dump-outputs: outputs up to DUMP_MAX_ENTRIES are written whole, longer ones as the same seeded sample every time"""
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import bench

    small = np.arange(10, dtype=np.float32)
    big = np.random.default_rng(0).standard_normal(bench.DUMP_MAX_ENTRIES + 1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    s, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)
    assert b.dtype == np.float64 and b.size == bench.DUMP_MAX_ENTRIES and np.isin(b, big).all()
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    assert 4 * 8 * bench.DUMP_MAX_ENTRIES <= 64e6   # the four outputs of a step stay under 64 MB


def test_bench_refuses_zero_steps():
    import subprocess
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
