"""Assembly, basis evaluation and point location OFF the unit box, against the multiprecision reference tests/mp_ref.py.

Every other numerical test compares a kernel with a float64 checker under |delta| <= 1e-12 max(1, ||A||max) on meshes of O(1) coordinates and
well-shaped cells.  Here the meshes are affine images of small generated ones -- mp_ref.CASES, 42 cases x orders 1 and 2:

    kind  base mesh                         scale          shift           stretch of axis 0        rotated after the stretch
    (1,1) interval(24)                      1e-6, 1, 1e6   0, 1e6 scale    1, 1e3, 1e6              --
    (1,2) street_grid(3, 3)                 1e-6, 1, 1e6   0, 1e6 scale    1, 1e3, 1e6              always (0.5 rad); + scale 100, shift (5e5, 4.5e6)
    (2,2) unit_square(4)                    1e-6, 1, 1e6   0, 1e6 scale    1, 1e3, 1e6              every stretched case (0.5 rad)
    (2,3) sphere level 1, height field(4)   1e-6, 1, 1e6   0, 1e6 scale    1, 30, 1e3               always (meshgen.rotation(4))
    (3,3) unit_cube(2)                      1e-6, 1, 1e6   0, 1e6 scale    1, 30, 1e3               every stretched case
          + the cube with a cap, a needle and a sliver glued on (volume / h^3 ~ 1e-9), unmoved and shifted + rotated

(not the full product: every value of every axis, and the corners largest stretch x shift x both extreme scales) -- and the bound is relative
to what was added up, per entry, with no floor:

    |A_gpu - A_mp|_ij <= c u S^(p)_ij,   S_ij = sum_{cells e holding i, j} sum_{terms t} ||K_{e,t}||max   (force: sum_e max_h |f_{e,h}|),

u = 2^-53, every cell's share weighted by kappa_2(J)^p (mp_ref.growth_powers): p = 0 on segments; on triangles in the plane and on tetrahedra p = 1 for
every term (the determinant of a stretched-then-rotated cell cancels, so the measure -- and with it mass, force, lumped mass, cell integrals -- is
only good to u kappa, and the adjugate inverse loses no more than that); on surfaces p = 2 for the terms with a J+ = (J^T J)^{-1} J^T and 1 for the
rest.  This is the growth of the reference's own float64 formulas as measured on the CPU checkers, not what was first
expected: the measure needs kappa where p = 0 was expected, tetrahedra need kappa where kappa^2 was allowed.  quadrature_nodes: <= c u max|x| of
the cell's vertices.  c is NOT tuned on the kernels: it is 4 r_cpu rounded up to a power of
two, r_cpu the worst ratio of the float64 CPU checkers on the same case list (tests/test_mp_ref_cpu.py measures it and fails if BOUNDS is
stale); the 4 covers another summation order and FMA contraction.

Operators: -laplacian, mass, diffusion(K) + advection(b) + reaction(c) with a non-symmetric K, the same without advection (the reference's mirrored
form), one expression of per-quadrature-node K, b, c fields, forcing; through fdapde_init and through fdapde_assemble_operator in every scatter
variant the mesh kind has.  On the same meshes: DOF table, boundary DOFs and pattern bit-exact, device set-up = host set-up (FDAPDE_SETUP_CHECK),
Psi rows and point location (not on surfaces: refused by design), and one dense-direct solve per mesh kind at scale 1e-6 and 1e6."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import mp_ref as mr
import segment_ref as sg
import surface_ref as sr

pytestmark = pytest.mark.gpu

CLASSES = ("stiff", "mass", "force", "lumped", "cell", "qnodes", "psi")
# (mesh kind, order, class) -> (r_cpu, c): r_cpu measured by tests/test_mp_ref_cpu.py on the float64 CPU checkers, c = 4 r_cpu rounded up to 2^k
BOUNDS = {
    ('11', 1, 'cell'): (1.76, 8), ('11', 1, 'force'): (1.98, 8), ('11', 1, 'lumped'): (1.62, 8), ('11', 1, 'mass'): (1.43, 8), ('11', 1, 'psi'): (0.1, 1), ('11', 1, 'qnodes'): (0.98, 4), ('11', 1, 'stiff'): (3.47, 16),
    ('11', 2, 'cell'): (1.64, 8), ('11', 2, 'force'): (3.3, 16), ('11', 2, 'lumped'): (0.92, 4), ('11', 2, 'mass'): (1.48, 8), ('11', 2, 'psi'): (0.35, 2), ('11', 2, 'qnodes'): (1, 4), ('11', 2, 'stiff'): (4.12, 32),
    ('12', 1, 'cell'): (3.18, 16), ('12', 1, 'force'): (3.05, 16), ('12', 1, 'lumped'): (2.25, 16), ('12', 1, 'mass'): (1.97, 8), ('12', 1, 'psi'): (0.35, 2), ('12', 1, 'qnodes'): (1, 4), ('12', 1, 'stiff'): (5.41, 32),
    ('12', 2, 'cell'): (2.68, 16), ('12', 2, 'force'): (3.59, 16), ('12', 2, 'lumped'): (1.08, 8), ('12', 2, 'mass'): (2.33, 16), ('12', 2, 'psi'): (1.39, 8), ('12', 2, 'qnodes'): (1.36, 8), ('12', 2, 'stiff'): (5.63, 32),
    ('22', 1, 'cell'): (2.21, 16), ('22', 1, 'force'): (0.6, 4), ('22', 1, 'lumped'): (0.9, 4), ('22', 1, 'mass'): (2.06, 16), ('22', 1, 'psi'): (0.11, 1), ('22', 1, 'qnodes'): (1, 4), ('22', 1, 'stiff'): (3.26, 16),
    ('22', 2, 'cell'): (1.59, 8), ('22', 2, 'force'): (1.81, 8), ('22', 2, 'lumped'): (0.81, 4), ('22', 2, 'mass'): (1.87, 8), ('22', 2, 'psi'): (0.43, 2), ('22', 2, 'qnodes'): (1.33, 8), ('22', 2, 'stiff'): (3.09, 16),
    ('23', 1, 'cell'): (2.34, 16), ('23', 1, 'force'): (0.95, 4), ('23', 1, 'lumped'): (1.49, 8), ('23', 1, 'mass'): (2.14, 16), ('23', 1, 'qnodes'): (1.42, 8), ('23', 1, 'stiff'): (2.32, 16),
    ('23', 2, 'cell'): (1.92, 8), ('23', 2, 'force'): (1.94, 8), ('23', 2, 'lumped'): (0.79, 4), ('23', 2, 'mass'): (2.08, 16), ('23', 2, 'qnodes'): (1.11, 8), ('23', 2, 'stiff'): (2.46, 16),
    ('33', 1, 'cell'): (4.7, 32), ('33', 1, 'force'): (2.34, 16), ('33', 1, 'lumped'): (1.75, 8), ('33', 1, 'mass'): (2.8, 16), ('33', 1, 'psi'): (2.64, 16), ('33', 1, 'qnodes'): (1.46, 8), ('33', 1, 'stiff'): (3.43, 16),
    ('33', 2, 'cell'): (4.7, 32), ('33', 2, 'force'): (3.85, 16), ('33', 2, 'lumped'): (1.54, 8), ('33', 2, 'mass'): (4.7, 32), ('33', 2, 'psi'): (6.09, 32), ('33', 2, 'qnodes'): (1.4, 8), ('33', 2, 'stiff'): (4.7, 32),
}


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    return capi


def _variants(capi, kind):
    rows = {"rows": capi.ASSEMBLY_ROWS}
    if kind in ("22", "33"):
        rows.update(atomic=capi.ASSEMBLY_ATOMIC, coloured=capi.ASSEMBLY_COLOURED, partitioned=capi.ASSEMBLY_PARTITIONED, wave=capi.ASSEMBLY_WAVE)
    return rows


_GPU_WORST = {}


def _check(key, what, ratio):
    """one figure against its bound; printed before it is asserted, and kept for the profile"""
    r_cpu, c = BOUNDS[key]
    print(f"{what}: {ratio:.3g} (c = {c:g}, r_cpu = {r_cpu:g})")
    _GPU_WORST[key] = max(_GPU_WORST.get(key, 0.0), ratio)
    path = os.environ.get("FDAPDE_ROBUSTNESS_PROFILE_GPU")
    if path:
        with open(path, "a") as f:
            f.write(f"{key[0]} {key[1]} {key[2]} {ratio:.6g} {what}\n")
    assert ratio <= c, (what, ratio, c)


def _cell_integrals(capi, c):
    import ctypes as C

    s = c.sizes()
    meas, pint = np.zeros(c.n_cells), np.zeros((c.n_cells, s["n_basis"]))
    c._check(c.lib.fdapde_cell_integrals(c._ctx, meas.ctypes.data_as(C.POINTER(C.c_double)), pint.ctypes.data_as(C.POINTER(C.c_double))))
    return meas, pint


# ---- assembly --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", mr.ORDERS)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_assembly_against_the_multiprecision_reference(env, case, order, monkeypatch):
    capi = env
    kind = case[0]
    nodes, cells, bnd, dofs, bdofs, nd, space = mr.space_of(case, order)
    monkeypatch.setenv("FDAPDE_SETUP_CHECK", "1")   # device set-up = host set-up, array for array (a mismatch fails fdapde_dofs_build)
    c = capi.Context(device=0)
    c.mesh_upload(nodes, cells, bnd)
    assert c.dofs_build(order) == nd
    monkeypatch.delenv("FDAPDE_SETUP_CHECK")
    gd, gb, coords = c.dofs_get()
    assert np.array_equal(gd, dofs) and np.array_equal(gb, bdofs)
    rp, ci = c.pattern_get()
    assert np.array_equal(rp, space.rowptr) and np.array_equal(ci, space.colidx)
    # order-2 DOF coordinates: the midpoints the device computed from THESE coordinates, against the float64 checkers' formula
    if kind in ("11", "12"):
        ref_coords = sg.dof_coords(nodes, cells, order)
    elif kind == "23":
        ref_coords = sr.dof_coords(nodes, cells, dofs, nd, order)
    else:
        from oracle import oracle as o

        ref_coords = o.dofs_coords(o.Mesh(nodes, cells, bnd), order, dofs, nd)
    assert np.abs(coords - ref_coords).max() <= 4 * mr.U * np.abs(nodes).max()
    rows = len(cells) * space.nq
    ops = mr.operators(capi, nodes.shape[1], rows)
    fq = mr.forcing_samples(rows)
    force_ref, mass_ref = space.forcing(fq), space.assemble(ops["mass"])
    lumped_ref = space.lumped(mass_ref)
    tag = f"{mr.case_id(case)} P{order}"
    for name, op in ops.items():
        ref = space.assemble(op)
        cls = "mass" if name == "mass" else "stiff"
        c.set_operator(op)
        c.set_forcing(fq)
        c.init()
        _check((kind, order, cls), f"{tag} init {name}", ref.ratio(c.matrix_values(capi.MAT_STIFF)))
        _check((kind, order, "mass"), f"{tag} init {name}: mass", mass_ref.ratio(c.matrix_values(capi.MAT_MASS)))
        _check((kind, order, "force"), f"{tag} init {name}: force", force_ref.ratio(c.force()))
        _check((kind, order, "lumped"), f"{tag} init {name}: lumped mass", lumped_ref.ratio(c.lump(capi.MAT_MASS)))
        for vname, v in _variants(capi, kind).items():
            c.assemble_operator(capi.MAT_STIFF, op, v)
            _check((kind, order, cls), f"{tag} assemble_operator[{vname}] {name}", ref.ratio(c.matrix_values(capi.MAT_STIFF)))
    for vname, v in _variants(capi, kind).items():
        if vname != "rows":   # fdapde_init in the other scatter variants (stiffness, mass and force in one call)
            c.set_operator(ops["nonsym_adv"])
            c.set_forcing(fq)
            c.init(v)
            _check((kind, order, "stiff"), f"{tag} init[{vname}] nonsym_adv",
                   space.assemble(ops["nonsym_adv"]).ratio(c.matrix_values(capi.MAT_STIFF)))
            _check((kind, order, "mass"), f"{tag} init[{vname}]: mass", mass_ref.ratio(c.matrix_values(capi.MAT_MASS)))
            _check((kind, order, "force"), f"{tag} init[{vname}]: force", force_ref.ratio(c.force()))
    meas, pint = _cell_integrals(capi, c)
    mm, ci_ref = space.measures(), space.cell_integrals()
    w = space.measure_weights()
    _check((kind, order, "cell"), f"{tag} cell measures", mr.ratio_plain(meas, mm, w * [float(v) for v in mm]))
    _check((kind, order, "cell"), f"{tag} cell integrals of the basis",
           mr.ratio_plain(pint, [v for row in ci_ref for v in row], np.repeat(w * [float(max(abs(v) for v in row)) for row in ci_ref], space.nb)))
    xmax = np.repeat([cell.xmax for cell in space.cells], space.nq * space.N)
    _check((kind, order, "qnodes"), f"{tag} quadrature nodes",
           mr.ratio_plain(c.quadrature_nodes(), [v for row in space.quadrature_nodes() for v in row], xmax))
    c.close()


# ---- Psi rows and point location -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", mr.ORDERS)
@pytest.mark.parametrize("case", [c for c in mr.CASES if mr.is_location_case(c)], ids=mr.case_id)
def test_point_location_and_psi_rows_off_the_unit_box(env, case, order):
    """rho = 4 u max|coordinate| ||J+||_inf is what the float64 rounding of a location is worth in barycentric units.  Every constructed inside / on
    point is located, in a cell of mp_ref's C(1e-12 + rho); on segments the lowest reference id wins wherever the candidates are unambiguous
    (C(1e-12 + 2 rho) = C(1e-12 + rho / 2): the kernel's own evaluation error is below rho / 4, a constructed point is off its cell by at most rho / 4);
    every point outside by 1e-3 gets -1; the global Psi row equals mp_ref's basis values within c (u kappa_2(J) + rho), and sums to 1 within the same"""
    capi = env
    kind = case[0]
    nodes, cells, bnd, dofs, _, nd, space = mr.space_of(case, order)
    pts, home, outside = mr.location_points(space)
    c = capi.Context(device=0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(order)
    psi, _, found = c.eval_pointwise(np.vstack([pts, outside]))
    c.close()
    n = len(pts)
    missed = np.nonzero(found[:n] < 0)[0]
    print(f"{mr.case_id(case)} P{order}: {n - missed.size} of {n} inside / on points located, {int((found[n:] >= 0).sum())} of {len(outside)} outside points located")
    assert missed.size == 0, (missed[:10], pts[missed[:10]])
    assert np.all(found[n:] == -1) and psi[n:].nnz == 0
    psi = psi.tocsr()
    worst = 0.0
    for i, p in enumerate(pts):
        e = int(found[i])
        cand = space.candidates(p)
        assert e in cand, (i, p, e, cand)
        if space.M == 1:
            wide, sure = space.candidates(p, k=2.0), space.candidates(p, k=0.5)
            if wide == sure:
                assert e == min(sure), (i, p, e, sure)
        d, vals, _ = space.psi_row(e, p)
        row = psi[i].toarray().ravel()
        tol = mr.U * space.cells[e].kappa + space.rho(e, p)
        expect = np.zeros(nd)
        err = 0.0
        for dof, v in zip(d, vals):
            err = max(err, abs(row[dof] - float(v)))
            expect[dof] = 1.0
        assert np.all(row[expect == 0.0] == 0.0)
        worst = max(worst, err / tol, abs(row.sum() - 1.0) / tol)
    _check((kind, order, "psi"), f"{mr.case_id(case)} P{order} Psi rows", worst)


# ---- one dense-direct solve per mesh kind in millimetres and in kilometres ---------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-6, 1e6])
@pytest.mark.parametrize("kind,mesh,rot", [("11", "interval", False), ("12", "streets", True), ("22", "square", True), ("23", "sphere", True),
                                           ("33", "cube", True)])
def test_dense_solve_at_extreme_scales(env, kind, mesh, rot, scale):
    """-laplacian + reaction(1 / scale^2) = f with Dirichlet data, order 2, through FDAPDE_SOLVER_DENSE (its row equilibration and the residual gates
    max |I - A X| < 1e-6 / 1e-13, with unit Dirichlet rows next to stiffness rows of 1e-10 ... 1e+8) against scipy's LU of mp_ref's matrix rounded
    to float64: <= 1e-8 relative.  Before the rows were equilibrated the interval at scale 1e-6 was refused as singular (max |I - A X| = 3.7e-6)."""
    capi = env
    case = (kind, mesh, scale, True, 1.0, rot)
    assert case in mr.CASES
    nodes, cells, bnd, dofs, bdofs, nd, space = mr.space_of(case, 2)
    assert nd <= 1000
    rows = len(cells) * space.nq
    k2 = 1.0 / scale ** 2
    fq = k2 * (1.0 + np.sin(np.arange(rows) * 0.37))
    ref_x = (np.array([[float(v) for v in row] for row in space.quadrature_nodes()]).mean(axis=0))   # a point of the mesh
    c = capi.Context(device=0)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(2)
    _, _, coords = c.dofs_get()
    g = 1.0 + ((coords - ref_x) / scale)[:, 0] * 0.5
    mk = lambda mod: -mod.laplacian() + mod.reaction(k2)
    c.set_operator(mk(capi))
    c.set_forcing(fq)
    c.set_dirichlet(g)
    c.init()
    info = c.solve(method=capi.SOLVER_DENSE)
    assert info.converged == 1 and info.method_used == capi.SOLVER_DENSE
    u = c.solution()
    c.close()
    A = sp.csr_matrix((space.assemble(mk(capi)).rounded(), space.colidx, space.rowptr), shape=(nd, nd))
    A, b = sr.set_dirichlet(A, space.forcing(fq).rounded(), bdofs, g)
    ref = spla.splu(A.tocsc()).solve(b)
    err = np.abs(u - ref).max() / np.abs(ref).max()
    print(f"{mr.case_id(case)}: dense solve vs LU of the multiprecision matrix {err:.3g}; entries {np.abs(A.data[A.data != 0]).min():.3g} .. {np.abs(A.data).max():.3g}")
    assert err <= 1e-8
