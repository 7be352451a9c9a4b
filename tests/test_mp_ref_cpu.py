"""The multiprecision reference (tests/mp_ref.py) pinned, and the float64 checkers measured against it -- CPU only.

  1. closed forms in exact rationals (fractions.Fraction): P1 mass |e| / 12 (1 + delta_ij) of a triangle, |e| / 20 (1 + delta_ij) of a tetrahedron, h / 6
     [[2, 1], [1, 2]] of a segment; P1 stiffness of the right triangle and of the unit segment.  mp_ref, with the quadrature constants in 50 digits,
     equals them to 1e-45.
  2. on well-shaped fixtures (<= 120 cells of unit_square_16, surface, network, unit_sphere) mp_ref and the float64 checker of each mesh kind
     (the C oracle, surface_ref, segment_ref) agree within the bounds of tests/test_gpu_geometry_robustness.py -- which pins mp_ref to
     checkers that the reference's golden vectors pin.
  3. the whole case list of mp_ref.CASES through the float64 checkers: the worst |delta| / (u S^(p)) per (mesh kind, order, class) is r_cpu.  The
     constants c of the GPU bounds are 4 r_cpu rounded up to a power of two (the 4 covers another summation order and FMA contraction, which change
     the constant and not the growth); they stand in test_gpu_geometry_robustness.BOUNDS next to the r_cpu they came from, and this file
     fails if a measured r_cpu no longer fits its c / 4, or exceeds 64 (then p, the reference or the scale is wrong, not the constant).
     FDAPDE_ROBUSTNESS_PROFILE=<path> writes the table (profiles/geometry_robustness.txt is such a run).
  4. rho = 4 u max|coordinate| ||J+||_inf <= 1e-6 on every point-location case, so that "outside by 1e-3" cannot be mistaken for rounding.

Takes about two minutes (the multiprecision assembly of ~80 small meshes)."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import mp_ref as mr
import segment_ref as sg
import surface_ref as sr
import test_gpu_geometry_robustness as G
from mp_ref import mpf
from oracle import oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. closed forms ----------------------------------------------------------------------------------------------------------------------
def _exact_space(nodes, cells):
    nodes = np.asarray(nodes, float)
    cells = np.asarray(cells, np.int32)
    return mr.Space(nodes, cells, cells, nodes.shape[0], 1, exact=True)


def _assert_equals(K, expect):
    for i, row in enumerate(expect):
        for j, v in enumerate(row):
            assert abs(K[i][j] - mr.M_(v)) <= mpf(10) ** -45 * max(1, abs(mr.M_(v))), (i, j, K[i][j], v)


def test_closed_form_triangle():
    x = [[Fraction(1, 4), Fraction(1, 8)], [Fraction(3, 2), Fraction(1, 2)], [Fraction(3, 8), Fraction(7, 4)]]   # dyadic: exact in float64
    area = abs((x[1][0] - x[0][0]) * (x[2][1] - x[0][1]) - (x[2][0] - x[0][0]) * (x[1][1] - x[0][1])) / 2
    s = _exact_space([[float(v) for v in p] for p in x], [[0, 1, 2]])
    assert abs(s.cells[0].measure - mr.M_(area)) <= mpf(10) ** -45
    _assert_equals(s.term_matrices(mr.REACTION, [1.0], None)[0], [[area / 12 * (2 if i == j else 1) for j in range(3)] for i in range(3)])
    r = _exact_space([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], [[0, 1, 2]])
    h = Fraction(1, 2)
    _assert_equals(r.term_matrices(mr.LAPLACIAN, None, None)[0], [[-2 * h, h, h], [h, -h, 0], [h, 0, -h]])   # laplacian() is -(grad, grad)
    # the same triangle as a surface cell in the plane z = 3: the pseudo-inverse branch gives the same matrices
    s3 = _exact_space([[float(v) for v in p] + [3.0] for p in x], [[0, 1, 2]])
    _assert_equals(s3.term_matrices(mr.REACTION, [1.0], None)[0], [[area / 12 * (2 if i == j else 1) for j in range(3)] for i in range(3)])
    K2, K3 = s.term_matrices(mr.LAPLACIAN, None, None)[0], s3.term_matrices(mr.LAPLACIAN, None, None)[0]
    assert max(abs(K2[i][j] - K3[i][j]) for i in range(3) for j in range(3)) <= mpf(10) ** -45


def test_closed_form_segment():
    for nodes, h in (([[0.0], [1.0]], Fraction(1)), ([[0.25], [2.0]], Fraction(7, 4)), ([[1.0, 2.0], [4.0, 6.0]], Fraction(5))):
        s = _exact_space(nodes, [[0, 1]])
        _assert_equals(s.term_matrices(mr.LAPLACIAN, None, None)[0], [[-1 / h, 1 / h], [1 / h, -1 / h]])
        _assert_equals(s.term_matrices(mr.REACTION, [1.0], None)[0], [[h / 3, h / 6], [h / 6, h / 3]])


def test_closed_form_tetrahedron():
    x = [[Fraction(0), Fraction(1, 4), Fraction(1, 2)], [Fraction(2), Fraction(1, 2), Fraction(1, 8)], [Fraction(1, 4), Fraction(3), Fraction(0)],
         [Fraction(1, 2), Fraction(1), Fraction(5, 2)]]
    J = [[x[k + 1][d] - x[0][d] for k in range(3)] for d in range(3)]
    det = (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])
           + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))
    vol = abs(det) / 6
    s = _exact_space([[float(v) for v in p] for p in x], [[0, 1, 2, 3]])
    assert abs(s.cells[0].measure - mr.M_(vol)) <= mpf(10) ** -45
    _assert_equals(s.term_matrices(mr.REACTION, [1.0], None)[0], [[vol / 20 * (2 if i == j else 1) for j in range(4)] for i in range(4)])
    # row sums of the stiffness vanish, and the unit tetrahedron's is the textbook one
    r = _exact_space([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], [[0, 1, 2, 3]])
    s6 = Fraction(1, 6)
    _assert_equals(r.term_matrices(mr.LAPLACIAN, None, None)[0], [[-3 * s6, s6, s6, s6], [s6, -s6, 0, 0], [s6, 0, -s6, 0], [s6, 0, 0, -s6]])


def test_float64_tables_are_the_exact_ones_to_their_printed_digits():
    """the checkers' tables are the reference's 15-digit constants: within 1e-15 of the exact rule, in the same node order"""
    for M in (1, 2, 3):
        qn, qw, psi, dpsi = mr.tables(M, 1)
        en, ew, epsi, _ = mr.exact_tables(M)
        for q in range(len(qw)):
            assert abs(qw[q] - ew[q]) <= 1e-15 and all(abs(qn[q][k] - en[q][k]) <= 1e-15 for k in range(M))
            assert all(abs(psi[i][q] - epsi[i][q]) <= 2e-15 for i in range(M + 1))


def test_basis_is_a_partition_of_unity_and_nodal():
    for M in (1, 2, 3):
        for order in (1, 2):
            nodes = mr.reference_nodes(M, order)
            for a, n in enumerate(nodes):
                v = mr.basis_at(M, order, [mr.M_(t) for t in n])
                assert all(abs(v[b] - (1 if a == b else 0)) <= mpf(10) ** -45 for b in range(len(nodes)))
            lam = [mpf(1) / 7, mpf(2) / 7, mpf(3) / 7, mpf(1) / 7][: M + 1]
            lam[0] += 1 - sum(lam)
            assert abs(sum(mr.basis_at(M, order, lam)) - 1) <= mpf(10) ** -45


# ---- the float64 checkers behind one interface -----------------------------------------------------------------------------------------------
def checker_results(kind, nodes, cells, bnd, dofs, nd, order, space):
    """every quantity of the GPU test through the float64 CPU checker of the mesh kind -> dict class -> (name -> float64 array in mp_ref's order)"""
    rows = len(cells) * space.nq
    ops = mr.operators(o, nodes.shape[1], rows)
    fq = mr.forcing_samples(rows)
    out = {}
    if kind in ("11", "12"):
        mats = {n: sg.values_in_pattern(sg.assemble(nodes, cells, dofs, nd, order, op), space.rowptr, space.colidx) for n, op in ops.items()}
        force = sg.forcing(nodes, cells, dofs, nd, order, fq)
        qn = sg.quadrature_nodes(nodes, cells, order)
        meas = sg.geometry(nodes, cells)[2]
        qw, psi = sg.tables(order)[1:3]
    elif kind == "23":
        mats = {n: sr.values_in_pattern(sr.assemble(nodes, cells, dofs, nd, order, op), space.rowptr, space.colidx) for n, op in ops.items()}
        force = sr.forcing(nodes, cells, dofs, nd, order, fq)
        qn = sr.quadrature_nodes(nodes, cells, order)
        meas = sr.geometry(nodes, cells)[2]
        qw, psi = sr.tables(order)[1:3]
    else:
        m = o.Mesh(np.ascontiguousarray(nodes), np.ascontiguousarray(cells, np.int32), np.ascontiguousarray(bnd, np.uint8))
        mats = {}
        for n, op in ops.items():
            A = o.assemble_operator(m, order, dofs, nd, op)
            assert np.array_equal(A.rowptr, space.rowptr) and np.array_equal(A.colidx, space.colidx)
            mats[n] = A.values
        force = o.assemble_forcing(m, order, dofs, nd, fq)
        qn = o.quadrature_nodes(m, order)
        meas = np.array([o.cell_geometry(m, e)[2] for e in range(len(cells))])
        qw = o.quadrature(m.M, order)[1]
        psi = o.basis_tables(m.M, order)[0]
    out["mats"] = mats
    out["force"] = force
    out["lumped"] = np.asarray(sp.csr_matrix((mats["mass"], space.colidx, space.rowptr), shape=(nd, nd)).sum(axis=1)).ravel()
    out["qnodes"] = qn
    out["measure"] = meas
    out["psi_int"] = meas[:, None] * (psi @ qw)[None, :]
    return out


def ratios(kind, space, res):
    """-> dict class -> worst |delta| / (u S^(p)) of one (case, order)"""
    N, rows = space.N, len(space.cells) * space.nq
    ops = mr.operators(o, N, rows)
    r = {}
    mass = None
    for n, op in ops.items():
        A = space.assemble(op)
        v = A.ratio(res["mats"][n])
        cls = "mass" if n == "mass" else "stiff"
        r[cls] = max(r.get(cls, 0.0), v)
        r["op:" + n] = v
        if n == "mass":
            mass = A
    r["force"] = space.forcing(mr.forcing_samples(rows)).ratio(res["force"])
    r["lumped"] = space.lumped(mass).ratio(res["lumped"])
    meas = space.measures()
    ci = space.cell_integrals()
    w = space.measure_weights()
    r["cell"] = max(mr.ratio_plain(res["measure"], meas, w * [float(v) for v in meas]),
                    mr.ratio_plain(res["psi_int"], [v for row in ci for v in row],
                                   np.repeat(w * [float(max(abs(v) for v in row)) for row in ci], space.nb)))
    xmax = np.repeat([c.xmax for c in space.cells], space.nq * N)
    r["qnodes"] = mr.ratio_plain(res["qnodes"], [v for row in space.quadrature_nodes() for v in row], xmax)
    return r


def psi_ratio_float64(space):
    """the float64 evaluation of a Psi row (J+ of the mesh kind's float64 checker -- the oracle's cofactor inverse, segment_ref's J / |J|^2 --,
    barycentric coordinates, basis) in the home cell of every constructed location, against mp_ref: worst |delta| / (u kappa + rho)"""
    pts, home, _ = mr.location_points(space)
    worst = 0.0
    if space.M == 1:
        invJ = sg.geometry(space.nodes, space.cells_idx)[1][:, None, :]
    else:
        m = o.Mesh(space.nodes, np.ascontiguousarray(space.cells_idx, np.int32), np.zeros(len(space.nodes), np.uint8))
        invJ = {e: o.cell_geometry(m, e)[1] for e in set(home.tolist())}
    for p, e in zip(pts, home.tolist()):
        x = space.nodes[space.cells_idx[e]]
        xi = invJ[e] @ (p - x[0])
        lam = np.concatenate([[1.0 - xi.sum()], xi])
        got = [float(v) for v in mr.basis_at(space.M, space.order, [mpf(float(t)) for t in lam])]   # (the basis formula itself in 50 digits)
        _, ref, _ = space.psi_row(e, p)
        tol = mr.U * space.cells[e].kappa + space.rho(e, p)
        worst = max(worst, max(abs(g - float(r)) for g, r in zip(got, ref)) / tol)
    return worst


# ---- 2. mp_ref against the checkers on the well-shaped fixtures --------------------------------------------------------------------------
def _sub(nodes, cells, bnd, n=120):
    """the first n cells of a mesh with the nodes they use"""
    cells = np.asarray(cells)[:n]
    used = np.unique(cells)
    new = -np.ones(len(nodes), np.int64)
    new[used] = np.arange(used.size)
    nodes = np.asarray(nodes, float).reshape(len(nodes), -1)
    return np.ascontiguousarray(nodes[used]), np.ascontiguousarray(new[cells].astype(np.int32)), np.ascontiguousarray(np.asarray(bnd, np.uint8)[used])


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("fixture", ["unit_square_16", "surface", "network", "unit_sphere"])
def test_mp_ref_agrees_with_the_float64_checkers_on_the_fixtures(fixture, order):
    o.build()
    m = o.load_mesh(os.path.join(ROOT, "tests", "golden", "mesh", fixture))
    nodes, cells, bnd = _sub(m.nodes, m.cells, m.boundary)
    kind = f"{cells.shape[1] - 1}{nodes.shape[1]}"
    dofs, _, nd = mr.enumerate_dofs(nodes, cells, bnd, order)
    space = mr.Space(nodes, cells, dofs, nd, order)
    r = ratios(kind, space, checker_results(kind, nodes, cells, bnd, dofs, nd, order, space))
    for cls in G.CLASSES:
        if cls != "psi":
            assert r[cls] <= G.BOUNDS[(kind, order, cls)][1], (fixture, order, cls, r[cls])


# ---- 3. r_cpu on the whole case list ---------------------------------------------------------------------------------------------------------
_R = {}


def _case_ratios(case, order):
    if (case, order) not in _R:
        nodes, cells, bnd, dofs, _, nd, space = mr.space_of(case, order)
        r = ratios(case[0], space, checker_results(case[0], nodes, cells, bnd, dofs, nd, order, space))
        if mr.is_location_case(case):
            r["psi"] = psi_ratio_float64(space)
        _R[(case, order)] = r
    return _R[(case, order)]


@pytest.mark.parametrize("order", mr.ORDERS)
@pytest.mark.parametrize("case", mr.CASES, ids=mr.case_id)
def test_float64_checkers_meet_the_bounds_with_a_factor_four_to_spare(case, order):
    r = _case_ratios(case, order)
    print(mr.case_id(case), order, {k: f"{v:.3g}" for k, v in r.items()})
    for cls in G.CLASSES:
        if cls in r:
            r_cpu, c = G.BOUNDS[(case[0], order, cls)]
            assert r[cls] <= 64.0, (cls, r[cls], "p, the reference or the scale is wrong")
            assert 4.0 * r[cls] <= c, (cls, r[cls], c)


def test_bounds_table_is_four_r_cpu_rounded_up_and_profile():
    """every (kind, order, class): c = 4 r_cpu rounded up to a power of two, r_cpu the worst ratio over the case list (recomputed here)"""
    worst, worst_op = {}, {}
    for case in mr.CASES:
        for order in mr.ORDERS:
            for cls, v in _case_ratios(case, order).items():
                d = worst_op if cls.startswith("op:") else worst
                d[(case[0], order, cls)] = max(d.get((case[0], order, cls), 0.0), v)
    lines = ["# r_cpu: worst |delta| / (u S^(p)) of the float64 CPU checkers against tests/mp_ref.py over mp_ref.CASES; c = 4 r_cpu rounded up to 2^k",
             "# p: power of kappa_2(J) weighting a cell's share of the scale (stiff: terms with a J+ / terms with the measure only)",
             "# kind order class            p     r_cpu      c"]
    for key in sorted(worst):
        kind, order, cls = key
        c = 2.0 ** math.ceil(math.log2(max(4.0 * worst[key], 1.0)))
        pj, pm = mr.growth_powers(int(kind[0]), int(kind[1]))
        p = {"stiff": f"{pj}/{pm}", "qnodes": "-", "psi": "-"}.get(cls, str(pm))
        lines.append(f"{kind:>4} {order:>5} {cls:<16} {p:<3} {worst[key]:7.3f} {c:6.0f}")
        r_tab, c_tab = G.BOUNDS[key]
        assert c_tab == 2.0 ** math.ceil(math.log2(max(4.0 * r_tab, 1.0))), key
        assert worst[key] <= r_tab * 1.0001 and c <= c_tab, (key, worst[key], r_tab)
    lines.append("# per operator (class stiff and mass split up)")
    for key in sorted(worst_op):
        lines.append(f"{key[0]:>4} {key[1]:>5} {key[2]:<22} {worst_op[key]:7.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    path = os.environ.get("FDAPDE_ROBUSTNESS_PROFILE")
    if path:
        with open(path, "w") as f:
            f.write(text)


# ---- 4. rho on the point-location cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in mr.CASES if mr.is_location_case(c)], ids=mr.case_id)
def test_rho_is_far_below_the_outside_margin(case):
    nodes, cells, _, _, _, _, space = mr.space_of(case, 1)
    pts, home, outside = mr.location_points(space)
    rho = max(space.rho(e, p) for p, e in zip(pts, home.tolist()))
    assert rho <= 1e-6, rho
    # every constructed inside / on point has a cell in C(1e-12 + rho); no outside point has one
    assert all(len(space.candidates(p)) > 0 for p in pts)
    assert all(len(space.candidates(p)) == 0 for p in outside)
