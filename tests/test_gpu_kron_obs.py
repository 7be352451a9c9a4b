"""The factored data term of the Kronecker-sum handle (csrc/kernels_kron_obs.h, host_kron_obs.cpp, eng_kron.hip): fdapde_kron_set_obs / fdapde_kron_obs_info
against scipy -- the explicit system A + scale B^T W B with B = sp.kron(Phi, Psi) (tests/kron_obs_ref.py), SuperLU, the q x q point-block Jacobi of the full
matrix.  Psi is the oracle's: areal rows over tiles of the bounding box or quasi_circle's golden incidence matrix, pointwise rows with some locations outside
the mesh.  tests/test_kron_obs_cpu.py checks, without a device, that the reference GMRES stays under half of the iteration budget handed over here."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import block_obs_ref as bo
import block_ref as br
import kron_obs_ref as ko
import kron_ref as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
MESHES = os.path.join(ROOT, "tests", "golden", "mesh")


@pytest.fixture(scope="module")
def env():
    from fdapde_loader import load_package

    load_package()
    from fdapde_core_amd import capi, workloads
    from oracle import oracle as o

    assert capi.load().fdapde_device_count() >= 1, "no HIP device visible: the GPU tests must not fall back to anything"
    o.build()
    return capi, workloads, o


def _oracle_mesh(o, name):
    if name == "one_triangle":
        return o.Mesh(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), np.array([[0, 1, 2]], dtype=np.int32), np.ones(3, dtype=np.uint8))
    return o.load_mesh(os.path.join(MESHES, name))


_spaces = {}


def _space(env, name, order, fresh=False):
    """-> dict(c, nd, rp, ci, mesh, dofs): a context with the space built, the oracle's mesh and DOF table (the same numbering); shared unless fresh"""
    capi, _, o = env
    key = (name, order)
    if fresh or key not in _spaces:
        m = _oracle_mesh(o, name)
        c = capi.Context(0)
        c.mesh_upload(np.ascontiguousarray(m.nodes), np.ascontiguousarray(m.cells, dtype=np.int32), np.ascontiguousarray(m.boundary))
        nd = c.dofs_build(order)
        dofs, _, ond, _ = o.enumerate_dofs(m, order)
        assert ond == nd and np.array_equal(c.dofs_get()[0], dofs), "the oracle and the library number the DOFs alike"
        rp, ci = c.pattern_get()
        s = {"c": c, "nd": nd, "rp": rp, "ci": ci, "mesh": m, "dofs": dofs}
        if fresh:
            return s
        _spaces[key] = s
    return _spaces[key]


def _init(env, s):
    """R1 = stiff(-laplacian), R0 = mass from the device, once per space"""
    capi = env[0]
    if "r1" not in s:
        c = s["c"]
        c.set_operator(-capi.laplacian())
        c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
        c.init()
        s["r1"], s["r0"] = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    return s["r1"], s["r0"]


def _psi(env, s, name, order, kind):
    """kind: tiles per axis | "golden" | "all" (ONE region over all cells) | "pointwise" (c_shaped: locs.csv + points of the bounding box, some outside) |
    "single" (one row with one entry): the kinds of tests/test_gpu_block_obs.py"""
    _, workloads, o = env
    m, dofs, nd = s["mesh"], s["dofs"], s["nd"]
    if kind == "pointwise":
        locs = workloads._read_fixture_csv(os.path.join(MESHES, name, "locs.csv"), float)
        pts = np.concatenate([locs, np.random.default_rng(3).uniform(m.nodes.min(axis=0), m.nodes.max(axis=0), size=(2000, 2))])
        P = bo.pointwise_psi(o, m, order, dofs, nd, pts)
        assert (np.diff(P.indptr) == 0).any() and (np.diff(P.indptr) > 0).sum() > 1000, "locations outside the mesh give empty rows"
        return P
    if kind == "single":
        return sp.csr_matrix((np.array([0.75]), np.array([1]), np.array([0, 1])), shape=(1, nd))
    inc = np.ones((1, m.n_cells)) if kind == "all" else bo.incidence(o, m, name, kind)
    return bo.areal_psi(o, m, order, dofs, nd, inc)


def _rule(rows, nnz):
    return 2 if nnz > 16 * rows else 1


def _random_terms(rng, q, nnz):
    """K = 3 dense random T_k; the last term shares the spatial factor (the same array) of the first: two distinct factors"""
    S = [rng.standard_normal(nnz) for _ in range(2)]
    return [(rng.standard_normal((q, q)), S[0]), (rng.standard_normal((q, q)), S[1]), (rng.standard_normal((q, q)), S[0])], 2


# ---- 1. product parity ----------------------------------------------------------------------------------------------------------------------------
QC, SPH, ALL, PTS, TRI = ("quasi_circle", 1, "golden"), ("unit_sphere", 1, 2), ("unit_square_16", 1, "all"), ("c_shaped", 2, "pointwise"), ("one_triangle", 1, "single")
# (q, p, Phi given) on two kinds each, every kind at least three times; q = 64 stays on the two smallest spaces (the reference forms Phi (x) Psi), and
# unit_sphere on team widths from 4 on (its rows of up to 113 entries are longer than one stride of 256 / QP there)
PRODUCT_CASES = [(1, 1, True, TRI), (1, 1, True, QC), (2, 1, True, ALL), (2, 1, True, TRI), (3, 5, True, QC), (3, 5, True, ALL), (6, 4, False, PTS), (6, 4, False, SPH),
                 (10, 7, True, ALL), (10, 7, True, PTS), (16, 16, True, SPH), (16, 16, True, PTS), (33, 40, True, QC), (33, 40, True, SPH), (64, 64, True, ALL),
                 (64, 64, True, TRI), (4, 64, True, PTS), (4, 64, True, QC)]
_worst_product = [0.0]


@pytest.mark.parametrize("q,p,phi_given,space", PRODUCT_CASES)
def test_product_with_a_term_against_the_explicit_system(env, q, p, phi_given, space):
    """y = (sum_k T_k (x) S_k + scale B^T W B) x for K = 3 random dense T_k (two spatial factors) against the explicit system's product in np.longdouble:
    per row |y - y_ref| <= 2 k eps (|A| |x| + |scale| |B|^T |W| |B| |x|), k = the pattern part's count of tests/test_gpu_kron.py (n_S (longest row + q) + 2)
    + the row's Psi^T length + the longest Psi row contributing to it + p + q: the rounded operations on the longest path to that output -- derived, not
    measured.  Under kron_obs_form 1 and 2 (reported by fdapde_kron_obs_info) and under the rule; no weights at scale -1, and random weights with about a
    third exact zeros at scale 0.37; the same bits from a second call."""
    name, order, kind = space
    s = _space(env, name, order)
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    Psi = _psi(env, s, name, order, kind)
    n_obs = Psi.shape[0]
    rows = np.diff(Psi.indptr)
    cols = np.bincount(Psi.indices, minlength=nd)
    if name == "quasi_circle":
        assert (cols == 0).sum() > nd // 2, "most DOFs are in no region"
    team = 2
    while team < max(p, q):
        team *= 2
    if name == "unit_sphere" or kind == "all":
        assert rows.max() > 256 // team, "rows longer than one stride of the wide form (256 / QP entries)"
    if kind == "all":
        assert rows.max() == nd == 289 and cols.max() == 1
    rng = np.random.default_rng(1000 * q + p)
    terms, n_s = _random_terms(rng, q, len(ci))
    x = rng.standard_normal(q * nd)
    Phi = rng.standard_normal((p, q)) if phi_given else None
    Phi_ref = Phi if phi_given else ko.identity_phi(p, q)
    w_rand = rng.uniform(0.5, 2.0, (p, n_obs)) * (rng.uniform(size=(p, n_obs)) >= 1.0 / 3.0)
    if w_rand.size >= 30:
        assert 0.1 < (w_rand == 0.0).mean() < 0.6
    c.kron_compute(terms)
    y_plain = c.kron_spmv(x)
    y_pat, mag_pat = ko.pattern_product_ld(terms, rp, ci, nd, x)
    k = ko.product_counts(n_s * (int(np.diff(rp).max()) + q) + 2, nd, q, p, Psi)
    refs = {}
    for weights, scale in ((None, -1.0), (w_rand, 0.37)):
        z, zm = ko.term_product_ld(Phi_ref, Psi, weights, scale, x)
        refs[scale] = (y_pat + z, 2 * k * np.longdouble(EPS) * (mag_pat + zm))
    bits = {}
    for form in (0, 1, 2):
        c.tune("kron_obs_form", form)
        for weights, scale in ((None, -1.0), (w_rand, 0.37)):
            c.kron_set_obs(Psi, Phi=Phi, weights=np.ones((p, n_obs)) if weights is None and not phi_given else weights, scale=scale)
            info = c.kron_obs_info()
            assert info["p"] == p and info["n_obs"] == n_obs and info["nnz"] == Psi.nnz
            if form == 0:
                assert info["form_rows"] == _rule(n_obs, Psi.nnz) and info["form_cols"] == _rule(nd, Psi.nnz)
                if kind in (2, "all"):
                    assert info["form_rows"] == 2
                if kind in ("pointwise", "single"):
                    assert info["form_rows"] == 1 and info["form_cols"] == 1
            else:
                assert info["form_rows"] == form and info["form_cols"] == form
            y_ref, bound = refs[scale]
            y = c.kron_spmv(x)
            err = np.abs(y.astype(np.longdouble) - y_ref)
            worst = float(np.max(err / np.maximum(bound, np.longdouble(1e-300))))
            _worst_product[0] = max(_worst_product[0], worst)
            print(f"{name} P{order} {kind} q {q} p {p}{'' if phi_given else ' Phi NULL'}: form {form} -> {info['form_rows']}/{info['form_cols']}, scale {scale}, weights "
                  f"{'random' if weights is not None else 'none'}: Psi {n_obs} x {nd}, longest row {rows.max()} / column {cols.max()}, worst |y - y_ref| / bound = "
                  f"{worst:.4f} (so far {_worst_product[0]:.4f})")
            assert np.all(err <= bound)
            assert np.array_equal(c.kron_spmv(x), y)
            if Psi.nnz > 0 and (weights is None or w_rand.any()):
                assert not np.array_equal(y, y_plain)
            bits[(info["form_rows"], info["form_cols"], scale)] = bits.get((info["form_rows"], info["form_cols"], scale), y)
            assert np.array_equal(bits[(info["form_rows"], info["form_cols"], scale)], y), "the rule's choice runs the same kernels as the forced form"
    c.tune("kron_obs_form", 0)
    c.kron_set_obs(None)
    assert np.array_equal(c.kron_spmv(x), y_plain)


# ---- 2. factored against on the pattern -----------------------------------------------------------------------------------------------------------
def test_factored_selection_term_against_the_five_term_handle(env):
    """unit_square_16 P1, m = 5: Psi = the rows of the identity at the observed nodes, Phi = NULL with p = m, no weights, scale -1 on the four-term handle is
    the five-term handle of kron_ref.spacetime_terms.  The products agree within the sum of the two bounds, GMRES by name meets its stop rule on both, both
    solutions are within 1e-6 of SuperLU"""
    import scipy.sparse.linalg as spl

    capi = env[0]
    s = _space(env, "unit_square_16", 1)
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    r1, r0 = _init(env, s)
    m, lam = 5, 1e-4
    q = 2 * m
    obs = br.observed_nodes(s["mesh"].n_nodes)
    Psi = sp.csr_matrix((np.ones(len(obs)), (np.arange(len(obs)), obs)), shape=(len(obs), nd))
    five = kr.spacetime_terms(rp, ci, r1, r0, obs, lam, lam, m)
    A = kr.explicit(five, rp, ci, nd)
    b = kr.spacetime_rhs(obs, lam, nd, m)
    x = np.random.default_rng(21).standard_normal(q * nd)
    max_len = int(np.diff(rp).max())
    y_ref, mag = kr.matvec_ld(A, x)
    bound5 = 2 * (4 * (max_len + q) + 2) * np.longdouble(EPS) * mag
    k4 = ko.product_counts(3 * (max_len + q) + 2, nd, q, m, Psi)
    bound4 = 2 * k4 * np.longdouble(EPS) * mag   # (|A| |x| of the explicit system: the selection term's entries are the Gram term's)
    c.kron_compute(five, symmetric=True)
    y5 = c.kron_spmv(x)
    x5, i5 = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=ko.RTOL, maxit=ko.MAXIT_CAP)
    c.kron_compute(five[1:], symmetric=True)
    c.kron_set_obs(Psi, Phi=None, weights=None, scale=-1.0)   # (p = q without weights ...)
    assert c.kron_obs_info()["p"] == q
    c.kron_set_obs((Psi.indptr.astype(np.int64), Psi.indices.astype(np.int32), Psi.data), Phi=None, weights=np.ones((m, len(obs))), scale=-1.0)   # ... p = m with them
    info = c.kron_obs_info()
    assert info["p"] == m and info["form_rows"] == 1 and info["form_cols"] == 1
    y4 = c.kron_spmv(x)
    x4, i4 = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=ko.RTOL, maxit=ko.MAXIT_CAP)
    c.kron_set_obs(None)
    assert np.all(np.abs(y5 - y_ref) <= bound5) and np.all(np.abs(y4 - y_ref) <= bound4)
    assert np.all(np.abs(y4.astype(np.longdouble) - y5) <= bound4 + bound5)
    x_lu = spl.splu(A.tocsc()).solve(b)
    e4, e5 = np.linalg.norm(x4 - x_lu) / np.linalg.norm(x_lu), np.linalg.norm(x5 - x_lu) / np.linalg.norm(x_lu)
    print(f"factored / on the pattern: iterations {i4.iters} / {i5.iters}, relres {i4.relres:.2e} / {i5.relres:.2e}, error against LU {e4:.2e} / {e5:.2e}, worst "
          f"|y4 - y5| / bound = {float(np.max(np.abs(y4.astype(np.longdouble) - y5) / np.maximum(bound4 + bound5, np.longdouble(1e-300)))):.4f}")
    for i in (i4, i5):
        assert i.converged == 1 and i.method_used == capi.SOLVER_GMRES and 0 < i.relres <= ko.RTOL and i.iters <= ko.MAXIT_CAP
    assert e4 <= 1e-6 and e5 <= 1e-6


# ---- 3. - 4. the space-time smoothing system with a factored term -----------------------------------------------------------------------------------
_systems = {}


def _spacetime(env, case):
    """-> (space, A, b, Psi, Phi, W, terms, D^-1, LU solution) with the handle computed and the term set; one factorisation per case"""
    import scipy.sparse.linalg as spl

    _, _, o = env
    name, order, m, p, lam, lam_t, design, miss = case
    s = _space(env, name, order)
    if case not in _systems:
        r1, r0 = _init(env, s)
        Psi = ko.design_psi(o, s["mesh"], name, order, s["dofs"], s["nd"], design)
        terms, Phi, W, b = ko.spacetime(s["rp"], s["ci"], r1, r0, Psi, lam, lam_t, m, p, miss)
        A = ko.system(terms, s["rp"], s["ci"], s["nd"], Phi, Psi, W)
        _systems[case] = (A, b, Psi, Phi, W, terms, spl.splu(A.tocsc()).solve(b))
    A, b, Psi, Phi, W, terms, x_lu = _systems[case]
    s["c"].kron_compute(terms, symmetric=True)
    s["c"].kron_set_obs(Psi, Phi=Phi, weights=W, scale=-1.0)
    return s, A, b, Psi, Phi, W, terms, x_lu


@pytest.mark.parametrize("case", ko.SOLVE_CASES, ids=lambda c: f"{c[0]}-P{c[1]}-m{c[2]}-p{c[3]}-{c[4]:g}-{c[5]:g}-{'-'.join(map(str, c[6]))}-{c[7]}")
def test_gmres_by_name_with_a_factored_term(env, case):
    """FDAPDE_SOLVER_GMRES, rtol 1e-10, at most 1 000 iterations (a cap: the reference needs 133 - 405, tests/test_kron_obs_cpu.py): converged, the scaled
    residual recomputed in np.longdouble with numpy's own inverses of the full matrix's D_i <= 10 RTOL, the error against SuperLU <= 1e-6; kron_fuse 0 and 1
    give the same bits; on the first case three right-hand sides, each equal to its one-column solve"""
    capi = env[0]
    s, A, b, Psi, Phi, W, terms, x_lu = _spacetime(env, case)
    c, nd, q = s["c"], s["nd"], 2 * case[2]
    Dinv = kr.block_jacobi_q(A, nd, q)
    x, info = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=ko.RTOL, maxit=ko.MAXIT_CAP)
    res = kr.scaled_residual_ld(A, Dinv, b, x)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    oi = c.kron_obs_info()
    print(f"{case}: Psi {Psi.shape[0]} x {nd}, forms {oi['form_rows']}/{oi['form_cols']}, iterations {info.iters}, relres {info.relres:.2e}, recomputed {res:.2e}, "
          f"error against LU {err:.2e}")
    assert info.converged == 1 and info.method_used == capi.SOLVER_GMRES
    assert 0 < info.iters <= ko.MAXIT_CAP and 0 < info.relres <= ko.RTOL
    assert res <= 10 * ko.RTOL
    assert err <= 1e-6
    c.tune("kron_fuse", 0)
    try:
        x0, i0 = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=ko.RTOL, maxit=ko.MAXIT_CAP)
    finally:
        c.tune("kron_fuse", 1)
    assert np.array_equal(x0, x) and i0.iters == info.iters
    if case == ko.SOLVE_CASES[0]:
        import scipy.sparse.linalg as spl

        rng = np.random.default_rng(8)   # (two more right-hand sides of the system's own kind: other observations z and forcings u)
        B = np.column_stack([b, ko.spacetime_rhs(Phi, Psi, W, case[4], case[2], nd, rng), ko.spacetime_rhs(Phi, Psi, W, case[4], case[2], nd, rng)])
        X, i3 = c.kron_solve(B, method=capi.SOLVER_GMRES, rtol=ko.RTOL, maxit=ko.MAXIT_CAP)
        assert i3.converged == 1 and np.array_equal(X[:, 0], x)
        lu = spl.splu(A.tocsc())
        for j in range(3):
            assert kr.scaled_residual_ld(A, Dinv, B[:, j], X[:, j]) <= 10 * ko.RTOL
            ref = lu.solve(B[:, j])
            assert np.linalg.norm(X[:, j] - ref) <= 1e-6 * np.linalg.norm(ref)


@pytest.mark.parametrize("case", ko.DENSE_CASES, ids=lambda c: f"{c[0]}-{'-'.join(map(str, c[6]))}")
def test_dense_by_name_with_a_factored_term(env, case):
    """FDAPDE_SOLVER_DENSE on the merged matrix, on the designs the Krylov stage cannot do within the cap: the bar of tests/test_gpu_kron.py's dense stage --
    residual <= 1e-9 |b|, solution <= 1e-7 |ref|"""
    capi = env[0]
    s, A, b, Psi, Phi, W, terms, x_lu = _spacetime(env, case)
    if case[0] == "unit_square_16":
        assert A.shape[0] == 2890
    x, info = s["c"].kron_solve(b, method=capi.SOLVER_DENSE)
    print(f"{case}: residual {np.linalg.norm(A @ x - b) / np.linalg.norm(b):.2e}, error {np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu):.2e}")
    assert info.method_used == capi.SOLVER_DENSE and info.converged == 1 and np.isfinite(info.relres) and info.iters in (0, 1)
    assert np.linalg.norm(A @ x - b) <= 1e-9 * np.linalg.norm(b)
    assert np.linalg.norm(x - x_lu) <= 1e-7 * np.linalg.norm(x_lu)


def test_dense_by_name_above_the_limit_is_refused(env):
    """unit_sphere P1, q = 16: q n = 9 392 > 8 192"""
    capi = env[0]
    s = _space(env, "unit_sphere", 1)
    c, nd = s["c"], s["nd"]
    assert 16 * nd == 9392
    rng = np.random.default_rng(5)
    c.kron_compute(_random_terms(rng, 16, len(s["ci"]))[0])
    c.kron_set_obs(_psi(env, s, "unit_sphere", 1, 2), Phi=rng.standard_normal((3, 16)))
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(np.ones(16 * nd), method=capi.SOLVER_DENSE)
    assert e.value.status == capi.EUNSUPPORTED
    c.kron_set_obs(None)


def test_open_method_hands_over_to_the_dense_inverse_with_a_term(env):
    """rent or buy as without a term, the parts of the rule that no clock decides: never the inverse within the first `dense_after` (2) columns of a matrix;
    with `dense_after` = 0 the inverse of the MERGED matrix at once, and it stays; a change of the term drops it"""
    capi = env[0]
    s, A, b, Psi, Phi, W, terms, x_lu = _spacetime(env, ko.SOLVE_CASES[0])
    c = s["c"]
    seen = []
    for _ in range(2):
        x, info = c.kron_solve(b)
        seen.append(info.method_used)
        assert info.converged == 1 and np.linalg.norm(x - x_lu) <= 1e-6 * np.linalg.norm(x_lu)
    c.tune("dense_after", 0)
    try:
        for _ in range(2):
            x, info = c.kron_solve(b)
            seen.append(info.method_used)
            assert info.converged == 1 and np.linalg.norm(x - x_lu) <= 1e-6 * np.linalg.norm(x_lu)
    finally:
        c.tune("dense_after", 2)
    x, info = c.kron_solve(b)
    seen.append(info.method_used)
    c.kron_set_obs(Psi, Phi=Phi, weights=W, scale=-1.0)   # the same term again: a new matrix as far as the handle knows
    x, info = c.kron_solve(b)
    seen.append(info.method_used)
    print("stages:", seen)
    assert seen == [capi.SOLVER_GMRES, capi.SOLVER_GMRES, capi.SOLVER_DENSE, capi.SOLVER_DENSE, capi.SOLVER_DENSE, capi.SOLVER_GMRES]


# ---- 5. lifecycle ---------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_of_the_term(env):
    capi, _, o = env
    s = _space(env, "unit_square_16", 1, fresh=True)
    never = _space(env, "unit_square_16", 1, fresh=True)   # a context that never has a term
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    Psi = _psi(env, s, "unit_square_16", 1, 4)
    n_obs = Psi.shape[0]
    q, p = 4, 3
    rng = np.random.default_rng(7)
    Phi = rng.standard_normal((p, q))
    with pytest.raises(capi.FdapdeError) as e:   # before fdapde_kron_compute
        c.kron_set_obs(Psi, Phi=Phi)
    assert e.value.status == capi.ENOTINIT
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_obs_info()
    assert e.value.status == capi.ENOTINIT
    terms, _ = _random_terms(rng, q, len(ci))
    x = rng.standard_normal(q * nd)
    c.kron_compute(terms)
    never["c"].kron_compute(terms)
    y_plain = never["c"].kron_spmv(x)
    assert np.array_equal(c.kron_spmv(x), y_plain)
    with pytest.raises(capi.FdapdeError) as e:   # no term yet
        c.kron_obs_info()
    assert e.value.status == capi.ENOTINIT
    c.kron_set_obs(Psi, Phi=Phi)
    y_term = c.kron_spmv(x)
    assert not np.array_equal(y_term, y_plain)
    assert np.allclose(y_term - y_plain, ko.term(Phi, Psi, None, -1.0) @ x, rtol=0, atol=1e-12 * np.abs(y_plain).max())
    # replacement: other weights change the product accordingly
    w = rng.uniform(0.5, 2.0, (p, n_obs)) * (rng.uniform(size=(p, n_obs)) >= 0.3)
    c.kron_set_obs(Psi, Phi=Phi, weights=w, scale=0.5)
    y_w = c.kron_spmv(x)
    assert np.allclose(y_w - y_plain, ko.term(Phi, Psi, w, 0.5) @ x, rtol=0, atol=1e-12 * np.abs(y_plain).max())
    assert not np.array_equal(y_w, y_term)
    # each malformed input: FDAPDE_EINVAL, and the previous term stays live
    ip, ix, v = Psi.indptr.astype(np.int64), Psi.indices.astype(np.int32), Psi.data.copy()
    good = (ip, ix, v)
    bad = []
    t = ix.copy(); t[3] = nd; bad.append(dict(Psi=(ip, t, v), Phi=Phi))                                # a column outside [0, n_dofs)
    t = ix.copy(); t[3] = -1; bad.append(dict(Psi=(ip, t, v), Phi=Phi))
    t = ix.copy(); t[[0, 1]] = t[[1, 0]]; bad.append(dict(Psi=(ip, t, v), Phi=Phi))                    # a row that is not strictly ascending
    t = ip.copy(); t[2] = t[1] - 1; bad.append(dict(Psi=(t, ix, v), Phi=Phi))                          # a non-monotone rowptr
    t = v.copy(); t[5] = np.nan; bad.append(dict(Psi=(ip, ix, t), Phi=Phi))                            # a value, a weight, a scale, an entry of Phi not finite
    t = w.copy(); t[p - 1, n_obs - 1] = np.inf; bad.append(dict(Psi=good, Phi=Phi, weights=t))
    bad.append(dict(Psi=good, Phi=Phi, scale=np.nan))
    t = Phi.copy(); t[1, 2] = np.nan; bad.append(dict(Psi=good, Phi=t))
    bad.append(dict(Psi=good, Phi=None, weights=np.ones((q + 1, n_obs))))                              # Phi == NULL with p > q
    bad.append(dict(Psi=good, Phi=np.ones((65, q))))                                                   # p out of range
    for kw in bad:
        with pytest.raises(capi.FdapdeError) as e:
            c.kron_set_obs(**kw)
        assert e.value.status == capi.EINVAL and "fdapde_kron_set_obs" in str(e.value)
        assert np.array_equal(c.kron_spmv(x), y_w)
    dp = C.POINTER(C.c_double)
    assert c.lib.fdapde_kron_set_obs(c._ctx, 0, Phi.ctypes.data_as(dp), C.c_int64(n_obs), ip.ctypes.data_as(C.POINTER(C.c_int64)), ix.ctypes.data_as(C.POINTER(C.c_int32)),
                                     v.ctypes.data_as(dp), None, C.c_double(-1.0)) == capi.EINVAL     # p = 0
    assert np.array_equal(c.kron_spmv(x), y_w)
    # FDAPDE_SOLVER_KRON_AMG with a term is refused; after clearing the term it solves again
    r1 = o.assemble_operator(s["mesh"], 1, s["dofs"], nd, -o.laplacian())
    r0 = o.assemble_operator(s["mesh"], 1, s["dofs"], nd, o.reaction(1.0))
    obs = br.observed_nodes(s["mesh"].n_nodes)
    m = 3
    st = kr.spacetime_terms(rp, ci, r1.values, r0.values, obs, 1e-4, 1e-4, m)
    b = kr.spacetime_rhs(obs, 1e-4, nd, m)
    xs = rng.standard_normal(2 * m * nd)
    c.kron_compute(st, symmetric=True)
    with pytest.raises(capi.FdapdeError) as e:   # the new matrix dropped the term
        c.kron_obs_info()
    assert e.value.status == capi.ENOTINIT
    c.kron_set_obs(Psi, Phi=np.hstack([np.eye(m), np.zeros((m, m))]))
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(b, method=capi.SOLVER_KRON_AMG)
    assert e.value.status == capi.EUNSUPPORTED and "term" in str(e.value)
    c.kron_solve(b, method=capi.SOLVER_GMRES, raise_on_noconv=False)   # (the term takes part in a solve before it is cleared)
    c.kron_set_obs(None)   # n_obs = 0 clears it
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_obs_info()
    assert e.value.status == capi.ENOTINIT
    xa, info = c.kron_solve(b, method=capi.SOLVER_KRON_AMG)
    A = kr.explicit(st, rp, ci, nd)
    assert info.converged == 1 and info.method_used == capi.SOLVER_KRON_AMG and np.linalg.norm(A @ xa - b) <= 1e-8 * np.linalg.norm(b)
    never["c"].kron_compute(st, symmetric=True)   # cleared: the pattern-only handle again, bit for bit
    assert np.array_equal(c.kron_spmv(xs), never["c"].kron_spmv(xs))
    xg, ig = c.kron_solve(b, method=capi.SOLVER_GMRES)
    xn, in_ = never["c"].kron_solve(b, method=capi.SOLVER_GMRES)
    assert np.array_equal(xg, xn) and ig.iters == in_.iters
    # after a new fdapde_kron_compute the product is the pattern-only one again, bit for bit
    c.kron_compute(terms)
    c.kron_set_obs(Psi, Phi=Phi, weights=w)
    c.kron_compute(terms)
    assert np.array_equal(c.kron_spmv(x), y_plain)
    # a rowptr of NULL clears as n_obs = 0 does
    c.kron_set_obs(Psi, Phi=Phi)
    assert c.lib.fdapde_kron_set_obs(c._ctx, 3, None, C.c_int64(3), None, None, None, None, C.c_double(-1.0)) == capi.OK
    assert np.array_equal(c.kron_spmv(x), y_plain)
    # a clone carries the knob, not the handle or the term
    c.kron_set_obs(Psi, Phi=Phi)
    c.tune("kron_obs_form", 2)
    k = c.clone()
    with pytest.raises(capi.FdapdeError) as e:
        k.kron_obs_info()
    assert e.value.status == capi.ENOTINIT
    with pytest.raises(capi.FdapdeError) as e:
        k.kron_set_obs(Psi, Phi=Phi)
    assert e.value.status == capi.ENOTINIT
    k.kron_compute(terms)
    k.kron_set_obs(sp.csr_matrix((np.array([0.75]), np.array([1]), np.array([0, 1])), shape=(1, nd)), Phi=Phi)   # (a one-entry Psi: narrow by the rule)
    assert k.kron_obs_info()["form_rows"] == 2 and k.kron_obs_info()["form_cols"] == 2
    k.close()
    # a new space drops the handle and the term with it
    c.dofs_build(1)
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_obs_info()
    assert e.value.status == capi.ENOTINIT
    c.close()
    never["c"].close()


def test_multi_device_context_is_refused(env):
    capi = env[0]
    c = capi.Context(devices=[0, 0])
    rp = np.array([0, 1], dtype=np.int64)
    ci = np.zeros(1, dtype=np.int32)
    v = np.ones(1)
    n = C.c_int64()
    assert c.lib.fdapde_kron_set_obs(c._ctx, 1, None, C.c_int64(1), rp.ctypes.data_as(C.POINTER(C.c_int64)), ci.ctypes.data_as(C.POINTER(C.c_int32)),
                                     v.ctypes.data_as(C.POINTER(C.c_double)), None, C.c_double(-1.0)) == capi.EUNSUPPORTED
    assert c.lib.fdapde_kron_obs_info(c._ctx, None, C.byref(n), None, None, None) == capi.EUNSUPPORTED
    c.close()


# ---- 6. diagonal blocks ---------------------------------------------------------------------------------------------------------------------------
def _near_identity_factor(rng, rp, ci, nd):
    """S_d = I + small random off-diagonal entries on the pattern (kron_ref.pivoting_terms)"""
    sd = 0.02 * rng.standard_normal(len(ci))
    sd[kr.gram_slots(rp, ci, nd)] = 1.0
    return sd


def test_the_term_alone_makes_the_diagonal_blocks_invertible(env):
    """A = T_b (x) S_d with a zero first row of T_b: every D_i = T_b is singular -- GMRES by name answers FDAPDE_ENOCONV.  The term 2 e_0 e_0^T (x) Psi^T Psi
    (Phi = NULL, p = 1) with Psi = [I; the 4 x 4 tiles] puts g_i >= 2 into the leading entry: GMRES runs and agrees with SuperLU"""
    import scipy.sparse.linalg as spl

    capi = env[0]
    s = _space(env, "unit_square_16", 1)
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    q = 3
    rng = np.random.default_rng(31)
    Tb = rng.standard_normal((q, q)) / np.sqrt(q) + 3.0 * np.eye(q)
    Tb[0, :] = 0.0
    terms = [(Tb, _near_identity_factor(rng, rp, ci, nd))]
    Psi = sp.vstack([sp.identity(nd, format="csr"), _psi(env, s, "unit_square_16", 1, 4)]).tocsr()
    b = rng.standard_normal(q * nd)
    c.kron_compute(terms)
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(b, method=capi.SOLVER_GMRES)
    assert e.value.status == capi.ENOCONV
    c.kron_set_obs(Psi, Phi=None, weights=np.ones((1, Psi.shape[0])), scale=2.0)
    x, info = c.kron_solve(b, method=capi.SOLVER_GMRES, rtol=ko.RTOL, maxit=ko.MAXIT_CAP)
    A = ko.system(terms, rp, ci, nd, ko.identity_phi(1, q), Psi, None, 2.0)
    x_lu = spl.splu(A.tocsc()).solve(b)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    res = kr.scaled_residual_ld(A, kr.block_jacobi_q(A, nd, q), b, x)
    print(f"the term makes every D_i invertible: iterations {info.iters}, relres {info.relres:.2e}, recomputed {res:.2e}, error against LU {err:.2e}")
    assert info.method_used == capi.SOLVER_GMRES and info.converged == 1 and info.relres <= ko.RTOL
    assert res <= 10 * ko.RTOL and err <= 1e-6
    c.kron_set_obs(None)   # ... and singular again without it
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(b, method=capi.SOLVER_GMRES)
    assert e.value.status == capi.ENOCONV


def test_a_term_that_cancels_the_leading_entry_makes_the_blocks_singular(env):
    """A = T_b (x) S_d with T_b[0, 1:] = 0 and S_d[i, i] = 1: D_i = T_b.  Psi = the rows of the identity at the observed nodes, Phi = NULL with p = 1, scale
    -T_b[0, 0]: the first row of D_i is EXACTLY zero at every observed DOF only WITH the term -- GMRES by name answers FDAPDE_ENOCONV, the open method goes
    to the dense inverse of the merged matrix"""
    import scipy.sparse.linalg as spl

    capi = env[0]
    s = _space(env, "unit_square_16", 1)
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    q = 3
    rng = np.random.default_rng(32)
    Tb = rng.standard_normal((q, q)) / np.sqrt(q) + 3.0 * np.eye(q)
    Tb[0, 1:] = 0.0
    terms = [(Tb, _near_identity_factor(rng, rp, ci, nd))]
    obs = br.observed_nodes(s["mesh"].n_nodes)
    Psi = sp.csr_matrix((np.ones(len(obs)), (np.arange(len(obs)), obs)), shape=(len(obs), nd))
    b = rng.standard_normal(q * nd)
    c.kron_compute(terms)
    x0, info0 = c.kron_solve(b, method=capi.SOLVER_GMRES)   # (without the term the blocks are T_b: the Krylov stage is there)
    assert info0.method_used == capi.SOLVER_GMRES and info0.converged == 1
    c.kron_set_obs(Psi, Phi=None, weights=np.ones((1, len(obs))), scale=-Tb[0, 0])
    with pytest.raises(capi.FdapdeError) as e:
        c.kron_solve(b, method=capi.SOLVER_GMRES)
    assert e.value.status == capi.ENOCONV
    x, info = c.kron_solve(b)
    assert info.method_used == capi.SOLVER_DENSE
    A = ko.system(terms, rp, ci, nd, ko.identity_phi(1, q), Psi, None, -Tb[0, 0])
    assert np.all(A[obs, :][:, obs].diagonal() == 0.0)
    x_lu = spl.splu(A.tocsc()).solve(b)
    assert np.linalg.norm(x - x_lu) <= 1e-7 * np.linalg.norm(x_lu)
    c.kron_set_obs(None)


# ---- 7. neighbours keep their bits ----------------------------------------------------------------------------------------------------------------
def test_other_solves_of_the_context_keep_their_bits(env):
    """fdapde_solve, the n x n handle and the 2 x 2 block handle before and after a Kronecker term is set and used"""
    capi = env[0]
    s = _space(env, "unit_square_16", 1, fresh=True)
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    rhs = np.random.default_rng(2).standard_normal((nd, 3))
    obs = br.observed_nodes(289)
    r1, r0 = c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS)
    blocks = br.smoothing_blocks(rp, ci, r1, r0, obs, 1e-4, nd)
    bb = br.smoothing_rhs(obs, 1e-4, nd)
    c.block_compute(*blocks, symmetric=True)

    def others():
        c.lin_compute(capi.MAT_STIFF)
        X, _ = c.lin_solve(rhs, rtol=1e-12)
        c.solve(rtol=1e-12)
        xg, _ = c.block_solve(bb, method=capi.SOLVER_GMRES)
        return X, c.solution(), xg, c.block_spmv(bb)

    before = others()
    Psi = _psi(env, s, "unit_square_16", 1, 4)
    m, p = 3, 4
    terms, Phi, W, b = ko.spacetime(rp, ci, r1, r0, Psi, 1e-2, 1.0, m, p, 0.3)
    c.kron_compute(terms, symmetric=True)
    c.kron_set_obs(Psi, Phi=Phi, weights=W)
    xk, _ = c.kron_solve(b, method=capi.SOLVER_GMRES, raise_on_noconv=False)
    c.kron_solve(b, method=capi.SOLVER_DENSE)
    c.kron_spmv(b)
    after = others()
    for u, w in zip(before, after):
        assert np.array_equal(u, w)
    xk2, _ = c.kron_solve(b, method=capi.SOLVER_GMRES, raise_on_noconv=False)   # ... and the Kronecker handle kept its own through theirs
    assert np.array_equal(xk, xk2)
    c.close()
