"""The factored data term of the 2 x 2 block handle (csrc/kernels_obs.h, host_obs.cpp, eng_block.hip): fdapde_block_set_obs / fdapde_block_obs_info against
scipy -- the explicit system sp.bmat of the four blocks + scale Psi^T W Psi (tests/block_obs_ref.py), SuperLU, scipy's GMRES(50) on the block-Jacobi-scaled
system (tests/block_ref.py).  Psi is the oracle's: areal rows over tiles of the bounding box or quasi_circle's golden incidence matrix, pointwise rows on
c_shaped.  tests/test_block_obs_cpu.py checks, without a device, that the reference GMRES stays under half of the iteration budget handed over here."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import block_obs_ref as bo
import block_ref as br

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


def _psi(env, s, name, order, kind):
    """kind: tiles per axis | "golden" | "all" (ONE region over all cells) | "pointwise" (c_shaped: locs.csv + points of the bounding box, some outside) |
    "single" (one row with one entry)"""
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
    return 64 if nnz > 16 * rows else 8


# ---- 1. product parity ----------------------------------------------------------------------------------------------------------------------------
PRODUCT_CASES = [("quasi_circle", 1, "golden"), ("quasi_circle", 2, "golden"), ("unit_sphere", 1, 2), ("unit_square_16", 1, "all"), ("c_shaped", 2, "pointwise"),
                 ("one_triangle", 1, "single")]


@pytest.mark.parametrize("name,order,kind", PRODUCT_CASES)
def test_product_with_a_term_against_the_explicit_system(env, name, order, kind):
    """y = (A + scale [Psi^T W Psi, 0; 0, 0]) x for random values in all four blocks, against the explicit system's product in extended precision: per row
    |y - y_ref| <= (terms + 1) eps (|A| |x| + |scale| |Psi|^T |W| |Psi| |x_1|), terms = twice the row's pattern entries + its Psi^T row length + the longest
    Psi row contributing to it -- the bound of that many rounded products summed in any order (the term's inner sums enter through their longest one).  The
    same bits from a second call; under block_obs_team 8 and 64 (reported by fdapde_block_obs_info), and the rule's choice under 0."""
    s = _space(env, name, order)
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    Psi = _psi(env, s, name, order, kind)
    rows = np.diff(Psi.indptr)
    cols = np.bincount(Psi.indices, minlength=nd)
    if name == "quasi_circle":
        assert (cols == 0).sum() > nd // 2, "most DOFs are in no region"
    if name == "unit_sphere":
        assert rows.max() > 64, "rows longer than one pass of 64 lanes"
    if kind == "all":
        assert rows.max() == nd == 289 and cols.max() == 1
    rng = np.random.default_rng(11)
    blocks = [rng.standard_normal(len(ci)) for _ in range(4)]
    x = rng.standard_normal(2 * nd)
    w_rand = rng.uniform(0.5, 2.0, Psi.shape[0])
    c.block_compute(*blocks)
    c.tune("block_obs_team", 0)
    c.block_set_obs(Psi)
    info = c.block_obs_info()
    assert info["n_obs"] == Psi.shape[0] and info["nnz"] == Psi.nnz
    assert info["team_rows"] == _rule(Psi.shape[0], Psi.nnz) and info["team_cols"] == _rule(nd, Psi.nnz)
    if kind in (2, "all"):
        assert info["team_rows"] == 64
    if kind in ("pointwise", "single"):
        assert info["team_rows"] == 8 and info["team_cols"] == 8
    refs = {}
    for team in (8, 64):
        c.tune("block_obs_team", team)
        for weights, scale in ((None, -1.0), (w_rand, 0.37)):
            c.block_set_obs(Psi, weights, scale)
            info = c.block_obs_info()
            assert info["team_rows"] == team and info["team_cols"] == team
            if scale not in refs:
                refs[scale] = (bo.product_reference(rp, ci, blocks, nd, Psi, weights, scale, x), bo.product_bound(rp, ci, blocks, nd, Psi, weights, scale, x))
            y_ref, bound = refs[scale]
            y = c.block_spmv(x)
            err = np.abs(y.astype(np.longdouble) - y_ref).astype(float)
            print(f"{name} P{order} {kind}: team {team}, scale {scale}, weights {'random' if weights is not None else 'none'}: Psi {Psi.shape[0]} x {nd}, "
                  f"longest row {rows.max()} / column {cols.max()}, worst |y - y_ref| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert np.all(err <= bound)
            assert np.array_equal(c.block_spmv(x), y)
    c.tune("block_obs_team", 0)


# ---- 2. pointwise equivalence ---------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("order", [1, 2])
def test_pointwise_term_equals_the_gram_matrix_on_the_pattern(env, order):
    """c_shaped, Psi from fdapde_eval_pointwise: the product with the factored term against the product with -fdapde_gram_pointwise's values in a11.  Both are
    within their own bound of the exact product: the factored one as in test 1; the on-pattern one (2 len + 1) eps |A| |x| (tests/test_gpu_block.py) plus
    what the Gram entries themselves carry, k eps sum |terms| per entry of k terms (test_gram_matrix_on_c_shaped) times |x_j| -- so they agree within the sum.
    The GMRES solutions of the two forms (lambda 1e-2, rtol 1e-12: each solution's error is the scaled system's condition times rtol) agree to 1e-8."""
    capi, workloads, _ = env
    s = _space(env, "c_shaped", order)
    c, nd, rp, ci, m = s["c"], s["nd"], s["rp"], s["ci"], s["mesh"]
    r1, r0 = _init(env, s)
    locs = workloads._read_fixture_csv(os.path.join(MESHES, "c_shaped", "locs.csv"), float)
    rng = np.random.default_rng(3)
    pts = np.concatenate([locs, rng.uniform(m.nodes.min(axis=0), m.nodes.max(axis=0), size=(2000, 2))])
    cells, vals = c.eval_pointwise_raw(pts)
    inside = np.flatnonzero(cells >= 0)
    assert (cells < 0).any() and len(inside) > 1000
    nb = vals.shape[1]
    Psi = sp.csr_matrix((vals[inside].reshape(-1), (np.repeat(inside, nb), s["dofs"][cells[inside]].reshape(-1))), shape=(len(pts), nd))
    Psi.sort_indices()
    lam = 1e-2
    for weights in (None, rng.uniform(0.5, 2.0, len(pts))):
        blocks = bo.smoothing_blocks(rp, ci, r1, r0, lam, nd)
        G = c.gram_pointwise(cells, vals, weights)
        with_gram = (-G,) + blocks[1:]
        x = rng.standard_normal(2 * nd)
        c.block_compute(*with_gram, symmetric=True)
        y_gram = c.block_spmv(x)
        b = bo.smoothing_rhs(Psi, lam, nd)
        x_gram, info_gram = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-12, maxit=2000)
        c.block_compute(*blocks, symmetric=True)
        c.block_set_obs(Psi, weights, -1.0)
        assert c.block_obs_info()["team_rows"] == 8
        y_term = c.block_spmv(x)
        x_term, info_term = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-12, maxit=2000)
        bound_term = bo.product_bound(rp, ci, blocks, nd, Psi, weights, -1.0, x)
        length = np.diff(rp)
        aP = abs(Psi).tocsr()
        w = np.ones(len(pts)) if weights is None else weights
        mag = (aP.T @ sp.diags(w) @ aP).tocsr()                              # sum |terms| per entry of the Gram matrix
        count = (aP.sign().T @ aP.sign()).tocsr()                            # k: its terms
        gram_entry = count.multiply(mag) * EPS
        absA = abs(br.bmat(rp, ci, with_gram, nd))
        bound_gram = (2 * np.concatenate([length, length]) + 1) * EPS * (absA @ np.abs(x))
        bound_gram[:nd] += gram_entry @ np.abs(x[:nd])
        worst = np.max(np.abs(y_term - y_gram) / np.maximum(bound_term + bound_gram, 1e-300))
        diff = np.linalg.norm(x_term - x_gram) / np.linalg.norm(x_gram)
        print(f"c_shaped P{order}, weights {'random' if weights is not None else 'none'}: worst |y_term - y_gram| / bound = {worst:.3f}; GMRES iterations "
              f"{info_term.iters} (term) / {info_gram.iters} (gram), |x_term - x_gram| / |x_gram| = {diff:.2e}")
        assert np.all(np.abs(y_term - y_gram) <= bound_term + bound_gram)
        assert info_term.converged == 1 and info_gram.converged == 1
        assert diff <= 1e-8


# ---- 3. - 5. the smoothing system with an areal term -------------------------------------------------------------------------------------------
_systems = {}


def _smoothing(env, name, order, lam, regions):
    """-> (space, A, b, Psi, blocks, LU solution) with the handle computed and the term set"""
    import scipy.sparse.linalg as spl

    s = _space(env, name, order)
    key = (name, order, lam, regions)
    if key not in _systems:
        r1, r0 = _init(env, s)
        Psi = _psi(env, s, name, order, regions)
        blocks = bo.smoothing_blocks(s["rp"], s["ci"], r1, r0, lam, s["nd"])
        A = bo.system(s["rp"], s["ci"], blocks, s["nd"], Psi)
        b = bo.smoothing_rhs(Psi, lam, s["nd"])
        _systems[key] = (A, b, Psi, blocks, spl.splu(A.tocsc()).solve(b))
    A, b, Psi, blocks, x_lu = _systems[key]
    s["c"].block_compute(*blocks, symmetric=True)
    s["c"].block_set_obs(Psi)
    return s, A, b, Psi, blocks, x_lu


@pytest.mark.parametrize("name,order,lam,regions", bo.KRYLOV_CASES)
def test_gmres_by_name_with_an_areal_term(env, name, order, lam, regions):
    """FDAPDE_SOLVER_GMRES, rtol 1e-10, at most 1 000 iterations (a cap: the reference needs 97 - 291, tests/test_block_obs_cpu.py): relres <= rtol, the scaled
    residual recomputed by scipy <= 1e-9, and the error against LU within 10 times that of scipy's GMRES(50) on the same scaled system"""
    capi = env[0]
    s, A, b, Psi, _, x_lu = _smoothing(env, name, order, lam, regions)
    nd = s["nd"]
    Dinv = br.block_jacobi(A, nd)
    x_ref, it_ref, info_ref = br.reference_gmres(A, Dinv, b)
    assert info_ref == 0
    e_ref = np.linalg.norm(x_ref - x_lu) / np.linalg.norm(x_lu)
    x, info = s["c"].block_solve(b, method=capi.SOLVER_GMRES, rtol=bo.RTOL, maxit=bo.MAXIT_CAP)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    res = br.scaled_residual(A, Dinv, b, x)
    print(f"{name} P{order} lambda {lam:g}, {Psi.shape[0]} regions: iterations {info.iters} (scipy {it_ref}), relres {info.relres:.2e}, recomputed {res:.2e}, "
          f"error against LU {err:.2e} (scipy {e_ref:.2e})")
    assert info.converged == 1 and info.method_used == capi.SOLVER_GMRES
    assert info.relres <= bo.RTOL
    assert res <= 1e-9
    assert info.iters <= bo.MAXIT_CAP
    assert err <= 10 * e_ref


@pytest.mark.parametrize("name,order,regions", [("quasi_circle", 2, "golden"), ("unit_square_16", 1, 4)])
def test_dense_by_name_with_an_areal_term(env, name, order, regions):
    """FDAPDE_SOLVER_DENSE on the merged matrix: the tolerances of test_dense_by_name_on_the_smoothing_system -- residual <= 1e-9 |b|, error <= 1e-7 |x_lu|"""
    capi = env[0]
    s, A, b, _, _, x_lu = _smoothing(env, name, order, 1e-4, regions)
    if name == "quasi_circle":
        assert 2 * s["nd"] == 2622
    x, info = s["c"].block_solve(b, method=capi.SOLVER_DENSE)
    print(f"{name} P{order}: residual {np.linalg.norm(A @ x - b) / np.linalg.norm(b):.2e}, error {np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu):.2e}")
    assert info.method_used == capi.SOLVER_DENSE and info.converged == 1
    assert np.linalg.norm(A @ x - b) <= 1e-9 * np.linalg.norm(b)
    assert np.linalg.norm(x - x_lu) <= 1e-7 * np.linalg.norm(x_lu)


def test_dense_by_name_above_the_limit_is_refused(env):
    """unit_sphere P2: 2 n = 8 386 > 8 192"""
    capi = env[0]
    s = _space(env, "unit_sphere", 2)
    c, nd = s["c"], s["nd"]
    assert 2 * nd == 8386
    rng = np.random.default_rng(5)
    c.block_compute(*[rng.standard_normal(len(s["ci"])) for _ in range(4)])
    c.block_set_obs(_psi(env, s, "unit_sphere", 2, 2))
    with pytest.raises(capi.FdapdeError) as e:
        c.block_solve(np.ones(2 * nd), method=capi.SOLVER_DENSE)
    assert e.value.status == capi.EUNSUPPORTED


def test_open_method_hands_over_to_the_dense_inverse_with_a_term(env):
    """rent or buy as without a term: GMRES for the first `dense_after` (2) columns, the inverse of the MERGED matrix once the Krylov columns have cost half of it"""
    capi = env[0]
    s, A, b, _, _, x_lu = _smoothing(env, "unit_square_16", 1, 1e-2, 4)
    seen = []
    for _ in range(8):
        x, info = s["c"].block_solve(b)
        seen.append(info.method_used)
        assert info.converged == 1 and np.linalg.norm(x - x_lu) <= 1e-6 * np.linalg.norm(x_lu)
    print("stages:", seen)
    assert seen[0] == capi.SOLVER_GMRES and seen[1] == capi.SOLVER_GMRES
    assert seen[-1] == capi.SOLVER_DENSE


# ---- 6. lifecycle ---------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_of_the_term(env):
    capi, _, o = env
    s = _space(env, "unit_square_16", 1, fresh=True)
    never = _space(env, "unit_square_16", 1, fresh=True)   # a context that never has a term
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    Psi = _psi(env, s, "unit_square_16", 1, 4)
    with pytest.raises(capi.FdapdeError) as e:   # before fdapde_block_compute
        c.block_set_obs(Psi)
    assert e.value.status == capi.ENOTINIT
    rng = np.random.default_rng(7)
    blocks = [rng.standard_normal(len(ci)) for _ in range(4)]
    x = rng.standard_normal(2 * nd)
    c.block_compute(*blocks)
    never["c"].block_compute(*blocks)
    y_plain = never["c"].block_spmv(x)
    assert np.array_equal(c.block_spmv(x), y_plain)
    with pytest.raises(capi.FdapdeError) as e:   # no term yet
        c.block_obs_info()
    assert e.value.status == capi.ENOTINIT
    c.block_set_obs(Psi)
    y_term = c.block_spmv(x)
    T = bo.term(Psi, None, -1.0)
    assert not np.array_equal(y_term, y_plain)
    assert np.allclose(y_term[:nd] - y_plain[:nd], T @ x[:nd], rtol=0, atol=1e-12 * np.abs(y_plain).max()) and np.array_equal(y_term[nd:], y_plain[nd:])
    # replacing the weights changes the product accordingly
    w = rng.uniform(0.5, 2.0, Psi.shape[0])
    c.block_set_obs(Psi, w)
    y_w = c.block_spmv(x)
    assert np.allclose(y_w[:nd] - y_plain[:nd], bo.term(Psi, w, -1.0) @ x[:nd], rtol=0, atol=1e-12 * np.abs(y_plain).max())
    assert not np.array_equal(y_w, y_term)
    # each malformed input: FDAPDE_EINVAL, and the previous term stays live
    ip, ix, v = Psi.indptr.astype(np.int64), Psi.indices.astype(np.int32), Psi.data.copy()
    bad = []
    t = ix.copy(); t[3] = nd; bad.append(((ip, t, v), None, -1.0))                                   # a column outside [0, n_dofs)
    t = ix.copy(); t[3] = -1; bad.append(((ip, t, v), None, -1.0))
    t = ix.copy(); t[[0, 1]] = t[[1, 0]]; bad.append(((ip, t, v), None, -1.0))                       # a row that is not strictly ascending
    t = ix.copy(); t[1] = t[0]; bad.append(((ip, t, v), None, -1.0))
    t = ip.copy(); t[2] = t[1] - 1; bad.append(((t, ix, v), None, -1.0))                             # a non-monotone rowptr
    t = v.copy(); t[5] = np.nan; bad.append(((ip, ix, t), None, -1.0))                               # a value, a weight, a scale that is not finite
    t = w.copy(); t[0] = np.inf; bad.append(((ip, ix, v), t, -1.0))
    bad.append(((ip, ix, v), None, np.nan))
    for psi, weights, scale in bad:
        with pytest.raises(capi.FdapdeError) as e:
            c.block_set_obs(psi, weights, scale)
        assert e.value.status == capi.EINVAL
        assert np.array_equal(c.block_spmv(x), y_w)
    # FDAPDE_SOLVER_BLOCK_AMG with a term is refused; after clearing the term it solves again
    r1 = o.assemble_operator(s["mesh"], 1, s["dofs"], nd, -o.laplacian())
    r0 = o.assemble_operator(s["mesh"], 1, s["dofs"], nd, o.reaction(1.0))
    obs = br.observed_nodes(s["mesh"].n_nodes)
    sm = br.smoothing_blocks(rp, ci, r1.values, r0.values, obs, 1e-4, nd)
    b = br.smoothing_rhs(obs, 1e-4, nd)
    c.block_compute(*sm, symmetric=True)
    with pytest.raises(capi.FdapdeError) as e:   # the new matrix dropped the term
        c.block_obs_info()
    assert e.value.status == capi.ENOTINIT
    c.block_set_obs(Psi)
    with pytest.raises(capi.FdapdeError) as e:
        c.block_solve(b, method=capi.SOLVER_BLOCK_AMG)
    assert e.value.status == capi.EUNSUPPORTED and "term" in str(e.value)
    c.block_set_obs(None)   # n_obs = 0 clears it
    with pytest.raises(capi.FdapdeError) as e:
        c.block_obs_info()
    assert e.value.status == capi.ENOTINIT
    xa, info = c.block_solve(b, method=capi.SOLVER_BLOCK_AMG)
    A = br.bmat(rp, ci, sm, nd)
    assert info.converged == 1 and info.method_used == capi.SOLVER_BLOCK_AMG and np.linalg.norm(A @ xa - b) <= 1e-8 * np.linalg.norm(b)
    never["c"].block_compute(*sm, symmetric=True)   # cleared: the pattern-only handle again, bit for bit
    assert np.array_equal(c.block_spmv(x), never["c"].block_spmv(x))
    xg, _ = c.block_solve(b, method=capi.SOLVER_GMRES)
    xn, _ = never["c"].block_solve(b, method=capi.SOLVER_GMRES)
    assert np.array_equal(xg, xn)
    # after a new fdapde_block_compute the product is the pattern-only one again, bit for bit
    c.block_set_obs(Psi, w)
    c.block_compute(*blocks)
    assert np.array_equal(c.block_spmv(x), y_plain)
    # a rowptr of NULL clears as n_obs = 0 does
    c.block_set_obs(Psi)
    assert c.lib.fdapde_block_set_obs(c._ctx, C.c_int64(3), None, None, None, None, C.c_double(-1.0)) == capi.OK
    assert np.array_equal(c.block_spmv(x), y_plain)
    c.close()
    never["c"].close()


def test_multi_device_context_is_refused(env):
    capi = env[0]
    c = capi.Context(devices=[0, 0])
    rp = np.array([0, 1], dtype=np.int64)
    ci = np.zeros(1, dtype=np.int32)
    v = np.ones(1)
    n = C.c_int64()
    assert c.lib.fdapde_block_set_obs(c._ctx, C.c_int64(1), rp.ctypes.data_as(C.POINTER(C.c_int64)), ci.ctypes.data_as(C.POINTER(C.c_int32)),
                                      v.ctypes.data_as(C.POINTER(C.c_double)), None, C.c_double(-1.0)) == capi.EUNSUPPORTED
    assert c.lib.fdapde_block_obs_info(c._ctx, C.byref(n), None, None, None) == capi.EUNSUPPORTED
    c.close()


# ---- 7. singular diagonal blocks ------------------------------------------------------------------------------------------------------------------
def test_the_term_alone_makes_a_diagonal_block_invertible(env):
    """a11 NULL and a12 = a21 = 0 on the diagonal of one DOF that lies in a region: D_i = diag(0, a22) without the term -- GMRES by name is refused --,
    diag(g_i, a22) with it: GMRES runs"""
    import scipy.sparse.linalg as spl

    capi = env[0]
    s = _space(env, "unit_square_16", 1)
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    r1, r0 = _init(env, s)
    Psi = _psi(env, s, "unit_square_16", 1, 4)
    i = int(Psi.indices[Psi.indptr[5]])
    d = rp[i] + np.searchsorted(ci[rp[i]:rp[i + 1]], i)
    blocks = [None if v is None else v.copy() for v in bo.smoothing_blocks(rp, ci, r1, r0, 1e-2, nd)]
    blocks[1][d] = 0.0
    blocks[2][d] = 0.0
    b = bo.smoothing_rhs(Psi, 1e-2, nd)
    c.block_compute(*blocks, symmetric=True)
    with pytest.raises(capi.FdapdeError) as e:
        c.block_solve(b, method=capi.SOLVER_GMRES)
    assert e.value.status == capi.EUNSUPPORTED
    c.block_set_obs(Psi)
    x, info = c.block_solve(b, method=capi.SOLVER_GMRES, rtol=1e-10, maxit=2000)
    A = bo.system(rp, ci, blocks, nd, Psi)
    x_lu = spl.splu(A.tocsc()).solve(b)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    print(f"the term makes D_{i} invertible: iterations {info.iters}, relres {info.relres:.2e}, error against LU {err:.2e}")
    assert info.method_used == capi.SOLVER_GMRES and info.converged == 1 and info.relres <= 1e-10
    assert br.scaled_residual(A, br.block_jacobi(A, nd), b, x) <= 1e-9


def test_a_term_that_cancels_a11_makes_the_block_singular(env):
    """Psi = rows of the identity at the observed nodes (g_i = -1 there, exactly), a11 = +1 and a12 = a21 = 0 on the diagonal of one observed DOF: D_i =
    diag(0, a22) only WITH the term -- GMRES by name is refused, the open method answers through the dense inverse of the merged matrix"""
    import scipy.sparse.linalg as spl

    capi = env[0]
    s = _space(env, "unit_square_16", 1)
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    r1, r0 = _init(env, s)
    obs = br.observed_nodes(s["mesh"].n_nodes)
    Psi = sp.csr_matrix((np.ones(len(obs)), (np.arange(len(obs)), obs)), shape=(len(obs), nd))
    i = int(obs[3])
    d = rp[i] + np.searchsorted(ci[rp[i]:rp[i + 1]], i)
    blocks = [None if v is None else v.copy() for v in bo.smoothing_blocks(rp, ci, r1, r0, 1e-4, nd)]
    blocks[0] = np.zeros(len(ci))
    blocks[0][d] = 1.0
    blocks[1][d] = 0.0
    blocks[2][d] = 0.0
    b = br.smoothing_rhs(obs, 1e-4, nd)
    c.block_compute(*blocks, symmetric=True)
    x0, info0 = c.block_solve(b, method=capi.SOLVER_GMRES, raise_on_noconv=False)   # (without the term the block is diag(1, a22): the Krylov stage is there)
    assert info0.method_used == capi.SOLVER_GMRES
    c.block_set_obs(Psi)
    with pytest.raises(capi.FdapdeError) as e:
        c.block_solve(b, method=capi.SOLVER_GMRES)
    assert e.value.status == capi.EUNSUPPORTED
    x, info = c.block_solve(b)
    assert info.method_used == capi.SOLVER_DENSE
    x_lu = spl.splu(bo.system(rp, ci, blocks, nd, Psi).tocsc()).solve(b)
    assert np.linalg.norm(x - x_lu) <= 1e-7 * np.linalg.norm(x_lu)


# ---- 8. neighbours keep their bits ----------------------------------------------------------------------------------------------------------------
def test_other_solves_of_the_context_keep_their_bits(env):
    """fdapde_solve and the n x n handle before and after a term is set and used"""
    capi = env[0]
    s = _space(env, "unit_square_16", 1, fresh=True)
    c, nd, rp, ci = s["c"], s["nd"], s["rp"], s["ci"]
    c.set_operator(-capi.laplacian() + capi.reaction(1.0))
    c.set_forcing(np.ones(c.quadrature_nodes().shape[0]))
    c.init()
    rhs = np.random.default_rng(2).standard_normal((nd, 3))

    def others():
        c.lin_compute(capi.MAT_STIFF)
        X, _ = c.lin_solve(rhs, rtol=1e-12)
        c.solve(rtol=1e-12)
        return X, c.solution()

    X0, u0 = others()
    Psi = _psi(env, s, "unit_square_16", 1, 4)
    blocks = bo.smoothing_blocks(rp, ci, c.matrix_values(capi.MAT_STIFF), c.matrix_values(capi.MAT_MASS), 1e-4, nd)
    b = bo.smoothing_rhs(Psi, 1e-4, nd)
    c.block_compute(*blocks, symmetric=True)
    c.block_set_obs(Psi)
    c.block_solve(b, method=capi.SOLVER_GMRES)
    c.block_solve(b, method=capi.SOLVER_DENSE)
    c.block_spmv(b)
    X1, u1 = others()
    assert np.array_equal(X0, X1) and np.array_equal(u0, u1)
    xb, _ = c.block_solve(b, method=capi.SOLVER_GMRES)   # ... and both handles live side by side
    assert np.linalg.norm(bo.system(rp, ci, blocks, nd, Psi) @ xb - b) <= 1e-6 * np.linalg.norm(b)
    c.close()
