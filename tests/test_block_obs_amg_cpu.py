"""FDAPDE_SOLVER_BLOCK_AMG with the factored data term carried (knob block_amg_obs) without a device: the reference side of tests/test_gpu_block_obs_amg.py is
checked here, and the entry point is there.
  * the restatement (tests/block_obs_amg_ref.py: block_amg_ref's hierarchy with the term Psi_l = Psi P_0 ... P_{l-1} on every level) on the fixture cases of
    the GPU test, rebuilt from the ORACLE's matrices: it converges to rtol 1e-10 in at most HALF of the budget the GPU test hands over (block_amg_ref.BUDGET_P1
    = 80, BUDGET_P2_2D = 120) -- a condition with a factor 2 to spare, not a measurement of the code under test --, within two of the count recorded when the
    feature was designed (COUNTS below), and agrees with SuperLU to 1e-6.  Ten of the thirteen counts are the recorded ones; the three that differ are 2 x 2
    tiles on unit_square_16 -- P1 at 1e-4: 16 for 17, P2 at 1e-2: 27 for 25, P2 at 1e-4: 21 for 22.  The P2 rows were recorded with level sizes "about 170"
    only (here 168 and 172: the matching's ties fall differently with lambda), the same three on meshgen's unit_square(16) give 17, 26, 22, and the two
    counts that came out lower stop within 15 - 30 % of the threshold (8.6e-11, 6.9e-11 against 1e-10): a count at the edge, not another method;
  * the other term shapes of the GPU test: weights with exact zeros, a11 on the pattern plus a term, a pointwise Psi of 400 random points;
  * the control: the term on level 0 only, the coarse levels from the pattern part alone, does NOT converge in 200 iterations on unit_square_16 with 4 x 4
    tiles at either lambda -- the coarse term is necessary;
  * the library exports fdapde_block_obs_amg_levels, and a host-only context answers FDAPDE_ENODEVICE."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import block_amg_ref as ba
import block_obs_amg_ref as boa
import block_obs_ref as bo
import block_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# iterations recorded for the restatement when the feature was designed, amg_coarse_rows = 256, rtol 1e-10
COUNTS = {("unit_square_16", 1, 1e-2, 4): 22, ("unit_square_16", 1, 1e-4, 4): 19, ("unit_square_16", 1, 1e-2, 2): 20, ("unit_square_16", 1, 1e-4, 2): 17,
          ("unit_square_16", 2, 1e-4, 4): 25, ("unit_square_16", 2, 1e-2, 2): 25, ("unit_square_16", 2, 1e-4, 2): 22, ("c_shaped", 2, 1e-2, 3): 26,
          ("c_shaped", 2, 1e-4, 3): 23, ("unit_sphere", 1, 1e-2, 2): 20, ("unit_sphere", 1, 1e-4, 2): 19, ("quasi_circle", 1, 1e-2, "golden"): 19,
          ("quasi_circle", 1, 1e-4, "golden"): 23}
_cases = {}


def _case(oracle, mesh_loader, name, order, lam, regions):
    key = (name, order, lam, regions)
    if key not in _cases:
        A, b, nd, Psi, (rp, ci, blocks) = bo.oracle_case(oracle, mesh_loader, name, order, lam, regions)
        _cases[key] = (A, b, nd, Psi, rp, ci, blocks, spl.splu(A.tocsc()).solve(b))
    return _cases[key]


@pytest.mark.parametrize("name,order,lam,regions", boa.AREAL_CASES)
def test_restatement_with_the_term_stays_under_half_of_the_budget(oracle, mesh_loader, name, order, lam, regions):
    A, b, nd, Psi, rp, ci, blocks, x_lu = _case(oracle, mesh_loader, name, order, lam, regions)
    x, it, ok, H = boa.solve(rp, ci, blocks, nd, Psi, b)
    err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print(f"{name} P{order} lambda {lam:g}, {regions}: rows {' / '.join(map(str, H.rows))}, nnz(Psi_l) {' / '.join(str(P.nnz) for P in H.Psi)}, longest row "
          f"{np.diff(Psi.indptr).max()}, iterations {it} (recorded {COUNTS[(name, order, lam, regions)]}), residual {res:.2e}, error against LU {err:.2e}")
    assert ok and res <= 1e-9
    assert 2 * it <= boa.budget(order)
    assert abs(it - COUNTS[(name, order, lam, regions)]) <= 2
    assert err <= 1e-6
    assert all(P.shape[0] == Psi.shape[0] for P in H.Psi), "every level keeps the rows of Psi"
    assert all(a.nnz >= c.nnz for a, c in zip(H.Psi, H.Psi[1:])), "the counts do not increase"


@pytest.mark.parametrize("lam,count", [(1e-2, 22), (1e-4, 22)])
def test_restatement_with_weights_that_hold_exact_zeros(oracle, mesh_loader, lam, count):
    A0, b, nd, Psi, rp, ci, blocks, _ = _case(oracle, mesh_loader, "unit_square_16", 1, lam, 4)
    rng = np.random.default_rng(5)
    w = rng.uniform(0.5, 1.5, Psi.shape[0])
    w[rng.uniform(size=len(w)) < 0.3] = 0.0
    assert (w == 0.0).any()
    A = bo.system(rp, ci, blocks, nd, Psi, w)
    x, it, ok, _ = boa.solve(rp, ci, blocks, nd, Psi, b, weights=w)
    err = np.linalg.norm(x - spl.splu(A.tocsc()).solve(b)) / np.linalg.norm(x)
    print(f"lambda {lam:g}: {int((w == 0).sum())} of {len(w)} weights zero, iterations {it} (recorded {count}), error against LU {err:.2e}")
    assert ok and 2 * it <= ba.BUDGET_P1 and err <= 1e-6
    assert abs(it - count) <= 2, "(the zero weights are drawn here, not in the recorded run: within two of it)"


@pytest.mark.parametrize("lam,count", [(1e-2, 22), (1e-4, 18)])
def test_restatement_with_a11_on_the_pattern_and_a_term(oracle, mesh_loader, lam, count):
    _, b, nd, Psi, rp, ci, blocks, _ = _case(oracle, mesh_loader, "unit_square_16", 1, lam, 4)
    m = mesh_loader("unit_square_16")
    obs = br.observed_nodes(m.n_nodes)
    with_a11 = (-br.gram_selection_values(rp, ci, obs, nd),) + tuple(blocks[1:])
    A = bo.system(rp, ci, with_a11, nd, Psi)
    x, it, ok, _ = boa.solve(rp, ci, with_a11, nd, Psi, b)
    err = np.linalg.norm(x - spl.splu(A.tocsc()).solve(b)) / np.linalg.norm(x)
    print(f"lambda {lam:g}: a11 on the pattern plus the term, iterations {it} (recorded {count}), error against LU {err:.2e}")
    assert ok and 2 * it <= ba.BUDGET_P1 and err <= 1e-6
    assert abs(it - count) <= 2


@pytest.mark.parametrize("lam,count", [(1e-2, 20), (1e-4, 16)])
def test_restatement_with_a_pointwise_term(oracle, mesh_loader, lam, count):
    _, _, nd, _, rp, ci, blocks, _ = _case(oracle, mesh_loader, "unit_square_16", 1, lam, 4)
    m = mesh_loader("unit_square_16")
    dofs = oracle.enumerate_dofs(m, 1)[0]
    pts = np.random.default_rng(9).uniform(0.0, 1.0, size=(400, 2))
    Psi = bo.pointwise_psi(oracle, m, 1, dofs, nd, pts)
    b = bo.smoothing_rhs(Psi, lam, nd)
    A = bo.system(rp, ci, blocks, nd, Psi)
    x, it, ok, H = boa.solve(rp, ci, blocks, nd, Psi, b)
    err = np.linalg.norm(x - spl.splu(A.tocsc()).solve(b)) / np.linalg.norm(x)
    print(f"lambda {lam:g}: 400 points, nnz(Psi_l) {' / '.join(str(P.nnz) for P in H.Psi)}, iterations {it} (recorded {count}), error against LU {err:.2e}")
    assert ok and 2 * it <= ba.BUDGET_P1 and err <= 1e-6
    assert abs(it - count) <= 2, "(the points are drawn here, not in the recorded run: within two of it)"


@pytest.mark.parametrize("lam", [1e-2, 1e-4])
def test_control_without_a_coarse_term_does_not_converge(oracle, mesh_loader, lam):
    A, b, nd, Psi, rp, ci, blocks, _ = _case(oracle, mesh_loader, "unit_square_16", 1, lam, 4)
    x, it, ok, _ = boa.solve(rp, ci, blocks, nd, Psi, b, coarse_term=False)
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print(f"lambda {lam:g}: the term on level 0 only: {it} iterations, relative residual {res:.2e}")
    assert not ok and it == 200


def test_entry_point_exists_and_needs_a_device():
    from fdapde_loader import load_package

    capi = load_package().capi
    lib = capi.load()
    assert hasattr(lib, "fdapde_block_obs_amg_levels") and "fdapde_block_obs_amg_levels" in capi.SYMBOLS
    assert hasattr(capi.Context, "block_amg_obs_levels")
    from fdapde_core_amd import workloads

    nodes, cells, bnd = workloads.load_fixture_mesh(os.path.join(ROOT, "tests", "golden", "mesh", "unit_square_16"))
    c = capi.Context(device=None)
    c.mesh_upload(nodes, cells, bnd)
    c.dofs_build(1)
    with pytest.raises(capi.FdapdeError) as e:
        c.block_amg_obs_levels()
    assert e.value.status == capi.ENODEVICE
    c.close()
