"""The reference side of the k-th iterate tests of tests/test_gpu_block_obs_amg.py without a device (tests/block_obs_amg_iter_ref.py).

Every case is rebuilt from the ORACLE's matrices and Psi, with aggregates from the restatement's passes in the caller's numbering (block_amg_ref: any valid
aggregates serve -- the device hands its own out), and the float64 twin of the scheme is measured against the extended-precision reference in the unit of the
GPU test's bounds: r_cpu(k) = max_i |x_k^f64 - x_k^ld|_i / (u s_i) over the entries with s_i > 0 with the same ratio of the residual (the entrywise unit),
and per field max |x_k^f64 - x_k^ld| / (u max s) (the unit of tests/test_gpu_block_iterates.py's multilevel stage):
  * r_cpu(k) per case and k is written to profiles/block_obs_amg_iterates.txt, both units;
  * the constants committed in block_obs_amg_iter_ref (c(k) = 4 r_cpu(k) rounded up to a power of two) must still fit.  The per-field
    constants stay below 2^12 as block_iter_ref's do.  The entrywise ones do not at k = 1, 2: the coarse solve spreads its rounding over the whole domain, and
    an entry where the first correction changes sign has a scale s_i far below the field's -- there the per-field bound is the one with teeth.
The reference checks itself: Psi_l of every level is Psi P_0 ... P_{l-1} as scipy forms it, the last level's dense matrix is the Galerkin product of the whole
matrix, and at k = 40 the reference agrees with SuperLU on the explicit system to 1e-9."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import block_amg_ref as ba
import block_iter_ref as ir
import block_obs_amg_iter_ref as oir
import block_obs_ref as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "block_obs_amg_iterates.txt")
HEADER = ["# k-th iterates of FDAPDE_SOLVER_BLOCK_AMG with the factored data term carried (knob block_amg_obs) against the extended-precision reference",
          "# (tests/block_obs_amg_iter_ref.py): worst ratios per case and k.  Unit: max_i |x - x_ref|_i / (u s_i) over s_i > 0, and |relres - rho_k| / (u || |A| s || / ||b||);",
          "# u = 2^-53.  cpu lines: the float64 numpy twin, rewritten by tests/test_block_obs_amg_iter_cpu.py; gpu lines: an MI355X, appended by",
          "# tests/test_gpu_block_obs_amg.py under FDAPDE_BLOCK_OBS_AMG_PROFILE."]
STAGES = ("cpu block_obs_amg ", "cpu block_obs_amg_field ")
_built = {}


def _case(oracle, mesh_loader, name):
    if name not in _built:
        fixture, order, lam, regions = oir.CASES[name]
        A, b, nd, Psi, (rp, ci, blocks) = bo.oracle_case(oracle, mesh_loader, fixture, order, lam, regions)
        rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
        H = ba.Hierarchy(rp, ci, blocks, nd, oir.COARSE_ROWS)
        aggs = [np.asarray(P.tocsr()[::2].indices // 2, dtype=np.int64) for P in H.P]
        _built[name] = (A, b, nd, Psi, rp, ci, blocks, aggs)
    return _built[name]


def test_constants_fit(oracle, mesh_loader):
    levels, runs, checks = {}, {}, []

    def run(name):
        if name not in runs:
            A, b, nd, Psi, rp, ci, blocks, aggs = _case(oracle, mesh_loader, name)
            K = max(oir.KS)
            runs[name] = (oir.iterates(rp, ci, blocks, nd, aggs, Psi, b, K), oir.iterates_float64(rp, ci, blocks, nd, aggs, Psi, b, K))
            levels[name] = len(aggs) + 1
        return runs[name]

    units = {"block_obs_amg": (lambda c, it: max(ir.entry_ratio(c.x.astype(np.float64), it), ir.relres_ratio(c.rho, it)), oir.C_OBS_AMG, None),
             "block_obs_amg_field": (lambda c, it: max(ir.field_ratios(c.x.astype(np.float64), it)), oir.C_OBS_AMG_FIELD, ir.C_MAX)}
    for stage, (unit, constants, cap) in units.items():
        worst, lines = {}, []
        for name in oir.CASES:
            ratios = {it.k: unit(c, it) for it, c in zip(*run(name))}
            for k in oir.KS:
                worst[k] = max(worst.get(k, 0.0), ratios[k])
            lines.append(f"cpu {stage} {name}: " + " ".join(f"{k}={ratios[k]:.3g}" for k in oir.KS))
        lines.append(f"cpu {stage} c(k) = 4 r_cpu(k) rounded up to a power of two: " + " ".join(f"{k}={ir.constant_for(worst[k]):g}" for k in sorted(worst)))
        print("\n".join(lines))
        ir.write_profile(PROFILE, HEADER, STAGES, f"cpu {stage} ", lines)
        checks.append((stage, worst, constants, cap))
    for stage, worst, constants, cap in checks:   # (both tables are written before the verdict)
        assert sorted(worst) == sorted(constants)
        for k in sorted(worst):
            assert 4.0 * worst[k] <= constants[k], (stage, k, worst[k], constants[k])   # (r_cpu still fits c / 4)
            assert cap is None or constants[k] <= cap
    assert levels["sq-p2-4x4"] >= 3 and levels["sphere-p1-2"] >= 3, "a level with GCR steps: the term inside y = A x"


@pytest.mark.parametrize("name", ["sq-p1-4x4", "sq-p2-4x4"])
def test_the_reference_checks_itself(oracle, mesh_loader, name):
    A, b, nd, Psi, rp, ci, blocks, aggs = _case(oracle, mesh_loader, name)
    H = oir.TermHierarchy(rp, ci, blocks, nd, aggs, Psi)
    # Psi_l against scipy's product
    P = Psi.tocsr()
    for l, agg in enumerate(aggs):
        nc = int(agg.max()) + 1
        P = (P @ sp.csr_matrix((np.ones(len(agg)), (np.arange(len(agg)), agg)), shape=(len(agg), nc))).tocsr()
        P.sort_indices()
        ip, idx, v = H.A[l + 1].term.P
        assert np.array_equal(ip, P.indptr) and np.array_equal(idx, P.indices)
        assert np.abs(v.astype(float) - P.data).max() <= 1e-14 * np.abs(P.data).max()
    assert H.psi_nnz[0] == Psi.nnz and all(a >= c for a, c in zip(H.psi_nnz, H.psi_nnz[1:]))
    # the last level's matrix is the Galerkin product of the explicit system (interleaved)
    perm = ba.stacked_to_interleaved(nd)
    M = A.tocsr()[perm][:, perm]
    for agg in aggs:
        nc = int(agg.max()) + 1
        Pb = sp.kron(sp.csr_matrix((np.ones(len(agg)), (np.arange(len(agg)), agg)), shape=(len(agg), nc)), sp.identity(2), format="csr")
        M = (Pb.T @ M @ Pb).tocsr()
    last = H.A[-1].dense().astype(float)
    assert np.abs(last - M.toarray()).max() <= 1e-13 * np.abs(last).max()
    # ... and the scheme converges to the solution
    its = ir.fgmres_iterates(H, b, 40)
    x_lu = spl.splu(A.tocsc()).solve(b)
    err = np.linalg.norm(its[-1].x.astype(float) - x_lu) / np.linalg.norm(x_lu)
    print(f"{name}: levels {[2 * r for r in H.rows]}, nnz(Psi_l) {H.psi_nnz}, |x_40 - x_lu| / |x_lu| = {err:.2e}, rho_40 = {its[-1].rho:.2e}")
    assert err <= 1e-9
