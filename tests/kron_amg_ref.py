"""Reference side of the FDAPDE_SOLVER_KRON_AMG tests (tests/test_kron_amg_cpu.py, tests/test_gpu_kron_amg.py): a numpy / scipy restatement of
csrc/eng_kron_amg.hip built on tests/block_amg_ref.py's `pairwise` / `galerkin` / `fgmres` (the device's row rules) --
  * A = sum_sigma T_sigma (x) S_sigma with the terms merged as fdapde_kron_compute merges them (terms that hand over the same array share a factor, their T
    summed);
  * aggregation on a SCALAR strength matrix on the pattern: -sum_sigma |T_sigma|_F |S_sigma[i,j]|, or the spatial factor of a named term as given;
  * P = P_scalar (x) I_q: every level is a Kronecker sum with the same T_sigma, the spatial factors summed per coarse entry in ascending fine-slot order;
  * cycle: 0.7 D^-1 with D the q x q diagonal blocks, the coarse correction, 0.7 D^-1; below the finest level two GCR steps around the next level's cycle;
  * an exact (SuperLU) last level once q n_l <= amg_coarse_rows, or where a level keeps more than 0.8 of its rows;
  * outer: flexible GMRES(50) on the UNSCALED system, stop rule |b - A x| <= rtol |b| on the true residual.
Vectors here are interleaved per DOF (unknown r of DOF i at i q + r) as on the device; `solve` takes and returns the reference's Kronecker order (r n + i).
The restatement numbers the DOFs as the caller does; the device aggregates in its internal order, so its aggregates -- and its counts by a few -- differ."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import block_amg_ref as ar
import kron_ref as kr

RTOL = ar.RTOL
COARSE_ROWS = ar.COARSE_ROWS   # what the GPU tests set `amg_coarse_rows` to: 289-DOF systems get several levels
STALL, OMEGA = ar.STALL, ar.OMEGA

# the budgets the GPU test hands over (caps: the restatement must stay under HALF of each, tests/test_kron_amg_cpu.py)
BUDGET_P1, BUDGET_P2_2D, LADDER_CAP = 80, 160, 40
# ("spacetime", mesh, order, m, lambda = lambda_T) | ("parabolic", mesh, order, q, dt) | ("dense_t", mesh, order, q, dt); a mesh is a fixture name or
# ("unit_square" | "unit_cube", nx) of meshgen
SPACETIME_CASES = [("spacetime",) + c for c in kr.SOLVE_CASES]
PARABOLIC_CASES = [("parabolic", "unit_square_16", 1, 10, 0.01), ("parabolic", "unit_sphere", 1, 5, 0.1)]
# the widths that can go wrong, on unit_square_16 P1 (289 rows: a partly empty last workgroup): q = 1 runs as a team of two with one idle lane, q = 33 as a
# team of 64 with 31; the dense T keeps the band skip from being the only path
WIDTH_CASES = ([("parabolic", "unit_square_16", 1, q, 0.01) for q in (1, 2, 3, 5, 33)] + [("spacetime", "unit_square_16", 1, q // 2, 1e-4) for q in (10, 16, 64)] +
               [("dense_t", "unit_square_16", 1, 5, 0.01)])
LADDERS = [[("spacetime", ("unit_square", nx), 1, 3, 1e-4) for nx in (16, 32, 64)], [("spacetime", ("unit_cube", nx), 1, 3, 1e-4) for nx in (8, 16)]]


def budget(case):
    return BUDGET_P2_2D if case[2] == 2 else BUDGET_P1


def case_id(case):
    kind, mesh, order, k, p = case
    name = mesh if isinstance(mesh, str) else f"{mesh[0]}({mesh[1]})"
    return f"{kind}-{name}-P{order}-{k}-{p:g}"


def parabolic_terms(R1, R0, q, dt):
    """the monolithic implicit-Euler system D_t (x) M + I (x) K of q steps: D_t lower bidiagonal (1 / dt, -1 / dt), non-symmetric"""
    Dt = (np.eye(q) - np.eye(q, k=-1)) / dt
    return [(Dt, np.asarray(R0, dtype=float)), (np.eye(q), np.asarray(R1, dtype=float))]


def dense_t_terms(R1, R0, q, dt):
    """T (x) M + I (x) K with a DENSE, diagonally dominant T: no band to skip"""
    rng = np.random.default_rng(77)
    T = (np.eye(q) + 0.1 * rng.standard_normal((q, q))) / dt
    assert np.all(T != 0.0)
    return [(T, np.asarray(R0, dtype=float)), (np.eye(q), np.asarray(R1, dtype=float))]


def system(case, rp, ci, R1, R0, obs):
    """-> (terms, q, b in the Kronecker order) of a case on the matrices of its space"""
    kind, _, _, k, p = case
    n = len(rp) - 1
    if kind == "spacetime":
        return kr.spacetime_terms(rp, ci, R1, R0, obs, p, p, k), 2 * k, kr.spacetime_rhs(obs, p, n, k)
    terms = parabolic_terms(R1, R0, k, p) if kind == "parabolic" else dense_t_terms(R1, R0, k, p)
    return terms, k, np.random.default_rng(5).standard_normal(k * n)


def merge(terms):
    """-> (T_sigma, S_sigma, the factor every term went into): terms whose S are the same array share a factor"""
    Ts, Ss, where = [], [], []
    for T, S in terms:
        for sg, have in enumerate(Ss):
            if have is S:
                Ts[sg] = Ts[sg] + np.asarray(T, dtype=float)
                where.append(sg)
                break
        else:
            Ts.append(np.array(T, dtype=float))
            Ss.append(S)
            where.append(len(Ss) - 1)
    return Ts, [np.asarray(S, dtype=float) for S in Ss], where


def strength_values(Ts, Ss, where, term=-1):
    """the scalar strength matrix on the pattern: by magnitude (the Frobenius norms weigh the factors), or the spatial factor of term `term` as given"""
    if term >= 0:
        return Ss[where[term]].copy()
    s = np.zeros(len(Ss[0]))
    for T, S in zip(Ts, Ss):
        s += np.sqrt(np.sum(T * T)) * np.abs(S)
    return -s


def _interleaved(rp, ci, Ts, Ss, n):
    return sum(sp.kron(sp.csr_matrix((S, ci, rp), shape=(n, n)), sp.csr_matrix(T), format="csr") for T, S in zip(Ts, Ss)).tocsr()


def _diag_inverse(rp, ci, Ts, Ss, n, q):
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.flatnonzero(rows == ci)
    assert len(d) == n
    D = sum(S[d][:, None, None] * T[None, :, :] for T, S in zip(Ts, Ss))
    assert np.all(np.linalg.cond(D) < 1e13), "a singular diagonal block: the device refuses (level 0) or ends the hierarchy one level above"
    Di = np.linalg.inv(D)
    r = (q * np.arange(n)[:, None, None] + np.arange(q)[None, :, None]) + np.zeros((1, 1, q), dtype=np.int64)
    c = (q * np.arange(n)[:, None, None] + np.arange(q)[None, None, :]) + np.zeros((1, q, 1), dtype=np.int64)
    return sp.csr_matrix((Di.reshape(-1), (r.reshape(-1), c.reshape(-1))), shape=(q * n, q * n))


class Hierarchy(ar.Hierarchy):
    """levels of (A interleaved, D^-1, P to the next level); rows[l] = q n_l.  cycle / correction / precondition are the block form's"""

    def __init__(self, rp, ci, terms, n, coarse_rows=COARSE_ROWS, term=-1):
        rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
        Ts, Ss, where = merge(terms)
        q = Ts[0].shape[0]
        s = strength_values(Ts, Ss, where, term)
        self.A, self.Dinv, self.P, self.rows, self.aggs = [], [], [], [], []
        while True:
            self.A.append(_interleaved(rp, ci, Ts, Ss, n))
            self.rows.append(q * n)
            if q * n <= coarse_rows:
                break
            agg1, n1 = ar.pairwise(rp, ci, s, n)
            rp1, ci1, v1 = ar.galerkin(rp, ci, [s] + Ss, agg1, n1, n)
            agg2, n2 = ar.pairwise(rp1, ci1, v1[0], n1)
            rp2, ci2, v2 = ar.galerkin(rp1, ci1, v1, agg2, n2, n1)
            if n2 > STALL * n and q * n2 > coarse_rows:
                assert q * n <= 8192, "coarsening stalled above the dense limit: the device answers FDAPDE_EUNSUPPORTED"
                break
            agg = agg2[agg1]
            self.aggs.append(agg)
            self.Dinv.append(_diag_inverse(rp, ci, Ts, Ss, n, q))
            self.P.append(sp.kron(sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, n2)), sp.identity(q), format="csr"))
            rp, ci, s, Ss, n = rp2, ci2, v2[0], v2[1:], n2
        self.last = spl.splu(self.A[-1].tocsc())


def kron_to_interleaved(n, q):
    """perm with z_interleaved = z_kron[perm]"""
    return np.arange(q * n).reshape(q, n).T.reshape(-1)


def solve(rp, ci, terms, n, b_kron, rtol=RTOL, maxit=200, coarse_rows=COARSE_ROWS, term=-1):
    """the restatement on the terms [(T, S_values)] -> (x in the Kronecker order, iterations, converged, rows per level)"""
    H = Hierarchy(rp, ci, terms, n, coarse_rows, term)
    q = H.rows[0] // n
    perm = kron_to_interleaved(n, q)
    x, it, ok = ar.fgmres(H.A[0], np.asarray(b_kron, dtype=float)[perm], H.precondition, rtol, maxit)
    out = np.empty(q * n)
    out[perm] = x
    return out, it, ok, H.rows
