"""Reference side of the FDAPDE_SOLVER_BLOCK_AMG tests (tests/test_block_amg_cpu.py, tests/test_gpu_block_amg.py): a numpy / scipy restatement of
csrc/eng_block_amg.hip with the device's rules (the row rules of csrc/amg_rows.h; tests/test_host_amg.py holds their host loops to `pairwise` and `galerkin`) --
  * aggregation: handshake matching on a SCALAR strength matrix on the pattern (the (2,1) block), theta 0.25, ten rounds of which the first three on strong
    couplings only, ties broken by the device's hash of the index pair; two pairwise passes per level, the second on the Galerkin matrix of the first;
  * block Galerkin matrices with P = P_scalar (x) I_2 (the four blocks summed per coarse entry in ascending fine-slot order);
  * cycle: 0.7 D^-1 with D the 2 x 2 diagonal blocks, the coarse correction, 0.7 D^-1; below the finest level two GCR steps around the next level's cycle, always;
  * an exact (SuperLU) last level once 2 n_l <= amg_coarse_rows, or where a level keeps more than 0.8 of its rows;
  * outer: flexible GMRES(50), right-preconditioned, classical Gram-Schmidt twice, on the UNSCALED system, stop rule |b - A x| <= rtol |b| on the true residual.
The restatement numbers the DOFs as the caller does; the device aggregates in its internal order, so its aggregates -- and its counts by a few -- differ."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

THETA, ROUNDS, STRONG_ROUNDS, STALL, OMEGA = 0.25, 10, 3, 0.8, 0.7
RTOL = 1e-10
COARSE_ROWS = 256   # what the GPU tests set `amg_coarse_rows` to: small systems get several levels

# the budgets the GPU test hands over (caps: the restatement must stay under HALF of each, tests/test_block_amg_cpu.py)
BUDGET_P1, BUDGET_P2_2D, BUDGET_P2_3D, LADDER_CAP = 80, 120, 200, 40
# (mesh, order, lambda, advection); a mesh is a fixture name or ("unit_square" | "unit_cube", nx) of meshgen
LU_CASES = [("unit_square_16", 1, 1e-2, False), ("unit_square_16", 1, 1e-4, False), ("unit_square_16", 1, 1e-6, False), ("unit_sphere", 1, 1e-4, False),
            ("unit_square_16", 1, 1e-4, True), (("unit_square", 32), 1, 1e-2, False), (("unit_square", 32), 1, 1e-4, False),
            (("unit_square", 32), 1, 1e-6, False), (("unit_cube", 8), 1, 1e-4, False)]
P2_2D_CASES = [("c_shaped", 2, 1e-4, False), (("unit_square", 16), 2, 1e-4, False)]
P2_3D_CASES = [("unit_sphere", 2, 1e-2, False)]
LADDERS = [([("unit_square", nx) for nx in (16, 32, 64)], 1e-2), ([("unit_square", nx) for nx in (16, 32, 64)], 1e-4),
           ([("unit_cube", nx) for nx in (8, 16)], 1e-4)]


def case_id(case):
    mesh, order, lam, adv = case
    name = mesh if isinstance(mesh, str) else f"{mesh[0]}({mesh[1]})"
    return f"{name}-P{order}-{lam:g}" + ("-advection" if adv else "")


def pair_hash(i, j):
    """amg_pair_hash (csrc/amg_rows.h): the same word from both ends of an edge"""
    lo, hi = np.minimum(i, j).astype(np.uint64), np.maximum(i, j).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = ((hi << np.uint64(32)) | lo) * np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(29)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(32)
    return (z & np.uint64(0xFFFFFFFF)).astype(np.int64)


def _transposed_values(rp, ci, a, n):
    t = sp.csr_matrix((np.arange(1, len(ci) + 1), ci, rp), shape=(n, n)).T.tocsr()
    t.sort_indices()
    assert np.array_equal(t.indptr, rp) and np.array_equal(t.indices, ci), "the pattern is structurally symmetric on every level"
    return a[t.data - 1]


def strength(rp, ci, a, n):
    """amg_strength_row (csrc/amg_rows.h): > 0 a strong coupling, < 0 (minus its strength) a weak one, 0 none"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    off = rows != ci
    s = np.where(off, -(a + _transposed_values(rp, ci, a, n)), 0.0)
    mneg = np.maximum.reduceat(np.where(off, s, 0.0), rp[:-1]).clip(min=0.0)
    mabs = np.maximum.reduceat(np.abs(s), rp[:-1])
    neg = (mneg > 0.0)[rows]
    thr = THETA * np.where(neg, mneg[rows], mabs[rows])
    v = np.where(neg, s, np.abs(s))
    return np.where(off & (v > 0.0), np.where(v >= thr, v, -v), 0.0), rows


def pairwise(rp, ci, a, n):
    """one handshake pass -> (agg, number of aggregates)"""
    sw, rows = strength(rp, ci, a, n)
    h = pair_hash(rows, ci)
    mate = np.full(n, -1)
    for rnd in range(ROUNDS):
        w = np.abs(sw) if rnd >= STRONG_ROUNDS else sw
        ok = (w > 0.0) & (rows != ci) & (mate[rows] < 0) & (mate[ci] < 0)
        k = np.flatnonzero(ok)
        order = k[np.lexsort((-ci[k], h[k], w[k], rows[k]))]   # per row ascending (w, hash, -j): the best candidate comes last
        prop = np.full(n, -1)
        prop[rows[order]] = ci[order]                         # (later writes win)
        i = np.flatnonzero(prop >= 0)
        i = i[prop[prop[i]] == i]
        mate[i] = prop[i]
    lead = (mate < 0) | (mate > np.arange(n))
    ident = np.cumsum(lead) - lead
    return np.where(lead, ident, ident[np.where(mate >= 0, mate, 0)]), int(lead.sum())


def galerkin(rp, ci, vals, agg, nc, n):
    """P^T A P of piecewise-constant P for every value array in `vals`: (agg(i) nc + agg(j)) keys, sums in ascending fine-slot order"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    keys = agg[rows].astype(np.int64) * nc + agg[ci]
    uniq, inv = np.unique(keys, return_inverse=True)
    out = []
    for v in vals:
        s = np.zeros(len(uniq))
        np.add.at(s, inv, v)
        out.append(s)
    rp_c = np.zeros(nc + 1, dtype=np.int64)
    np.add.at(rp_c, uniq // nc + 1, 1)
    return np.cumsum(rp_c), (uniq % nc).astype(np.int64), out


def _interleaved(rp, ci, blocks, n):
    E = [np.array([[1.0, 0.0], [0.0, 0.0]]), np.array([[0.0, 1.0], [0.0, 0.0]]), np.array([[0.0, 0.0], [1.0, 0.0]]), np.array([[0.0, 0.0], [0.0, 1.0]])]
    return sum(sp.kron(sp.csr_matrix((b, ci, rp), shape=(n, n)), e, format="csr") for b, e in zip(blocks, E)).tocsr()


def _diag_inverse(rp, ci, blocks, n):
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.flatnonzero(rows == ci)
    assert len(d) == n
    a, b, c, e = (blk[d] for blk in blocks)
    det = a * e - b * c
    mx = np.max(np.abs([a, b, c, e]), axis=0)
    assert np.all(np.abs(det) > 1e-14 * mx * mx), "a singular diagonal block: the device refuses (level 0) or ends the hierarchy one level above"
    return _interleaved(np.arange(n + 1), np.arange(n), [e / det, -b / det, -c / det, a / det], n)


class Hierarchy:
    """levels of (A interleaved, D^-1, P to the next level); rows[l] = 2 n_l"""

    def __init__(self, rp, ci, blocks, n, coarse_rows=COARSE_ROWS, strength_block=2):
        rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
        blocks = [np.zeros(len(ci)) if b is None else np.asarray(b, dtype=float) for b in blocks]
        s = blocks[strength_block]
        self.A, self.Dinv, self.P, self.rows = [], [], [], []
        while True:
            self.A.append(_interleaved(rp, ci, blocks, n))
            self.rows.append(2 * n)
            if 2 * n <= coarse_rows:
                break
            agg1, n1 = pairwise(rp, ci, s, n)
            rp1, ci1, v1 = galerkin(rp, ci, [s] + blocks, agg1, n1, n)
            agg2, n2 = pairwise(rp1, ci1, v1[0], n1)
            rp2, ci2, v2 = galerkin(rp1, ci1, v1, agg2, n2, n1)
            if n2 > STALL * n and 2 * n2 > coarse_rows:
                assert 2 * n <= 8192, "coarsening stalled above the dense limit: the device answers FDAPDE_EUNSUPPORTED"
                break
            agg = agg2[agg1]
            self.Dinv.append(_diag_inverse(rp, ci, blocks, n))
            self.P.append(sp.kron(sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, n2)), sp.identity(2), format="csr"))
            rp, ci, s, blocks, n = rp2, ci2, v2[0], v2[1:], n2
        self.last = spl.splu(self.A[-1].tocsc())

    def cycle(self, l, r):
        A, Dinv, P = self.A[l], self.Dinv[l], self.P[l]
        zt = OMEGA * (Dinv @ r)
        z = zt + P @ self.correction(l + 1, P.T @ (r - A @ zt))
        return z + OMEGA * (Dinv @ (r - A @ z))

    def correction(self, m, b):
        """the exact last level; elsewhere two GCR steps around the cycle (k_amg_coef's arithmetic: a step that cannot be taken contributes nothing)"""
        if m + 1 == len(self.A):
            return self.last.solve(b)
        A = self.A[m]
        c = self.cycle(m, b)
        v = A @ c
        rho1 = v @ v
        a1 = (v @ b) / rho1 if rho1 > 0.0 else 0.0
        rt = b - a1 * v
        d = self.cycle(m, rt)
        w = A @ d
        gamma = v @ w
        rho2 = w @ w - gamma * gamma / rho1 if rho1 > 0.0 else 0.0
        cd = (w @ rt) / rho2 if rho2 > 0.0 else 0.0
        cc = a1 - (cd * gamma / rho1 if rho1 > 0.0 else 0.0)
        return cc * c + cd * d

    def precondition(self, v):
        return self.last.solve(v) if len(self.A) == 1 else self.cycle(0, v)


def fgmres(A, b, precondition, rtol=RTOL, maxit=200, restart=50):
    """flexible GMRES(restart), right-preconditioned, Gram-Schmidt twice; the true residual at every restart decides -> (x, iterations, converged)"""
    n = len(b)
    x = np.zeros(n)
    bb = b @ b
    r, it = b.copy(), 0
    rr = bb
    converged = not bb > 0.0
    while not converged and it < maxit:
        beta = np.sqrt(rr)
        V, Z = np.zeros((restart + 1, n)), np.zeros((restart, n))
        H = np.zeros((restart + 1, restart))
        cs, sn, g = np.zeros(restart), np.zeros(restart), np.zeros(restart + 1)
        V[0], g[0] = r / beta, beta
        k = 0
        while k < restart and it < maxit:
            Z[k] = precondition(V[k])
            w = A @ Z[k]
            for _ in range(2):
                h = V[:k + 1] @ w
                w = w - V[:k + 1].T @ h
                H[:k + 1, k] += h
            hn = np.linalg.norm(w)
            H[k + 1, k] = hn
            for i in range(k):
                H[i, k], H[i + 1, k] = cs[i] * H[i, k] + sn[i] * H[i + 1, k], -sn[i] * H[i, k] + cs[i] * H[i + 1, k]
            d = np.hypot(H[k, k], H[k + 1, k])
            cs[k], sn[k] = H[k, k] / d, H[k + 1, k] / d
            H[k, k], H[k + 1, k] = d, 0.0
            g[k + 1], g[k] = -sn[k] * g[k], cs[k] * g[k]
            k, it = k + 1, it + 1
            if g[k] * g[k] <= rtol * rtol * bb or not hn > 1e-300:
                break
            V[k] = w / hn
        y = np.linalg.solve(np.triu(H[:k, :k]), g[:k])
        x = x + Z[:k].T @ y
        r = b - A @ x
        rr = r @ r
        converged = rr <= rtol * rtol * bb
    return x, it, converged


def stacked_to_interleaved(n):
    """perm with z_interleaved = z_stacked[perm]"""
    return np.arange(2 * n).reshape(2, n).T.reshape(-1)


def solve(rp, ci, blocks, n, b_stacked, rtol=RTOL, maxit=200, coarse_rows=COARSE_ROWS):
    """the restatement on the four blocks (value arrays on the pattern) -> (x stacked, iterations, converged, rows per level)"""
    H = Hierarchy(rp, ci, blocks, n, coarse_rows)
    perm = stacked_to_interleaved(n)
    x, it, ok = fgmres(H.A[0], np.asarray(b_stacked, dtype=float)[perm], H.precondition, rtol, maxit)
    out = np.empty(2 * n)
    out[perm] = x
    return out, it, ok, H.rows
