"""Reference side of the absorption tests (tests/test_amg_absorb_cpu.py, tests/test_gpu_amg_absorb.py): a numpy / scipy restatement of the multilevel set-up
with the knob `amg_absorb`, on top of tests/block_amg_ref.py --
  * the handshake matching of block_amg_ref.pairwise, kept as `mate`, and the ABSORPTION pass (amg_absorb_row, csrc/amg_rows.h; k_amg_absorb of csrc/eng_amg.hip): every row the ten rounds
    left single looks along its row at the entries with a coupling (strong or weak) to a PAIRED row, takes the one with the largest |coupling| (ties: the
    larger hash of the index pair, then the smaller index) and joins that pair's aggregate; a single without a paired neighbour stays a singleton;
  * the SCALAR K-cycle of csrc/eng_amg.hip: damped Jacobi 1.5 / lambda_max(D^-1 A) by 15 power steps, the coarse correction, damped Jacobi;
    below the finest level two flexible-CG steps around the next level's cycle, always; an exact (SuperLU) last level once n_l <= amg_coarse_rows or where a
    level of at most 8 192 rows keeps more than 0.8 of its rows; block_amg_ref.fgmres outside;
  * the block hierarchy of block_amg_ref.Hierarchy with the same passes (its cycle and its GCR steps are inherited unchanged).
A hierarchy that stalls above its dense limit raises Stalled: the device answers FDAPDE_EUNSUPPORTED (amg_absorb 0) or builds again with absorption (2).
The restatement numbers the rows as the caller does; the device aggregates in its internal order, so its aggregates -- and its counts by a few -- differ."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import block_amg_ref as ar

COARSE_ROWS = 256          # what the GPU test sets `amg_coarse_rows` to for the scalar cases
KEEP = 0.35                # every level of a hierarchy built with absorption keeps at most this share of the rows above it (the restatement: <= 0.23)
SCALAR_DENSE_LIMIT = 8192  # kDenseMaxRows
# iteration caps the GPU test hands over: conditions with a factor 2 to spare over this restatement (tests/test_amg_absorb_cpu.py holds it to HALF of each)
CAP_3D, CAP_2D, CAP_BLOCK = 40, 50, ar.BUDGET_P1
LADDER_3D = [("unit_cube", nx) for nx in (8, 16, 32)]
LADDER_2D = [("unit_square", nx) for nx in (32, 64, 128)]
# the smallest refusal: the block system on unit_cube(16), lambda 1e-4, amg_coarse_rows 32, dense_rows 48
BLOCK_CASE, BLOCK_COARSE_ROWS, BLOCK_DENSE_ROWS = (("unit_cube", 16), 1, 1e-4, False), 32, 48


def ladder_forcing(n_quadrature):
    """the forcing of the capped scalar cases at the quadrature nodes, on both sides: seeded white noise.  The caps are twice what this restatement needs for
    such a load (2-D 22 / 22 / 23, 3-D 14 / 17 / 18 with absorption); a smooth load costs it two or three iterations more (1 + sin(3 x) y: 24 / 24 / 26 and
    14 / 18 / 20), the same two or three with and without absorption"""
    return np.random.default_rng(20).standard_normal(n_quadrature)


class Stalled(Exception):
    """coarsening stalled above the dense limit; .rows: the rows of the level that kept more than 0.8 of them"""

    def __init__(self, rows):
        super().__init__(f"coarsening stalled at a level of {rows} rows")
        self.rows = rows


def matching(rp, ci, a, n):
    """the ten handshake rounds of block_amg_ref.pairwise -> (mate, strength per entry, row of every entry, hash of every entry)"""
    sw, rows = ar.strength(rp, ci, a, n)
    h = ar.pair_hash(rows, ci)
    mate = np.full(n, -1)
    for rnd in range(ar.ROUNDS):
        w = np.abs(sw) if rnd >= ar.STRONG_ROUNDS else sw
        k = np.flatnonzero((w > 0.0) & (rows != ci) & (mate[rows] < 0) & (mate[ci] < 0))
        order = k[np.lexsort((-ci[k], h[k], w[k], rows[k]))]
        prop = np.full(n, -1)
        prop[rows[order]] = ci[order]
        i = np.flatnonzero(prop >= 0)
        i = i[prop[prop[i]] == i]
        mate[i] = prop[i]
    return mate, sw, rows, h


def absorb(ci, sw, rows, h, mate):
    """amg_absorb_row (csrc/amg_rows.h) for every row: the paired row a single joins, -1 for none"""
    w = np.abs(sw)
    k = np.flatnonzero((w > 0.0) & (rows != ci) & (mate[rows] < 0) & (mate[ci] >= 0))
    order = k[np.lexsort((-ci[k], h[k], w[k], rows[k]))]   # per row ascending (w, hash, -j): the best candidate comes last
    host = np.full(len(mate), -1)
    host[rows[order]] = ci[order]
    return host


def pairwise(rp, ci, a, n, absorbing):
    """one pass -> (agg, number of aggregates, rows left single by the matching); without absorption this is block_amg_ref.pairwise"""
    mate, sw, rows, h = matching(rp, ci, a, n)
    host = absorb(ci, sw, rows, h, mate) if absorbing else np.full(n, -1)
    idx = np.arange(n)
    lead = (host < 0) & ((mate < 0) | (mate > idx))
    ident = np.cumsum(lead) - lead
    hs = np.where(host >= 0, host, 0)
    of_host = ident[np.minimum(hs, np.where(mate[hs] >= 0, mate[hs], 0))]
    agg = np.where(host >= 0, of_host, np.where(lead, ident, ident[np.where(mate >= 0, mate, 0)]))
    return agg, int(lead.sum()), int((mate < 0).sum())


def _two_passes(rp, ci, vals, n, absorbing):
    """both passes of a level on vals[0] -> (row -> aggregate, n2, coarse rowptr, colidx, coarse value arrays, singles of pass 1 and 2)"""
    agg1, n1, s1 = pairwise(rp, ci, vals[0], n, absorbing)
    rp1, ci1, v1 = ar.galerkin(rp, ci, vals, agg1, n1, n)
    agg2, n2, s2 = pairwise(rp1, ci1, v1[0], n1, absorbing)
    rp2, ci2, v2 = ar.galerkin(rp1, ci1, v1, agg2, n2, n1)
    return agg2[agg1], n2, rp2, ci2, v2, (s1, s2)


def hashvec(n):
    """k_amg_hashvec: the power iteration's fixed start"""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(11)).astype(float) * (2.0 / 9007199254740992.0) - 1.0


class ScalarHierarchy:
    """levels of (A, om D^-1, P to the next level) of a matrix without excluded rows (the interior block of a Dirichlet problem); rows[l] = n_l"""

    def __init__(self, A, absorbing, coarse_rows=COARSE_ROWS, dense_limit=SCALAR_DENSE_LIMIT):
        A = sp.csr_matrix(A)
        A.sort_indices()
        rp, ci, a, n = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(float), A.shape[0]
        self.A, self.omd, self.P, self.rows, self.nnz, self.singles = [], [], [], [], [], []
        while True:
            self.A.append(sp.csr_matrix((a, ci, rp), shape=(n, n)))
            self.rows.append(n)
            self.nnz.append(len(ci))
            if n <= coarse_rows:
                break
            agg, n2, rp2, ci2, v2, singles = _two_passes(rp, ci, [a], n, absorbing)
            if n2 > ar.STALL * n and n2 > coarse_rows:
                if n > dense_limit:
                    raise Stalled(n)
                break
            self.singles.append(singles)
            self.P.append(sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, n2)))
            rp, ci, a, n = rp2, ci2, v2[0], n2
        for A_l in self.A[:-1]:
            dinv = 1.0 / A_l.diagonal()
            x, lam = hashvec(A_l.shape[0]), 0.0
            for _ in range(15):
                y = dinv * (A_l @ x)
                h0, h1 = x @ x, y @ y
                lam = np.sqrt(h1 / h0)
                x = y / np.sqrt(h1)
            self.omd.append(1.5 / lam * dinv)
        self.last = spl.splu(self.A[-1].tocsc())

    def cycle(self, l, r):
        A, omd, P = self.A[l], self.omd[l], self.P[l]
        zt = omd * r
        z = zt + P @ self.correction(l + 1, P.T @ (r - A @ zt))
        return z + omd * (r - A @ z)

    def correction(self, m, b):
        """the exact last level; elsewhere two flexible-CG steps around the cycle (k_amg_coef: a step that cannot be taken contributes nothing)"""
        if m + 1 == len(self.A):
            return self.last.solve(b)
        A = self.A[m]
        c = self.cycle(m, b)
        v = A @ c
        rho1 = c @ v
        a1 = (c @ b) / rho1 if rho1 > 0.0 else 0.0
        rt = b - a1 * v
        d = self.cycle(m, rt)
        w = A @ d
        gamma = d @ v
        rho2 = d @ w - gamma * gamma / rho1 if rho1 > 0.0 else 0.0
        cd = (d @ rt) / rho2 if rho2 > 0.0 else 0.0
        cc = a1 - (cd * gamma / rho1 if rho1 > 0.0 else 0.0)
        return cc * c + cd * d

    def precondition(self, v):
        return self.last.solve(v) if len(self.A) == 1 else self.cycle(0, v)


def scalar_solve(A, b, absorbing, rtol=ar.RTOL, maxit=200, coarse_rows=COARSE_ROWS):
    """-> (x, iterations, converged, hierarchy)"""
    H = ScalarHierarchy(A, absorbing, coarse_rows)
    x, it, ok = ar.fgmres(H.A[0], np.asarray(b, dtype=float), H.precondition, rtol, maxit)
    return x, it, ok, H


class BlockHierarchy(ar.Hierarchy):
    """block_amg_ref.Hierarchy with the passes above and a dense limit of its own (`dense_rows`); cycle, correction and precondition are inherited"""

    def __init__(self, rp, ci, blocks, n, absorbing, coarse_rows, dense_rows=8192, strength_block=2):
        rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
        blocks = [np.zeros(len(ci)) if b is None else np.asarray(b, dtype=float) for b in blocks]
        s = blocks[strength_block]
        self.A, self.Dinv, self.P, self.rows = [], [], [], []
        while True:
            self.A.append(ar._interleaved(rp, ci, blocks, n))
            self.rows.append(2 * n)
            if 2 * n <= coarse_rows:
                break
            agg, n2, rp2, ci2, v2, _ = _two_passes(rp, ci, [s] + blocks, n, absorbing)
            if n2 > ar.STALL * n and 2 * n2 > coarse_rows:
                if 2 * n > dense_rows:
                    raise Stalled(2 * n)
                break
            self.Dinv.append(ar._diag_inverse(rp, ci, blocks, n))
            self.P.append(sp.kron(sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, n2)), sp.identity(2), format="csr"))
            rp, ci, s, blocks, n = rp2, ci2, v2[0], v2[1:], n2
        self.last = spl.splu(self.A[-1].tocsc())


def block_solve(rp, ci, blocks, n, b_stacked, absorbing, coarse_rows, dense_rows=8192, rtol=ar.RTOL, maxit=200):
    """-> (x stacked, iterations, converged, rows per level as 2 n_l)"""
    H = BlockHierarchy(rp, ci, blocks, n, absorbing, coarse_rows, dense_rows)
    perm = ar.stacked_to_interleaved(n)
    x, it, ok = ar.fgmres(H.A[0], np.asarray(b_stacked, dtype=float)[perm], H.precondition, rtol, maxit)
    out = np.empty(2 * n)
    out[perm] = x
    return out, it, ok, H.rows


def kept(rows):
    """share of its rows every level below the first keeps"""
    return [rows[l + 1] / rows[l] for l in range(len(rows) - 1)]
