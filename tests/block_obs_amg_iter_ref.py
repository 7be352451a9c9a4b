"""Extended-precision reference for the k-th iterate of FDAPDE_SOLVER_BLOCK_AMG with the factored data term carried through the hierarchy (knob block_amg_obs;
tests/test_block_obs_amg_iter_cpu.py, tests/test_gpu_block_obs_amg.py): tests/block_iter_ref.py's scheme -- its Hierarchy, ObsTerm and the scale s, imported --
with a level being the pair (block CSR matrix on the level's pattern, Psi_l): the level's matrix is A_l + scale [Psi_l^T W Psi_l, 0; 0, 0], the term applied as
its two rectangular products, its diagonal share in D_l^-1, the last level's dense matrix with the term merged in.  The aggregates are DATA (the device's,
fdapde_amg_aggregates); Psi_{l+1} = Psi_l P_s: the same rows, the columns through the aggregates, equal columns summed in ascending fine-column order.

With the aggregates fixed, iterate k is ONE vector in exact arithmetic.  `TermHierarchy(..., dt=np.float64, like_device=True)` is the float64 twin the way the
device runs it; it measures the constants, it is never the thing tested."""
import numpy as np
import scipy.sparse as sp

import block_iter_ref as ir

LD, U = ir.LD, ir.U


def coarsen_psi(Psi, agg, nc, dt):
    """Psi P_s in dtype dt -> (indptr, indices, data): per row the coarse columns ascending, each the sum of its fine entries in ascending fine-column order
    (obs_coarsen, csrc/host_obs.cpp)"""
    ip, idx, v = Psi
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    keys = rows * np.int64(nc) + agg[idx]
    order = np.argsort(keys, kind="stable")   # (stable: the fine columns of a coarse entry stay ascending)
    ks = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if len(ks) else np.zeros(0, dtype=np.int64)
    uniq = ks[starts]
    data = np.add.reduceat(v[order], starts) if len(ks) else np.zeros(0, dtype=dt)
    ipc = np.zeros(len(ip), dtype=np.int64)
    np.add.at(ipc, uniq // nc + 1, 1)
    return np.cumsum(ipc), (uniq % nc).astype(np.int64), data.astype(dt)


class LevelTerm(ir.ObsTerm):
    """ObsTerm of a level from (indptr, indices, data) in dtype dt"""

    def __init__(self, csr, n, w, scale, dt):
        ip, idx, v = csr
        self.n = n
        P = sp.csr_matrix((np.arange(1, len(idx) + 1), idx, ip), shape=(len(ip) - 1, n))
        T = P.T.tocsr()
        T.sort_indices()
        self.P = (np.asarray(ip, dtype=np.int64), np.asarray(idx, dtype=np.int64), np.asarray(v, dtype=dt))
        self.T = (T.indptr.astype(np.int64), T.indices.astype(np.int64), self.P[2][T.data - 1])
        self.w, self.scale, self.dt = np.asarray(w, dtype=dt), dt(scale), dt

    def dense(self):
        """scale Psi^T W Psi as a dense n x n array in dt"""
        m = len(self.P[0]) - 1
        D = np.zeros((m, self.n), dtype=self.dt)
        D[np.repeat(np.arange(m), np.diff(self.P[0])), self.P[1]] = self.P[2]
        return self.scale * (D.T @ (self.w[:, None] * D))


def _first_field(z):
    return np.stack([z, np.zeros_like(z)], axis=1).reshape(-1)


class TermLevel:
    """a level's matrix: the block CSR part and the term beside it; what block_iter_ref.Hierarchy asks of a level"""

    def __init__(self, base, term):
        self.base, self.term = base, term
        self.rp, self.ci, self.n, self.dt, self.bv = base.rp, base.ci, base.n, base.dt, base.bv

    def mv(self, x):   # (the pattern product, then the term's two products added: the order of the device's launches)
        return self.base.mv(x) + _first_field(self.term.apply(x.reshape(-1, 2)[:, 0]))

    def amv(self, x):
        return self.base.amv(x) + _first_field(self.term.apply(x.reshape(-1, 2)[:, 0], absolute=True))

    def diagonal_blocks(self):
        d = self.base.diagonal_blocks().copy()
        d[:, 0] += self.term.diagonal()
        return d

    def dense(self):
        M = self.base.dense()
        M[0::2, 0::2] += self.term.dense()
        return M


class TermHierarchy(ir.Hierarchy):
    """block_iter_ref.Hierarchy on given aggregates with the term on every level.  .psi_nnz[l] = nnz(Psi_l)"""

    def __init__(self, rp, ci, blocks, n, aggregates, Psi, weights=None, scale=-1.0, dt=LD, like_device=False):
        self.dt, self.like_device = dt, like_device
        bv = np.stack([np.zeros(len(ci)) if b is None else np.asarray(b, dtype=float) for b in blocks], axis=1)
        P = Psi.tocsr().copy()
        P.sum_duplicates()
        P.sort_indices()
        self._w = np.ones(P.shape[0]) if weights is None else np.asarray(weights, dtype=float)
        self._scale = scale
        csr = (P.indptr.astype(np.int64), P.indices.astype(np.int64), P.data.astype(dt))
        self._levels(TermLevel(ir.BlockCsr(rp, ci, bv, dt), LevelTerm(csr, n, self._w, scale, dt)), n, aggregates)
        self.psi_nnz = [len(A.term.P[1]) for A in self.A]

    def _galerkin(self, A, agg, nc):
        return TermLevel(ir.galerkin(A.base, agg, nc), LevelTerm(coarsen_psi(A.term.P, agg, nc, self.dt), nc, self._w, self._scale, self.dt))


def iterates(rp, ci, blocks, n, aggregates, Psi, b, K, weights=None, scale=-1.0, restart=50):
    """the extended-precision reference -> [Iterate k = 1 .. K]"""
    return ir.fgmres_iterates(TermHierarchy(rp, ci, blocks, n, aggregates, Psi, weights, scale), b, K, restart)


def iterates_float64(rp, ci, blocks, n, aggregates, Psi, b, K, weights=None, scale=-1.0, restart=50):
    """the checker: the same scheme in float64 as the device runs it"""
    return ir.fgmres_iterates(TermHierarchy(rp, ci, blocks, n, aggregates, Psi, weights, scale, dt=np.float64, like_device=True), b, K, restart)


# ---- the cases and the constants both tests share ---------------------------------------------------------------------------------------------------
# (fixture, order, lambda, tiles per axis); amg_coarse_rows = 256; each at k = 1, 2, 3, 5, 8, under block_obs_team 8 and 64 against one reference
CASES = {
    "sq-p1-4x4": ("unit_square_16", 1, 1e-2, 4),   # 16 rows of 25: the partial workgroup of a T = 8 launch
    "sq-p1-2x2": ("unit_square_16", 1, 1e-2, 2),   # rows of 81: two trips of a 64-lane team
    "sq-p2-4x4": ("unit_square_16", 2, 1e-4, 4),   # three levels: GCR steps with the term inside y
    "sphere-p1-2": ("unit_sphere", 1, 1e-2, 2),    # a surface, three levels
}
KS = (1, 2, 3, 5, 8)
COARSE_ROWS = 256
TEAMS = (8, 64)
# c(k) = 4 r_cpu(k) rounded up to a power of two, r_cpu(k) = max_i |x_k^f64 - x_k^ld|_i / (u s_i) over the cases -- and the same ratio of
# the residual --: tests/test_block_obs_amg_iter_cpu.py measures it with the restatement's aggregates and fails if a constant no longer fits
C_OBS_AMG = {1: 262144.0, 2: 2048.0, 3: 1024.0, 5: 512.0, 8: 256.0}
# the same rule in block_iter_ref.field_ratios' unit, per field max |x - x_ref| / (u max s): the unit of the multilevel stage's older iterate test, asserted too
C_OBS_AMG_FIELD = {1: 256.0, 2: 64.0, 3: 64.0, 5: 64.0, 8: 32.0}
