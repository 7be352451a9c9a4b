"""Extended-precision reference for the k-th iterate of the Kronecker-sum handle's two Krylov stages, with the scale its error is measured in -- plain
numpy, nothing of the library (tests/test_kron_iter_cpu.py, tests/test_gpu_kron_iterates.py).  Built on tests/block_iter_ref.py: its (flexible) GMRES, the
GCR correction in k_amg_coef's reading, the written-out LU of the last level and the units of the bounds are used as they are.

The operator A = sum_sigma T_sigma (x) S_sigma is applied FACTORED, Y = sum_sigma S_sigma X T_sigma^T on n x q arrays (row i: the q unknowns of DOF i), the
row sums of S_sigma X by reduceat; no q n-row matrix is formed except the last level's.  Terms that hand over the same array share a factor
(kron_amg_ref.merge).  D^-1: the q x q diagonal blocks inverted by Gaussian elimination with partial pivoting written out, vectorised over the DOFs; with a
factored data term live (fdapde_kron_set_obs) the blocks of the full matrix A + scale (Phi (x) Psi)^T W (Phi (x) Psi), the term applied as two rectangular
products.

FDAPDE_SOLVER_KRON_AMG (csrc/eng_kron_amg.hip).  The aggregates are DATA (fdapde_kron_amg_aggregates, level 0 in the reference numbering).  P = P_scalar
(x) I_q: the n_S spatial values of a coarse entry are summed over its fine entries, the time factors are those of level 0 on every level; the cycle 0.7
D^-1 / coarse correction / 0.7 D^-1, two GCR steps below the finest level, the last level exactly, flexible GMRES on the UNSCALED system restarted from
the true residual.  With the aggregates fixed, iterate k is ONE vector in exact arithmetic.

The handle's GMRES stage (kron_gmres through handle_gmres, operator launch_kron_op): GMRES(m) on D^-1 A z = D^-1 b, with and without the factored term.

Vectors go in and out in the KRONECKER order (unknown r of DOF i at r n + i), as fdapde_kron_solve takes them; inside they are interleaved per DOF.

Scale and units as in block_iter_ref: s = sum_j |y_j| |z_j| entrywise.  Multilevel stage: per unknown r = 0 .. q - 1 the n entries of that unknown are
one field, max |x - x_ref| / (u max s) over the field.  GMRES stage: entrywise |x - x_ref|_i <= c u s_i, exactly 0 where s_i = 0.  relres against rho_k
in units of u || |A| s || / ||b||; for the GMRES stage |A| stands for |D^-1| (|A| + |term|), the two products the device forms one after the other.

`Hierarchy(..., dt=np.float64, like_device=True)`, `fgmres_float64` and `gmres_float64` are the two schemes in float64 the way the device runs them (the
diagonal blocks by the same elimination in float64, the last level as the explicit inverse of the row-equilibrated matrix, D^-1 (A x) and D^-1 z formed
apart and added): measuring sticks for the constants, never the thing tested."""
import numpy as np

import block_iter_ref as ir
import kron_amg_ref as ka

LD, U, OMEGA, LAST_LEVEL_ROWS = ir.LD, ir.U, ir.OMEGA, ir.LAST_LEVEL_ROWS
Iterate = ir.Iterate
LDS_FACTOR_DOUBLES = 1024   # kKronLdsFactorDoubles: the time factors ride in LDS where n_S q^2 is at most this


def to_rows(v, n, q):
    """Kronecker order (r n + i) -> interleaved per DOF (i q + r), flat"""
    return np.asarray(v).reshape(q, n).T.reshape(-1).copy()


def to_kron(v, n, q):
    return np.asarray(v).reshape(n, q).T.reshape(-1).copy()


class KronCsr:
    """sum_sigma T_sigma (x) S_sigma on a pattern: Ts[sigma] q x q, Ss[sigma] one value per pattern entry; vectors interleaved per DOF"""

    def __init__(self, rp, ci, Ts, Ss, dt):
        self.rp, self.ci, self.n, self.dt = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), len(rp) - 1, dt
        self.Ts = [np.asarray(T, dtype=dt) for T in Ts]
        self.S = np.stack([np.asarray(S, dtype=dt) for S in Ss], axis=1)   # (entries, n_S)
        self.q = self.Ts[0].shape[0]
        assert self.S.shape == (len(self.ci), len(self.Ts)) and (np.diff(self.rp) > 0).all() and all(T.shape == (self.q, self.q) for T in self.Ts)

    def _mv(self, Ts, S, x):
        G = x.reshape(self.n, self.q)[self.ci]
        Y = np.zeros((self.n, self.q), dtype=self.dt)
        for sg, T in enumerate(Ts):
            Y += np.add.reduceat(S[:, sg, None] * G, self.rp[:-1], axis=0) @ T.T
        return Y.reshape(-1)

    def mv(self, x):
        return self._mv(self.Ts, self.S, x)

    def amv(self, x):
        return self._mv([np.abs(T) for T in self.Ts], np.abs(self.S), np.abs(x))

    def _entry_blocks(self, k):
        """sum_sigma S_sigma[k] T_sigma for the pattern entries k -> (len(k), q, q)"""
        return sum(self.S[k, sg, None, None] * T[None, :, :] for sg, T in enumerate(self.Ts))

    def diagonal_blocks(self):
        d = np.flatnonzero(ir._rows_of(self.rp) == self.ci)
        assert len(d) == self.n, "every row holds its diagonal entry"
        return self._entry_blocks(d)

    def dense(self):
        """the q n-row matrix, interleaved per DOF (the last level only)"""
        M = np.zeros((self.n, self.n, self.q, self.q), dtype=self.dt)
        M[ir._rows_of(self.rp), self.ci] = self._entry_blocks(np.arange(len(self.ci)))
        return M.transpose(0, 2, 1, 3).reshape(self.n * self.q, self.n * self.q)


def galerkin(A, agg, nc):
    """P^T A P for P = P_scalar (x) I_q: the n_S spatial values of every coarse entry summed over its fine entries, the time factors unchanged"""
    keys = agg[ir._rows_of(A.rp)] * np.int64(nc) + agg[A.ci]
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    uniq = ks[starts]
    rp_c = np.zeros(nc + 1, dtype=np.int64)
    np.add.at(rp_c, uniq // nc + 1, 1)
    S = ir._segment_sums(A.S, order, starts)
    return KronCsr(np.cumsum(rp_c), uniq % nc, A.Ts, [S[:, sg] for sg in range(S.shape[1])], A.dt)


def blocks_inverse(D):
    """the inverses of q x q blocks (n, q, q): Gauss-Jordan with partial pivoting, written out (numpy.linalg has no extended precision), all blocks at once;
    a pivot not above 1e-14 of its block's largest entry is what the device refuses"""
    n, q, _ = D.shape
    M = np.concatenate([D, np.broadcast_to(np.eye(q, dtype=D.dtype), D.shape)], axis=2)
    idx = np.arange(n)
    mx = np.abs(D).max(axis=(1, 2))
    for k in range(q):
        p = k + np.argmax(np.abs(M[:, k:, k]), axis=1)
        top, low = M[idx, k].copy(), M[idx, p].copy()
        M[idx, k], M[idx, p] = low, top
        piv = M[:, k, k].copy()
        assert np.all(np.abs(piv) > 1e-14 * mx), "a singular diagonal block: the device refuses (level 0) or ends the hierarchy one level above"
        M[:, k] = M[:, k] / piv[:, None]
        f = M[:, :, k].copy()
        f[:, k] = 0
        M -= f[:, :, None] * M[:, k][:, None, :]
    return M[:, :, q:].copy()


def dinv_apply(dinv, r):
    q = dinv.shape[1]
    return np.einsum("irs,is->ir", dinv, r.reshape(-1, q)).reshape(-1)


def blocks_lu(D):
    """P D = L U of q x q blocks (n, q, q) with partial pivoting, all blocks at once -> (LU in one array, row order (n, q)): a third of the inverse's work,
    for hierarchies of many DOFs at q = 33"""
    n, q, _ = D.shape
    M = D.copy()
    idx = np.arange(n)
    perm = np.tile(np.arange(q), (n, 1))
    mx = np.abs(D).max(axis=(1, 2))
    for k in range(q):
        p = k + np.argmax(np.abs(M[:, k:, k]), axis=1)
        top, low = M[idx, k].copy(), M[idx, p].copy()
        M[idx, k], M[idx, p] = low, top
        pk, pp = perm[idx, k].copy(), perm[idx, p].copy()
        perm[idx, k], perm[idx, p] = pp, pk
        assert np.all(np.abs(M[:, k, k]) > 1e-14 * mx), "a singular diagonal block: the device refuses (level 0) or ends the hierarchy one level above"
        M[:, k + 1:, k] /= M[:, k, k, None]
        M[:, k + 1:, k + 1:] -= M[:, k + 1:, k, None] * M[:, k, None, k + 1:]
    return M, perm


def blocks_solve(lu, perm, r):
    """D_i z_i = r_i for every block, from blocks_lu's factors"""
    n, q, _ = lu.shape
    y = np.take_along_axis(r.reshape(n, q), perm, axis=1)
    for i in range(1, q):
        y[:, i] -= (lu[:, i, :i] * y[:, :i]).sum(axis=1)
    for i in range(q - 1, -1, -1):
        y[:, i] = (y[:, i] - (lu[:, i, i + 1:] * y[:, i + 1:]).sum(axis=1)) / lu[:, i, i]
    return y.reshape(-1)


class Hierarchy(ir.Hierarchy):
    """the levels FDAPDE_SOLVER_KRON_AMG builds on GIVEN aggregates (aggregates[l][i] = the DOF of level l + 1 that DOF i of level l belongs to, level 0 in
    the caller's numbering).  .rows[l] / .entries[l]: DOFs and pattern entries of level l -- the device reports q n_l and q^2 nnz_l.  cycle, correction,
    precondition and the last level's solve are block_iter_ref.Hierarchy's"""

    def __init__(self, rp, ci, terms, n, aggregates, dt=LD, like_device=False):
        self.dt, self.like_device = dt, like_device
        Ts, Ss, _ = ka.merge(terms)
        self.per = self.q = Ts[0].shape[0]
        self.n_s = len(Ss)
        self._levels(KronCsr(rp, ci, Ts, Ss, dt), n, aggregates)

    def _diag_inverse(self, A):
        """like_device: the explicit inverses (k_kron_diag_inv's arithmetic in float64); the reference solves with the blocks' factors instead"""
        return blocks_inverse(A.diagonal_blocks()) if self.like_device else blocks_lu(A.diagonal_blocks())

    def _galerkin(self, A, agg, nc):
        return galerkin(A, agg, nc)

    def smooth(self, l, r):
        return dinv_apply(self.dinv[l], r) if self.like_device else blocks_solve(*self.dinv[l], r)


def _pack(out, n, q):
    return [Iterate(k + 1, to_kron(x, n, q), to_kron(s, n, q), float(rho), float(rs)) for k, (x, s, rho, rs) in enumerate(out)]


def fgmres_iterates(H, b, K, restart=50):
    """flexible GMRES, right-preconditioned by H's cycle, on the unscaled system, restarted every `restart` vectors from the true residual as fgmres_outer
    does -> [Iterate k = 1 .. K] in H's dtype (np.longdouble: the reference); b and the iterates in the Kronecker order"""
    A = H.A[0]
    return _pack(ir._iterates(H.dt, A.mv, A.amv, H.precondition, to_rows(np.asarray(b, dtype=float), A.n, A.q).astype(H.dt), K, restart), A.n, A.q)


def fgmres_float64(rp, ci, terms, n, aggregates, b, K, restart=50):
    """the checker: the same scheme in float64 as the device runs it"""
    return fgmres_iterates(Hierarchy(rp, ci, terms, n, aggregates, dt=np.float64, like_device=True), b, K, restart)


class ObsTerm:
    """scale (Phi (x) Psi)^T W (Phi (x) Psi) applied as its rectangular products in dtype dt: Phi p x q dense (None: [I_p 0]), Psi n_obs x n of any row
    length, W (p, n_obs) or flat in the Kronecker order (instant tau, location k at tau n_obs + k), None: ones"""

    def __init__(self, Phi, Psi, W, scale, q, dt):
        P = Psi.tocsr().copy()
        P.sum_duplicates()
        P.sort_indices()
        T = P.T.tocsr()
        T.sort_indices()
        self.P = (P.indptr, P.indices, P.data.astype(dt))
        self.T = (T.indptr, T.indices, T.data.astype(dt))
        n_obs = P.shape[0]
        if Phi is None:
            p = q if W is None else (np.shape(W)[0] if np.ndim(W) == 2 else np.size(W) // n_obs)
            Phi = np.eye(p, q)
        self.Phi = np.asarray(Phi, dtype=float).astype(dt)
        self.p = self.Phi.shape[0]
        assert self.Phi.shape == (self.p, q)
        self.Wt = (np.ones((self.p, n_obs)) if W is None else np.asarray(W, dtype=float).reshape(self.p, n_obs)).T.astype(dt)   # (n_obs, p)
        self.scale, self.q, self.dt = dt(scale), q, dt

    def apply(self, x, absolute=False):
        """the term times x (interleaved), or |scale| |B|^T |W| |B| |x|"""
        f = np.abs if absolute else (lambda v: v)
        P, T = ((m[0], m[1], f(m[2])) for m in (self.P, self.T))
        Phi = f(self.Phi)
        t = f(self.Wt) * (ir.csr_product(*P, f(x).reshape(-1, self.q)) @ Phi.T)   # (n_obs, p): W (Phi (x) Psi) x
        return (f(self.scale) * (ir.csr_product(*T, t) @ Phi)).reshape(-1)

    def diagonal_blocks(self):
        """the term's share of every DOF's diagonal block: Phi^T diag(g_i) Phi, g_i[tau] = scale sum_k w[tau, k] Psi[k, i]^2 -> (n, q, q)"""
        ip, idx, v = self.T
        g = self.scale * ir.csr_product(ip, idx, v * v, self.Wt)   # (n, p)
        return np.einsum("tr,it,ts->irs", self.Phi, g, self.Phi)


def _gmres(rp, ci, terms, n, b, K, restart, dt, like_device, obs):
    Ts, Ss, _ = ka.merge(terms)
    A = KronCsr(rp, ci, Ts, Ss, dt)
    assert A.n == n
    q = A.q
    D = A.diagonal_blocks()
    term = None
    if obs is not None:
        term = ObsTerm(obs["Phi"], obs["Psi"], obs["W"], obs["scale"], q, dt)
        D = D + term.diagonal_blocks()
    dinv = blocks_inverse(D)
    adinv = np.abs(dinv)
    bt = dinv_apply(dinv, to_rows(np.asarray(b, dtype=float), n, q).astype(dt))

    def mv(x):
        if term is None:
            return dinv_apply(dinv, A.mv(x))
        if like_device:   # (launch_kron_op, then the scatter with D^-1: two products added)
            return dinv_apply(dinv, A.mv(x)) + dinv_apply(dinv, term.apply(x))
        return dinv_apply(dinv, A.mv(x) + term.apply(x))

    def amv(x):
        return dinv_apply(adinv, A.amv(x) + (term.apply(x, absolute=True) if term is not None else 0))

    return _pack(ir._iterates(dt, mv, amv, None, bt, K, restart), n, q)


def gmres_iterates(rp, ci, terms, n, b, K, restart=50, obs=None):
    """GMRES(restart) on D^-1 A z = D^-1 b, D^-1 formed in np.longdouble -> [Iterate]: x_k, s = sum_j |y_j| |v_j|, rho_k and res_scale of the SCALED system.
    obs = dict(Phi, Psi, W, scale): A and D are the full matrix's"""
    return _gmres(rp, ci, terms, n, b, K, restart, LD, False, obs)


def gmres_float64(rp, ci, terms, n, b, K, restart=50, obs=None):
    return _gmres(rp, ci, terms, n, b, K, restart, np.float64, True, obs)


# ---- the units of the bounds -----------------------------------------------------------------------------------------------------------------------
def field_ratios(x, ref, q):
    """FDAPDE_SOLVER_KRON_AMG's unit: per unknown r (the n entries r n .. (r + 1) n of the Kronecker order are one field) max |x - ref.x| / (u max s)"""
    n = len(ref.x) // q
    err = np.abs(np.asarray(x).astype(LD) - ref.x).reshape(q, n).max(axis=1)
    smax = ref.s.reshape(q, n).max(axis=1)
    return [float(e / (U * s)) if s > 0 else (0.0 if e == 0 else float("inf")) for e, s in zip(err, smax)]


entry_ratio, relres_ratio, constant_for, C_MAX = ir.entry_ratio, ir.relres_ratio, ir.constant_for, ir.C_MAX


def residual(A, b, x):
    """|b - A x| / |b| of a vector in the Kronecker order, in A's dtype"""
    bl = to_rows(np.asarray(b, dtype=float), A.n, A.q).astype(A.dt)
    r = bl - A.mv(to_rows(x, A.n, A.q).astype(A.dt))
    return float(np.sqrt(r @ r) / np.sqrt(bl @ bl))


def residual_scale(A, b, x):
    """|| |A| |x| + |b| || / |b|: what a rounding of every term of b - A x moves the relative residual by, in units of u"""
    bl = np.abs(to_rows(np.asarray(b, dtype=float), A.n, A.q).astype(A.dt))
    t = A.amv(to_rows(x, A.n, A.q).astype(A.dt)) + bl
    return float(np.sqrt(t @ t) / np.sqrt(bl @ bl))


# ---- the cases and the constants both tests share ---------------------------------------------------------------------------------------------------
# a system is a case of kron_amg_ref.system -- ("spacetime", mesh, order, m, lambda = lambda_T) | ("parabolic" | "dense_t", mesh, order, q, dt) -- or
# ("spacetime_t", mesh, order, m, lambda, lambda_T) | ("spacetime+1", ...): the space-time system with one more DISTINCT spatial factor (lambda M_t (x) 0.25 R0 on the last block, an array of its own);
# meshes are meshgen's
SQ16, SQ64, SQ160 = ("unit_square", 16), ("unit_square", 64), ("unit_square", 160)
SYSTEMS = {
    "a": ("spacetime", SQ16, 1, 3, 1e-4),      # q = 6: Q = 8 with idle lanes; symmetric indefinite
    "b": ("parabolic", SQ16, 1, 1, 0.01),      # a team of 2 with one idle lane
    "c": ("parabolic", SQ16, 1, 2, 0.01),      # a full team of 2
    "d": ("parabolic", SQ16, 1, 5, 0.01),      # bidiagonal T: the band skip of kamg_time; a non-symmetric chain
    "e": ("dense_t", SQ16, 1, 5, 0.01),        # no band to skip
    "f": ("spacetime", SQ16, 1, 8, 1e-4),      # q = 16, n_S = 4: n_S q^2 = 1 024, the time factors in LDS at the limit
    "f+": ("spacetime+1", SQ16, 1, 8, 1e-4),   # n_S = 5: 1 280 doubles, from global memory
    "g": ("parabolic", SQ16, 1, 33, 0.01),     # Q = 64, 31 idle lanes, the factors from global memory
    # q = 64: Q = 64 full.  lambda = 1e-2 with lambda_T = 1e-4: at lambda_T = lambda the float64 checker is 4e3 to 2e4 units off the reference at k = 1
    # for every lambda from 1e-4 to 100 (with the exact D^-1 and last level as well: the cycle's own sums cancel), at lambda_T <= lambda / 100 it is 5
    "h": ("spacetime_t", SQ16, 1, 32, 1e-2, 1e-4),
    "i": ("parabolic", ("unit_cube", 8), 1, 3, 0.01),
    "j": ("parabolic", ("unit_square", 8), 2, 3, 0.01),   # P2: rows of 6 .. 19 entries
    "o": ("parabolic", SQ64, 1, 33, 0.01),     # 4 225 DOFs: n Q / 256 = 1 057 workgroups' worth of rows on level 0, np at its cap
    # 25 921 DOFs.  k_kamg_spmv_dots runs on the levels with GCR steps only, 1 .. last - 1, never on level 0: its row loop takes a second trip where such a
    # level has more than 1 024 workgroups' worth of rows, n_l Q / 256 > 1 024, i.e. more than 4 096 DOFs at Q = 64 -- level 1 of this mesh under absorption
    "p": ("parabolic", SQ160, 1, 33, 0.01),
}
# (system, knobs, the k a solve stops at).  amg_coarse_rows per case: the last level has at most LAST_LEVEL_ROWS rows, and (k, l apart) there are >= 3 levels
AMG_CASES = {
    "a": ("a", dict(amg_coarse_rows=256), (1, 2, 3, 5, 8)),
    "b": ("b", dict(amg_coarse_rows=32), (1, 2, 3, 5, 8)),
    "c": ("c", dict(amg_coarse_rows=64), (1, 2, 3, 5, 8)),
    "d": ("d", dict(amg_coarse_rows=256), (1, 2, 3, 5, 8)),
    "e": ("e", dict(amg_coarse_rows=256), (1, 2, 3, 5, 8)),
    "f": ("f", dict(amg_coarse_rows=700), (1, 2, 3, 5)),
    "f+": ("f+", dict(amg_coarse_rows=700), (1, 2, 3, 5)),
    "g": ("g", dict(amg_coarse_rows=700), (1, 2, 3, 5)),
    "h": ("h", dict(amg_coarse_rows=700), (1, 2, 3)),
    "i": ("i", dict(amg_coarse_rows=256, amg_absorb=1), (1, 2, 3, 5)),
    "j": ("j", dict(amg_coarse_rows=128), (1, 2, 3, 5)),
    # q n = 578 <= amg_coarse_rows: one level, amg_dense_cols alone.  k = 1 only: the first iterate is the solution, there is no second one
    "k": ("c", dict(amg_coarse_rows=600), (1,)),
    "l": ("c", dict(amg_coarse_rows=200), (1, 2, 3)),     # two levels exactly: the cycle without GCR steps
    "m": ("a", dict(amg_coarse_rows=256, gmres_m=3), (5,)),
    "n": ("d", dict(amg_coarse_rows=256), (1, 2, 3)),     # two different columns in one call
    # o, p: without absorption the matching pairs fewer and fewer rows on the coarse levels and the hierarchy ends by the stall rule at a last level of 891
    # and 3 531 rows, above LAST_LEVEL_ROWS under every amg_coarse_rows: hence amg_absorb = 1, under which a level keeps about a fifth of its DOFs
    "o": ("o", dict(amg_coarse_rows=700, amg_absorb=1), (1, 2)),
    "p": ("p", dict(amg_coarse_rows=700, amg_absorb=1), (1,)),
}
THREE_LEVELS = tuple(c for c in AMG_CASES if c not in ("k", "l"))
# (system, knobs, right-hand side, k)
GMRES_CASES = {
    "q1": ("b", {}, "system", (1, 2, 3, 5, 8)),
    "q5": ("d", {}, "system", (1, 2, 3, 5, 8)),
    "q33": ("g", {}, "system", (1, 2, 3, 5, 8)),
    "q5-nofuse": ("d", dict(kron_fuse=0), "system", (1, 2, 3, 5, 8)),
    "q5-restart": ("d", dict(gmres_m=3), "system", (5, 7)),
    "q5-unit": ("d", {}, "unit", (1, 2, 3)),
}
# with a factored term on the four pattern terms of the space-time system (kron_obs_ref.spacetime): (mesh, m, p, lambda = lambda_T, design of
# kron_obs_ref.design_psi, share of missing observations, Phi: "hats" = [H, 0] | "null" = NULL with p < q | "dense" = random p x q with p > q,
# knobs, edit of Psi, k).  Two choices keep the float64 checker under 2^12 / 4 units: lambda = 100 (at 1e-4 the diagonal blocks of the full matrix
# have a condition number of 1e5 and the checker is 5e4 units off at k = 1), and a right-hand side with ONE non-zero unknown per DOF, the data of the first
# time unknown (entries 0 .. n): D_i^-1 b_i is then one product per entry.  With every unknown random, the worst of the q n entries of D^-1 b cancels by a
# factor of about q n -- 2.5e3 to 5e3 units at k = 1 measured on these cases -- which says nothing about the code under test
SQ32 = ("unit_square", 32)
GMRES_OBS_CASES = {
    "points-narrow": (SQ16, 3, 4, 1e2, ("points", 400), 0.3, "hats", dict(kron_obs_form=1), None, (1, 2, 3, 5, 8)),
    "points-wide": (SQ16, 3, 4, 1e2, ("points", 400), 0.3, "hats", dict(kron_obs_form=2), None, (1, 2, 3, 5, 8)),
    "tiles-narrow": (SQ32, 3, 4, 1e2, ("tiles", 2), 0.3, "hats", dict(kron_obs_form=1), None, (1, 2, 3, 5, 8)),   # 4 tiles: rows of 289 entries
    "tiles-wide": (SQ32, 3, 4, 1e2, ("tiles", 2), 0.3, "hats", dict(kron_obs_form=2), None, (1, 2, 3, 5, 8)),
    "phi-null": (SQ16, 3, 3, 1e2, ("points", 400), 0.3, "null", {}, None, (1, 2, 3, 5, 8)),
    "phi-dense": (SQ16, 3, 12, 1e2, ("points", 400), 0.3, "dense", {}, None, (1, 2, 3, 5, 8)),   # QP = 16 above the product's Q = 8
    "holes": (SQ16, 3, 4, 1e2, ("points", 400), 0.3, "hats", {}, "holes", (1, 2, 3, 5, 8)),      # an empty row of Psi and an empty row of Psi^T
}
# c(k) = 4 r_cpu(k) rounded up to a power of two, r_cpu the worst ratio of the float64 checkers above against the reference over the cases and both units
# (the iterate's and relres'): tests/test_kron_iter_cpu.py measures it on the oracle's matrices and fails if a constant no longer fits or exceeds 2^12
C_AMG = {1: 1024.0, 2: 128.0, 3: 32.0, 5: 32.0, 8: 32.0}
C_GMRES = {1: 512.0, 2: 512.0, 3: 128.0, 5: 128.0, 7: 32.0, 8: 64.0}
C_GMRES_OBS = {1: 512.0, 2: 4096.0, 3: 128.0, 5: 4096.0, 8: 512.0}


def system(case, rp, ci, R1, R0, obs):
    """-> (terms, q, b in the Kronecker order): kron_amg_ref.system, and the space-time system with one more distinct spatial factor"""
    import kron_ref as kr

    if case[0] == "spacetime_t":
        m, lam, lam_t = case[3:]
        return kr.spacetime_terms(rp, ci, R1, R0, obs, lam, lam_t, m), 2 * m, kr.spacetime_rhs(obs, lam, len(rp) - 1, m)
    if case[0] != "spacetime+1":
        return ka.system(case, rp, ci, R1, R0, obs)
    terms, q, b = ka.system(("spacetime",) + tuple(case[1:]), rp, ci, R1, R0, obs)
    m, lam = case[3], case[4]
    return terms + [(kr._in_block(lam * kr.time_mass(m), m, 1, 1), 0.25 * np.asarray(R0, dtype=float))], q, b


def second_column(b):
    """case n's other right-hand side"""
    return np.random.default_rng(11).standard_normal(len(b))


def unit_rhs(n, q, dof, r=0):
    """one unit entry, unknown r of DOF dof"""
    b = np.zeros(q * n)
    b[r * n + dof] = 1.0
    return b


def obs_system(case, rp, ci, R1, R0, Psi):
    """-> (terms, q, b, obs = dict(Phi, Psi, W, scale) for the reference, Phi as handed to fdapde_kron_set_obs) of a case of GMRES_OBS_CASES"""
    import kron_obs_ref as ko

    _, m, p, lam, _, miss, phi, _, _, _ = case
    terms, Phi, W, b = ko.spacetime(rp, ci, R1, R0, Psi, lam, lam, m, p, miss)
    q = 2 * m
    given = Phi
    if phi == "null":
        assert p < q
        Phi, given = ko.identity_phi(p, q), None
        b = ko.spacetime_rhs(Phi, Psi, W, lam, m, len(rp) - 1, np.random.default_rng(6))
    elif phi == "dense":
        assert p > q
        Phi = given = np.random.default_rng(8).standard_normal((p, q)) / np.sqrt(p)
        b = ko.spacetime_rhs(Phi, Psi, W, lam, m, len(rp) - 1, np.random.default_rng(6))
    b[len(rp) - 1:] = 0.0   # (see GMRES_OBS_CASES: the data of the first time unknown alone)
    return terms, q, b, dict(Phi=Phi, Psi=Psi, W=W, scale=-1.0), given


def with_holes(Psi):
    """Psi with one row emptied and every entry of one column removed: an observation outside the mesh, and a DOF that no observation touches"""
    P = Psi.tocsr().copy()
    col = int(P.indices[P.indptr[P.shape[0] // 2]])
    P = P.tolil()
    P[7, :] = 0
    P[:, col] = 0
    P = P.tocsr()
    P.eliminate_zeros()
    P.sort_indices()
    assert P.indptr[8] == P.indptr[7] and not (P.indices == col).any()
    return P
