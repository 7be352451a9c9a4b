"""Extended-precision reference for the k-th iterate of the 2 x 2 block handle's two Krylov stages, with the scale its error is measured in -- plain numpy,
nothing of the library (tests/test_block_iter_cpu.py, tests/test_gpu_block_iterates.py).

FDAPDE_SOLVER_BLOCK_AMG (csrc/eng_block_amg.hip).  The aggregates are DATA here: the matching is a heuristic that `amg_setup_check` already holds to host
loops bit for bit, and a restatement in the caller's numbering pairs other rows than the device does in its internal order.  Everything numerical that is
built on the aggregates is restated: P = P_scalar (x) I_2, the block Galerkin sums, D^-1 of the 2 x 2 diagonal blocks, the cycle 0.7 D^-1 / coarse
correction / 0.7 D^-1, the two GCR steps below the finest level in k_amg_coef's reading, the last level solved exactly, and flexible GMRES around it on the
UNSCALED system, restarted from the true residual.  With the aggregates fixed, iterate k of that scheme is ONE vector in exact arithmetic: the order of
the sums, the team width of a kernel, the form of the last level's solve and the orthogonalisation variant do not change it.

The handle's GMRES stage (block_gmres in csrc/eng_block.hip): GMRES(m) on D^-1 A z = D^-1 b with D^-1 formed here, in np.longdouble; with a factored data
term live (fdapde_block_set_obs) A and D are the full matrix's, the term applied as its two rectangular products (ObsTerm, GMRES_OBS_CASES).

Vectors are handed in and out STACKED in the caller's numbering (f = the first block row's n entries, then g), as fdapde_block_solve takes them.

The scale of entry i of iterate k is the magnitude of everything that was added up to make it: s = sum_j |y_j| |z_j| over the correction vectors of the
cycles so far (z_j = M^-1 v_j for the flexible form, the basis vector v_j for the GMRES stage), entrywise.  Where s_i = 0 the Krylov front has not arrived.

`Hierarchy(..., dt=np.float64, like_device=True)`, `fgmres_float64` and `gmres_float64` are the same two schemes in float64 the way the device runs them
(classical Gram-Schmidt twice, Givens rotations, the last level as the explicit inverse of the row-equilibrated matrix with a refinement step where it asks
for one, D^-1 folded into the values in float64).  They are the measuring stick for the constants of the GPU test, never the thing tested."""
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble must carry a 64-bit mantissa (x87 extended or wider) on the machine that runs the reference"
U = 2.0 ** -53
OMEGA = 0.7
LAST_LEVEL_ROWS = 700   # the written-out elimination is for a last level of a few hundred rows


@dataclass
class Iterate:
    k: int
    x: np.ndarray      # stacked, caller's numbering
    s: np.ndarray      # the per-entry scale of x
    rho: float         # ||b - A x_k|| / ||b|| (the GMRES stage: of the scaled system)
    res_scale: float   # || |A| s || / ||b||: what a rounding of relative size u in every term of x moves rho by


def interleave(v):
    """stacked (f then g) -> interleaved per row"""
    n = len(v) // 2
    return np.asarray(v).reshape(2, n).T.reshape(-1).copy()


def stack(v):
    n = len(v) // 2
    return np.asarray(v).reshape(n, 2).T.reshape(-1).copy()


def _rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


class BlockCsr:
    """block rows on a pattern: bv[k] = (a11, a12, a21, a22) of entry k; vectors interleaved per row.  Row sums by reduceat: every row holds its diagonal"""

    def __init__(self, rp, ci, bv, dt):
        self.rp, self.ci, self.n, self.dt = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), len(rp) - 1, dt
        self.bv = np.asarray(bv, dtype=dt)
        assert self.bv.shape == (len(self.ci), 4) and (np.diff(self.rp) > 0).all()
        self.abs = np.abs(self.bv)

    def _mv(self, bv, x):
        xj = x.reshape(self.n, 2)[self.ci]
        top = np.add.reduceat(bv[:, 0] * xj[:, 0] + bv[:, 1] * xj[:, 1], self.rp[:-1])
        bot = np.add.reduceat(bv[:, 2] * xj[:, 0] + bv[:, 3] * xj[:, 1], self.rp[:-1])
        return np.stack([top, bot], axis=1).reshape(-1)

    def mv(self, x):
        return self._mv(self.bv, x)

    def amv(self, x):
        return self._mv(self.abs, np.abs(x))

    def diagonal_blocks(self):
        d = np.flatnonzero(_rows_of(self.rp) == self.ci)
        assert len(d) == self.n, "every block row holds its diagonal block"
        return self.bv[d]

    def dense(self):
        M = np.zeros((2 * self.n, 2 * self.n), dtype=self.dt)
        r = _rows_of(self.rp)
        for q, (p, c) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            M[2 * r + p, 2 * self.ci + c] = self.bv[:, q]
        return M

    def left_scaled(self, dinv, like_device):
        """D^-1 A on the pattern; like_device: the products of k_block_scale, in its order"""
        d = dinv[_rows_of(self.rp)]
        a, b, c, e = (self.bv[:, q] for q in range(4))
        return BlockCsr(self.rp, self.ci, np.stack([d[:, 0] * a + d[:, 1] * c, d[:, 0] * b + d[:, 1] * e, d[:, 2] * a + d[:, 3] * c, d[:, 2] * b + d[:, 3] * e],
                                                   axis=1), self.dt)


def block_diag_inverse(diag, dt, like_device=False):
    """the inverses of 2 x 2 blocks (a, b, c, e) -> (e, -b, -c, a) / det; like_device: k_block_diag_inv's 1.0 / det first"""
    a, b, c, e = (diag[:, q] for q in range(4))
    det = a * e - b * c
    mx = np.max(np.abs(diag), axis=1)
    assert np.all(np.abs(det) > 1e-14 * mx * mx), "a singular diagonal block: the device refuses (level 0) or ends the hierarchy one level above"
    if like_device:
        inv = dt(1.0) / det
        return np.stack([e * inv, -b * inv, -c * inv, a * inv], axis=1)
    return np.stack([e / det, -b / det, -c / det, a / det], axis=1)


def _dinv_apply(dinv, r):
    r2 = r.reshape(-1, 2)
    return np.stack([dinv[:, 0] * r2[:, 0] + dinv[:, 1] * r2[:, 1], dinv[:, 2] * r2[:, 0] + dinv[:, 3] * r2[:, 1]], axis=1).reshape(-1)


def _segment_sums(values, order, starts):
    return np.add.reduceat(values[order], starts, axis=0)


def galerkin(A, agg, nc):
    """P^T A P for P = P_scalar (x) I_2 of the map row -> aggregate: the four block values of every coarse entry summed over its fine entries"""
    keys = agg[_rows_of(A.rp)] * np.int64(nc) + agg[A.ci]
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    uniq = ks[starts]
    rp_c = np.zeros(nc + 1, dtype=np.int64)
    np.add.at(rp_c, uniq // nc + 1, 1)
    return BlockCsr(np.cumsum(rp_c), uniq % nc, _segment_sums(A.bv, order, starts), A.dt)


def lu_partial_pivoting(M):
    """Gaussian elimination with partial pivoting, written out (numpy.linalg has no extended precision) -> (LU in one array, row order)"""
    A = M.copy()
    n = A.shape[0]
    perm = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        assert A[p, k] != 0, "the last level is singular"
        if p != k:
            A[[k, p]] = A[[p, k]]
            perm[[k, p]] = perm[[p, k]]
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
    return A, perm


def lu_solve(lu, perm, b):
    n = len(b)
    y = b[perm].copy()
    for i in range(1, n):
        y[i] -= lu[i, :i] @ y[:i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - lu[i, i + 1:] @ y[i + 1:]) / lu[i, i]
    return y


class Hierarchy:
    """the levels FDAPDE_SOLVER_BLOCK_AMG builds on GIVEN aggregates: aggregates[l][i] = the row of level l + 1 that block row i of level l belongs to
    (level 0 in the caller's numbering).  .rows[l] / .entries[l]: block rows and pattern entries of level l"""

    def __init__(self, rp, ci, blocks, n, aggregates, dt=LD, like_device=False):
        self.dt, self.like_device = dt, like_device
        bv = np.stack([np.zeros(len(ci)) if b is None else np.asarray(b, dtype=float) for b in blocks], axis=1)
        self._levels(BlockCsr(rp, ci, bv, dt), n, aggregates)

    per = 2   # unknowns per row (tests/kron_iter_ref.py: q)

    def _diag_inverse(self, A):
        return block_diag_inverse(A.diagonal_blocks(), self.dt, self.like_device)

    def _galerkin(self, A, agg, nc):
        return galerkin(A, agg, nc)

    def _levels(self, A0, n, aggregates):
        """every level from level 0's matrix and the maps row -> row of the next level"""
        self.A = [A0]
        self.agg, self.members, self.dinv = [], [], []
        assert n == self.A[0].n
        for agg in aggregates:
            A = self.A[-1]
            agg = np.asarray(agg, dtype=np.int64)
            nc = int(agg.max()) + 1
            assert agg.shape == (A.n,) and agg.min() == 0 and len(np.unique(agg)) == nc, "every row has an aggregate and every aggregate a row"
            order = np.argsort(agg, kind="stable")
            self.agg.append(agg)
            self.members.append((order, np.flatnonzero(np.concatenate([[True], np.diff(agg[order]) != 0]))))
            self.dinv.append(self._diag_inverse(A))
            self.A.append(self._galerkin(A, agg, nc))
        self.rows = [A.n for A in self.A]
        self.entries = [len(A.ci) for A in self.A]
        self._set_last(self.A[-1].dense())

    def _set_last(self, last):
        """the last level's solve from its dense matrix (interleaved order)"""
        assert last.shape[0] <= LAST_LEVEL_ROWS, last.shape
        if self.like_device:   # the explicit inverse of the row-equilibrated matrix (csrc/eng_dense.hip), one refinement step where max |I - A X| asks for it
            rs = 1.0 / np.abs(last).max(axis=1)
            self.last, self.X = last, np.linalg.inv(rs[:, None] * last) * rs[None, :]
            self.refine = not np.abs(np.eye(len(rs)) - last @ self.X).max() < 1e-13
        else:
            self.lu = lu_partial_pivoting(last)

    def solve_last(self, b):
        if not self.like_device:
            return lu_solve(*self.lu, b)
        x = self.X @ b
        return x + self.X @ (b - self.last @ x) if self.refine else x

    def restrict(self, l, r):
        order, starts = self.members[l]
        return _segment_sums(r.reshape(-1, self.per), order, starts).reshape(-1)

    def prolong(self, l, e):
        return e.reshape(-1, self.per)[self.agg[l]].reshape(-1)

    def smooth(self, l, r):
        """D^-1 r of level l"""
        return _dinv_apply(self.dinv[l], r)

    def cycle(self, l, r):
        """block_amg_ref.Hierarchy.cycle's formulas"""
        A = self.A[l]
        om = self.dt(OMEGA)
        zt = om * self.smooth(l, r)
        z = zt + self.prolong(l, self.correction(l + 1, self.restrict(l, r - A.mv(zt))))
        return z + om * self.smooth(l, r - A.mv(z))

    def correction(self, m, b):
        """the last level exactly; elsewhere two GCR steps around the cycle with k_amg_coef's rules: a step that cannot be taken contributes nothing"""
        if m + 1 == len(self.A):
            return self.solve_last(b)
        A, zero = self.A[m], self.dt(0)
        c = self.cycle(m, b)
        v = A.mv(c)
        rho1 = v @ v
        a1 = (v @ b) / rho1 if rho1 > 0 and np.isfinite(rho1) else zero
        if not np.isfinite(a1):
            a1 = zero
        rt = b - a1 * v
        d = self.cycle(m, rt)
        w = A.mv(d)
        gamma = v @ w
        rho2 = w @ w - gamma * gamma / rho1 if rho1 > 0 else zero
        cd = (w @ rt) / rho2 if rho2 > 0 and np.isfinite(rho2) else zero
        cc = a1 - (cd * gamma / rho1 if rho1 > 0 else zero)
        if not (np.isfinite(cd) and np.isfinite(cc)):
            cd, cc = zero, a1
        return cc * c + cd * d

    def precondition(self, v):
        return self.solve_last(v) if len(self.A) == 1 else self.cycle(0, v)


def _iterates(dt, mv, amv, precondition, b, K, restart):
    """(flexible) GMRES(restart) in dtype dt on the interleaved system: Gram-Schmidt twice, Givens rotations, the iterate of EVERY k formed from the
    least-squares problem of the columns so far, a restart from the true residual after `restart` vectors -> [(x_k, s_k, rho_k, res_scale_k)] interleaved.
    precondition None: plain GMRES, z_j = v_j"""
    n = len(b)
    norm = lambda v: np.sqrt(v @ v)
    bnorm = norm(b)
    x0, s0 = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
    r = b.copy()
    out = []
    while len(out) < K:
        beta = norm(r)
        m = min(restart, K - len(out))
        V, Z = np.zeros((m + 1, n), dtype=dt), np.zeros((m, n), dtype=dt)
        H = np.zeros((m + 1, m), dtype=dt)
        cs, sn, g = np.zeros(m, dtype=dt), np.zeros(m, dtype=dt), np.zeros(m + 1, dtype=dt)
        V[0], g[0] = r / beta, beta
        for j in range(m):
            Z[j] = V[j] if precondition is None else precondition(V[j])
            w = mv(Z[j])
            for _ in range(2):
                h = V[:j + 1] @ w
                w = w - V[:j + 1].T @ h
                H[:j + 1, j] += h
            hn = norm(w)
            H[j + 1, j] = hn
            for i in range(j):
                H[i, j], H[i + 1, j] = cs[i] * H[i, j] + sn[i] * H[i + 1, j], -sn[i] * H[i, j] + cs[i] * H[i + 1, j]
            d = np.sqrt(H[j, j] * H[j, j] + hn * hn)
            cs[j], sn[j] = H[j, j] / d, hn / d
            H[j, j], H[j + 1, j] = d, 0
            g[j + 1], g[j] = -sn[j] * g[j], cs[j] * g[j]
            k = j + 1
            y = np.zeros(k, dtype=dt)
            for i in range(k - 1, -1, -1):
                y[i] = (g[i] - H[i, i + 1:k] @ y[i + 1:]) / H[i, i]
            x = x0 + Z[:k].T @ y
            s = s0 + np.abs(Z[:k]).T @ np.abs(y)
            rk = b - mv(x)
            out.append((x, s, norm(rk) / bnorm, norm(amv(s)) / bnorm))
            assert hn > 0, "no happy breakdown inside the iterations a test asks for"
            V[j + 1] = w / hn
        x0, s0, r = x, s, rk
    return out


def _pack(out):
    return [Iterate(k + 1, stack(x), stack(s), float(rho), float(rs)) for k, (x, s, rho, rs) in enumerate(out)]


def fgmres_iterates(H, b, K, restart=50):
    """flexible GMRES, right-preconditioned by H's cycle, on the unscaled system, restarted every `restart` vectors from the true residual as fgmres_outer
    does -> [Iterate k = 1 .. K] in H's dtype (np.longdouble: the reference)"""
    A = H.A[0]
    return _pack(_iterates(H.dt, A.mv, A.amv, H.precondition, interleave(np.asarray(b, dtype=float)).astype(H.dt), K, restart))


def fgmres_float64(rp, ci, blocks, n, aggregates, b, K, restart=50):
    """the checker: the same scheme in float64 as the device runs it"""
    return fgmres_iterates(Hierarchy(rp, ci, blocks, n, aggregates, dt=np.float64, like_device=True), b, K, restart)


def csr_product(indptr, indices, data, X):
    """M X for a CSR matrix of ANY row length (an empty row gives 0) and X of one or two axes, the row sums by reduceat in the precision of data and X"""
    indptr = np.asarray(indptr, dtype=np.int64)
    terms = data * X[indices] if X.ndim == 1 else data[:, None] * X[indices]
    out = np.zeros((len(indptr) - 1,) + X.shape[1:], dtype=terms.dtype)
    filled = np.flatnonzero(np.diff(indptr) > 0)
    if len(filled):
        out[filled] = np.add.reduceat(terms, indptr[filled], axis=0)
    return out


class ObsTerm:
    """the factored data term scale Psi^T W Psi of the first field (fdapde_block_set_obs), applied as its two rectangular products in dtype dt"""

    def __init__(self, Psi, weights, scale, dt):
        P = Psi.tocsr().copy()
        P.sum_duplicates()
        P.sort_indices()
        T = P.T.tocsr()
        T.sort_indices()
        self.P = (P.indptr, P.indices, P.data.astype(dt))
        self.T = (T.indptr, T.indices, T.data.astype(dt))
        self.w = (np.ones(P.shape[0]) if weights is None else np.asarray(weights, dtype=float)).astype(dt)
        self.scale, self.dt = dt(scale), dt

    def apply(self, x1, absolute=False):
        """scale Psi^T W Psi x1, or |scale| |Psi|^T |W| |Psi| |x1|"""
        f = np.abs if absolute else (lambda v: v)
        P, T = ((m[0], m[1], f(m[2])) for m in (self.P, self.T))
        return f(self.scale) * csr_product(*T, f(self.w) * csr_product(*P, f(x1)))

    def diagonal(self):
        """the term's share of every DOF's diagonal entry: scale sum_k w_k Psi[k, i]^2"""
        ip, idx, v = self.T
        return self.scale * csr_product(ip, idx, v * v, self.w)


def _gmres(rp, ci, blocks, n, b, K, restart, dt, like_device, obs=None):
    bv = np.stack([np.zeros(len(ci)) if v is None else np.asarray(v, dtype=float) for v in blocks], axis=1)
    A = BlockCsr(rp, ci, bv, dt)
    assert A.n == n
    diag = A.diagonal_blocks()
    if obs is not None:   # the diagonal blocks of the full matrix: the term's share goes to a11
        term = ObsTerm(*obs, dt)
        diag = diag.copy()
        diag[:, 0] += term.diagonal()
    dinv = block_diag_inverse(diag, dt, like_device)
    At = A.left_scaled(dinv, like_device)
    bt = _dinv_apply(dinv, interleave(np.asarray(b, dtype=float)).astype(dt))
    if obs is None:
        return _pack(_iterates(dt, At.mv, At.amv, None, bt, K, restart))

    def first_field(z):
        return np.stack([z, np.zeros_like(z)], axis=1).reshape(-1)

    def mv(x):   # (as launch_obs_term: the scaled pattern product, then D^-1 [z; 0] added)
        return At.mv(x) + _dinv_apply(dinv, first_field(term.apply(x.reshape(-1, 2)[:, 0])))

    def amv(x):
        return At.amv(x) + _dinv_apply(np.abs(dinv), first_field(term.apply(x.reshape(-1, 2)[:, 0], absolute=True)))

    return _pack(_iterates(dt, mv, amv, None, bt, K, restart))


def gmres_iterates(rp, ci, blocks, n, b, K, restart=50, obs=None):
    """GMRES(restart) on D^-1 A z = D^-1 b, D^-1 formed in np.longdouble -> [Iterate]: x_k, s = sum_j |y_j| |v_j|, rho_k and res_scale of the SCALED system.
    obs = (Psi, weights, scale): A and D are the full matrix's, A + scale [Psi^T W Psi, 0; 0, 0], the term applied as its two rectangular products"""
    return _gmres(rp, ci, blocks, n, b, K, restart, LD, False, obs)


def gmres_float64(rp, ci, blocks, n, b, K, restart=50, obs=None):
    return _gmres(rp, ci, blocks, n, b, K, restart, np.float64, True, obs)


# ---- the units of the bounds -----------------------------------------------------------------------------------------------------------------------
def field_ratios(x, ref):
    """FDAPDE_SOLVER_BLOCK_AMG's unit: per field (f, g), max |x - ref.x| / (u max s) -- the coarse solve spreads its rounding over the whole domain, and
    lambda scales the two fields differently"""
    n = len(ref.x) // 2
    err = np.abs(np.asarray(x).astype(LD) - ref.x)
    return [float(err[h].max() / (U * ref.s[h].max())) for h in (slice(0, n), slice(n, 2 * n))]


def entry_ratio(x, ref):
    """the GMRES stage's unit: max_i |x - ref.x|_i / (u s_i) over the entries with s_i > 0; entries with s_i = 0 must be exactly 0 (-> inf otherwise)"""
    err = np.abs(np.asarray(x).astype(LD) - ref.x)
    live = ref.s > 0
    if (err[~live] != 0).any():
        return float("inf")
    return float((err[live] / (U * ref.s[live])).max()) if live.any() else 0.0


def relres_ratio(relres, ref):
    return abs(float(relres) - ref.rho) / (U * ref.res_scale)


# ---- the cases and the constants both tests share ---------------------------------------------------------------------------------------------------
# (mesh, order, lambda, advection, knobs, the k a solve stops at); meshes are meshgen's
AMG_CASES = {
    "a": (("unit_square", 16), 1, 1e-2, False, {}, (1, 2, 3, 5, 8)),
    "b": (("unit_square", 32), 1, 1e-4, False, {}, (1, 2, 3, 5, 8)),
    "c": (("unit_cube", 8), 1, 1e-4, False, {}, (1, 2, 3, 5)),
    "d": (("unit_cube", 5), 2, 1e-2, False, {}, (1, 2, 3, 5)),
    "e": (("unit_square", 32), 1, 1e-4, False, dict(amg_absorb=1), (1, 2, 3, 5)),
    "f": (("unit_square", 16), 1, 1e-2, True, {}, (1, 2, 3, 5)),
    "g": (("unit_square", 16), 1, 1e-2, False, dict(amg_coarse_rows=256), (1, 2, 3)),
    "h": (("unit_square", 16), 1, 1e-2, False, dict(gmres_m=3), (5,)),
}
AMG_COARSE_ROWS = 64
# (system of AMG_CASES, knobs, right-hand side, k)
GMRES_CASES = {
    "a": ("a", {}, "smoothing", (1, 2, 3, 5, 8)),
    "c": ("c", {}, "smoothing", (1, 2, 3, 5, 8)),
    "d": ("d", {}, "smoothing", (1, 2, 3, 5, 8)),
    "f": ("f", {}, "smoothing", (1, 2, 3, 5, 8)),
    "a-restart": ("a", dict(gmres_m=3), "smoothing", (5, 7)),
    "a-unit": ("a", {}, "unit", (1, 2, 3)),
}
# c(k) = 4 r_cpu(k) rounded up to a power of two, r_cpu the worst ratio of the float64 checkers above against the reference over the cases and both units
# (the iterate's and relres'): tests/test_block_iter_cpu.py measures it on the oracle's matrices and fails if a constant no longer fits or exceeds 2^12
C_AMG = {1: 64.0, 2: 16.0, 3: 16.0, 5: 32.0, 8: 16.0}
C_GMRES = {1: 2048.0, 2: 4096.0, 3: 256.0, 5: 128.0, 7: 32.0, 8: 64.0}
C_MAX = 2.0 ** 12
# the GMRES stage with a factored data term live (block_obs_ref's system: the (1,1) block is the term's alone), on the mesh, order and lambda of a system
# of AMG_CASES: (system, design as kron_obs_ref.design_psi takes it, k).  Each runs under block_obs_team = 8 and = 64 against the same reference; a set of
# constants of its own by the same rule
GMRES_OBS_CASES = {
    "a-areal": ("a", ("tiles", 2), (1, 2, 3, 5, 8)),      # 4 tiles: rows of 81 entries
    "a-points": ("a", ("points", 400), (1, 2, 3, 5, 8)),  # rows of 3
}
OBS_TEAMS = (8, 64)
C_GMRES_OBS = {1: 256.0, 2: 32.0, 3: 64.0, 5: 64.0, 8: 64.0}


def constant_for(r_cpu):
    return float(2.0 ** np.ceil(np.log2(max(4.0 * r_cpu, 1.0))))


# ---- the profile the CPU tests write (tests/test_block_iter_cpu.py, tests/test_kron_iter_cpu.py) -------------------------------------------------------
def write_profile(path, header, stages, tag, lines):
    """replace the block of lines that starts with `tag`: the header, the CPU tables in a fixed order, then whatever else the file holds (the GPU's lines)"""
    import os

    old = open(path).read().splitlines() if os.path.exists(path) else []
    groups = {t: [ln for ln in old if ln.startswith(t)] for t in stages}
    groups[tag] = lines
    rest = [ln for ln in old if ln and not ln.startswith("#") and not ln.startswith(tuple(stages))]
    new = list(header) + [ln for t in stages for ln in groups[t]] + rest
    if new != old:   # (a run that measures what is committed leaves the file alone)
        with open(path, "w") as fh:
            fh.write("\n".join(new) + "\n")


def constants_table(path, header, stages, stage, cases, measure, constants):
    """measure(name, K) -> {k: worst ratio} for every (name, ks) of cases; writes the stage's lines and holds the committed constants to the rule"""
    worst, lines = {}, []
    for name, ks in cases:
        ratios = measure(name, max(ks))
        for k in ks:
            worst[k] = max(worst.get(k, 0.0), ratios[k])
        lines.append(f"cpu {stage} {name}: " + " ".join(f"{k}={ratios[k]:.3g}" for k in ks))
    lines.append(f"cpu {stage} c(k) = 4 r_cpu(k) rounded up to a power of two: " + " ".join(f"{k}={constant_for(worst[k]):g}" for k in sorted(worst)))
    print("\n".join(lines))
    write_profile(path, header, stages, f"cpu {stage} ", lines)
    assert sorted(worst) == sorted(constants)
    for k in sorted(worst):
        assert 4.0 * worst[k] <= constants[k], (stage, k, worst[k], constants[k])   # (r_cpu still fits c / 4)
        assert constants[k] <= C_MAX, "a case whose checker needs more is replaced by a better-conditioned one: the constant is not raised"
    return worst


def interior_dof(rp, n):
    """a DOF with a row of the greatest length (an interior one) near the middle of the numbering"""
    length = np.diff(rp)
    full = np.flatnonzero(length == length.max())
    return int(full[np.argmin(np.abs(full - n // 2))])


def unit_rhs(n, dof):
    """one unit entry in the f-part"""
    b = np.zeros(2 * n)
    b[dof] = 1.0
    return b
