"""Extended-precision reference for the k-th iterate of FDAPDE_SOLVER_AMG (csrc/eng_amg.hip), with the scale its error is measured in -- plain numpy, nothing
of the library (tests/test_amg_iter_cpu.py, tests/test_gpu_amg_iterates.py).  The scalar counterpart of tests/block_iter_ref.py: what does not depend on the
form -- the written-out elimination, the flexible GMRES loop, constant_for, relres_ratio -- is imported from there.

DATA from the device: the aggregates of every level (fdapde_amg_aggregates; -1 = a row of no aggregate, the Dirichlet rows of fdapde_solve's level 0) and the
damping omega_l of every level that has a next one (fdapde_amg_damping), taken as the exact float64 the cycle kernels take, and the order of level 0's rows
(fdapde_amg_order), which only the check of omega needs.  Everything numerical that is built on
them is RESTATED in np.longdouble: the Galerkin sums of piecewise-constant P (entries with a side in no aggregate are dropped), D^-1 (0 on the rows of no
aggregate), the cycle

    zt = om D^-1 r,   r_c = P^T (r - A zt),   z = zt + P e,   out = z + om D^-1 (r - A z),

the coarse correction e below the finest level -- two steps around the next level's cycle in k_amg_coef's reading, guards included: flexible CG for a
symmetric hierarchy, GCR otherwise --, the last level solved exactly, and flexible GMRES on K u = rhs from the Dirichlet lift (K: A with unit rows on the
Dirichlet DOFs, rhs: f on the free rows and g on the Dirichlet rows), its stop rule and relres relative to the lift's residual as amg_run_cols.  With the
aggregates and omega fixed, iterate k of that scheme is ONE vector in exact arithmetic.

omega itself is checked apart: `damping` restates level_prepare's estimator (15 power steps on D^-1 A off k_amg_hashvec's vector -- a function of the row index
in the device's order --, 1.5 / the last Rayleigh root) in any dtype, and the GPU test holds the device's omega to the np.longdouble one within OMEGA_RTOL.

The scale of entry i of iterate k is s = sum_j |y_j| |z_j| over the correction vectors so far (block_iter_ref's); res_scale = || |K| s || / ||r_lift||.

`Hierarchy(..., dt=np.float64, like_device=True)` and `iterates_float64` are the same scheme in float64 as the device runs it (the last level as the explicit
inverse of the row-equilibrated matrix, Gram-Schmidt twice, Givens rotations): the measuring stick for the constants, never the thing tested."""
import numpy as np

from amg_absorb_ref import hashvec
from block_iter_ref import LD, U, C_MAX, LAST_LEVEL_ROWS, Iterate, _iterates, _rows_of, constant_for, lu_partial_pivoting, lu_solve, relres_ratio  # noqa: F401


class Csr:
    """rows on a pattern in dtype dt; every row holds an entry (its diagonal), so row sums go by reduceat"""

    def __init__(self, rp, ci, a, dt):
        self.rp, self.ci, self.n, self.dt = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), len(rp) - 1, dt
        self.a = np.asarray(a, dtype=dt)
        assert self.a.shape == self.ci.shape and (np.diff(self.rp) > 0).all()

    def mv(self, x):
        return np.add.reduceat(self.a * x[self.ci], self.rp[:-1])

    def amv(self, x):
        return np.add.reduceat(np.abs(self.a) * np.abs(x)[self.ci], self.rp[:-1])

    def diagonal(self):
        d = np.flatnonzero(_rows_of(self.rp) == self.ci)
        assert len(d) == self.n, "every row holds its diagonal entry"
        return self.a[d]

    def dense(self):
        M = np.zeros((self.n, self.n), dtype=self.dt)
        M[_rows_of(self.rp), self.ci] = self.a
        return M


def galerkin(A, agg, nc):
    """P^T A P of the map row -> aggregate (-1: none): every coarse entry the sum of its fine entries; entries with a side in no aggregate are dropped"""
    ai, aj = agg[_rows_of(A.rp)], agg[A.ci]
    keep = np.flatnonzero((ai >= 0) & (aj >= 0))
    keys = ai[keep] * np.int64(nc) + aj[keep]
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    uniq = ks[starts]
    rp_c = np.zeros(nc + 1, dtype=np.int64)
    np.add.at(rp_c, uniq // nc + 1, 1)
    return Csr(np.cumsum(rp_c), uniq % nc, np.add.reduceat(A.a[keep][order], starts), A.dt)


def diag_inverse(A, agg, dt):
    """D^-1, 0 on the rows of no aggregate"""
    d = A.diagonal()
    assert (d[agg >= 0] != 0).all()
    return np.where(agg >= 0, dt(1.0) / np.where(agg >= 0, d, dt(1.0)), dt(0.0))


def damping(A, dinv, dt=LD, order=None):
    """level_prepare's estimate in dtype dt: 15 power steps on D^-1 A off k_amg_hashvec's vector (0 where D^-1 is), omega = 1.5 / sqrt(y.y / x.x) of the last.
    The vector is a function of the row index in the DEVICE's order: order[i] = the row of A that the device's row i is (fdapde_amg_order; None: A's own order)"""
    start = hashvec(A.n)
    if order is not None:
        order = np.asarray(order, dtype=np.int64)
        assert np.array_equal(np.sort(order), np.arange(A.n)), "a permutation of the rows"
        start = np.zeros(A.n)
        start[order] = hashvec(A.n)
    x = np.where(dinv == 0, 0.0, start).astype(dt)
    lam = dt(0.0)
    for _ in range(15):
        y = dinv * A.mv(x)
        h0, h1 = x @ x, y @ y
        if not h0 > 0 or not np.isfinite(h1):
            break
        lam = np.sqrt(h1 / h0)
        if not h1 > 0:
            break
        x = y * (dt(1.0) / np.sqrt(h1))
    return dt(1.5) / lam if lam > 0 and np.isfinite(lam) else dt(0.0)


class Hierarchy:
    """the levels FDAPDE_SOLVER_AMG builds on GIVEN aggregates and damping: aggregates[l][i] = the row of level l + 1 that row i of level l belongs to or -1
    (level 0 in the caller's numbering), omegas[l] the float64 damping of level l.  The level-0 matrix is K or A alike: its rows of no aggregate are never
    read (D^-1 is 0 there and the correction is), except by the one-level form, whose level is K itself.  .rows[l] / .entries[l] as fdapde_amg_hierarchy"""

    def __init__(self, rp, ci, a, aggregates, omegas, symmetric, dt=LD, like_device=False):
        self.dt, self.like_device, self.sym = dt, like_device, bool(symmetric)
        self.A = [Csr(rp, ci, a, dt)]
        self.agg, self.members, self.dinv = [], [], []
        self.om = [dt(float(w)) for w in omegas]
        assert len(self.om) == len(aggregates)
        for l, agg in enumerate(aggregates):
            A = self.A[-1]
            agg = np.asarray(agg, dtype=np.int64)
            nc = int(agg.max()) + 1
            assert agg.shape == (A.n,) and agg.min() >= -1 and len(np.unique(agg[agg >= 0])) == nc, "a map onto the next level's rows"
            assert l == 0 or agg.min() == 0, "only level 0 has rows of no aggregate"
            live = np.flatnonzero(agg >= 0)
            order = live[np.argsort(agg[live], kind="stable")]
            self.agg.append(agg)
            self.members.append((order, np.flatnonzero(np.concatenate([[True], np.diff(agg[order]) != 0]))))
            self.dinv.append(diag_inverse(A, agg, dt))
            self.A.append(galerkin(A, agg, nc))
        self.rows = [A.n for A in self.A]
        self.entries = [len(A.ci) for A in self.A]
        last = self.A[-1].dense()
        assert last.shape[0] <= LAST_LEVEL_ROWS, last.shape
        if like_device:   # the explicit inverse of the row-equilibrated matrix (csrc/eng_dense.hip), one refinement step where max |I - A X| asks for it
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
        return np.add.reduceat(r[order], starts)

    def prolong(self, l, e):
        agg = self.agg[l]
        return np.where(agg >= 0, e[np.maximum(agg, 0)], self.dt(0.0))

    def cycle(self, l, r):
        A, omd = self.A[l], self.om[l] * self.dinv[l]
        zt = omd * r
        z = zt + self.prolong(l, self.correction(l + 1, self.restrict(l, r - A.mv(zt))))
        return z + omd * (r - A.mv(z))

    def correction(self, m, b):
        """the last level exactly; elsewhere two steps around the cycle with k_amg_coef's dots and rules -- flexible CG: rho1 = c.v, alpha1 = c.b, gamma = d.v,
        rho2 = d.w - gamma^2 / rho1, alpha2 = d.rt; GCR: rho1 = v.v, alpha1 = v.b, gamma = v.w, rho2 = w.w - gamma^2 / rho1, alpha2 = w.rt --: a step that
        cannot be taken (rho <= 0, not finite) contributes nothing"""
        if m + 1 == len(self.A):
            return self.solve_last(b)
        A, zero = self.A[m], self.dt(0)
        c = self.cycle(m, b)
        v = A.mv(c)
        rho1, t1 = (c @ v, c @ b) if self.sym else (v @ v, v @ b)
        a1 = t1 / rho1 if rho1 > 0 and np.isfinite(rho1) else zero
        if not np.isfinite(a1):
            a1 = zero
        rt = b - a1 * v
        d = self.cycle(m, rt)
        w = A.mv(d)
        gamma, t1, t2 = (d @ v, d @ w, d @ rt) if self.sym else (v @ w, w @ w, w @ rt)
        rho2 = t1 - gamma * gamma / rho1 if rho1 > 0 else zero
        cd = t2 / rho2 if rho2 > 0 and np.isfinite(rho2) else zero
        cc = a1 - (cd * gamma / rho1 if rho1 > 0 else zero)
        if not (np.isfinite(cd) and np.isfinite(cc)):
            cd, cc = zero, a1
        return cc * c + cd * d

    def precondition(self, v):
        return self.solve_last(v) if len(self.A) == 1 else self.cycle(0, v)

    def estimated_damping(self, order0=None, dt=None):
        """the restated estimator on this hierarchy's own matrices, per level that has a next one; order0: the device's order of level 0's rows"""
        dt = dt or self.dt
        return [damping(Csr(A.rp, A.ci, A.a.astype(dt), dt), dinv.astype(dt), dt, order0 if l == 0 else None) for l, (A, dinv) in enumerate(zip(self.A[:-1], self.dinv))]


def unit_rows(rp, ci, a, bnd):
    """K: A with unit rows on the Dirichlet DOFs (fem_solver_base.h's row-zeroed system)"""
    rows = _rows_of(np.asarray(rp, dtype=np.int64))
    on = np.asarray(bnd, dtype=bool)[rows]
    return np.where(on, (rows == np.asarray(ci)).astype(float), np.asarray(a, dtype=float))


def iterates(H, rhs, K, lift=None, restart=50):
    """flexible GMRES on (level 0 of H) u = rhs from `lift` (the Dirichlet data on the Dirichlet rows, 0 elsewhere; None: from 0), right-preconditioned by H's
    cycle -> [Iterate k = 1 .. K] in H's dtype: x, s, rho_k and res_scale relative to the lift's residual.  Level 0 of H must be K (unit_rows)"""
    A = H.A[0]
    x0 = np.zeros(A.n, dtype=H.dt) if lift is None else np.asarray(lift, dtype=float).astype(H.dt)
    r0 = np.asarray(rhs, dtype=float).astype(H.dt) - A.mv(x0)
    return [Iterate(k + 1, x0 + d, s, float(rho), float(rs)) for k, (d, s, rho, rs) in enumerate(_iterates(H.dt, A.mv, A.amv, H.precondition, r0, K, restart))]


def iterates_float64(rp, ci, a, aggregates, omegas, symmetric, rhs, K, lift=None, restart=50):
    """the checker: the same scheme in float64 as the device runs it"""
    return iterates(Hierarchy(rp, ci, a, aggregates, omegas, symmetric, dt=np.float64, like_device=True), rhs, K, lift, restart)


def iterate_ratio(x, ref, free):
    """the unit of the bound: max |x - ref.x| / (u max s) over the free entries"""
    err = np.abs(np.asarray(x).astype(LD) - ref.x)[free]
    return float(err.max() / (U * ref.s[free].max()))


def teams(rows, entries):
    """the lane count of every level that has a next one, as level_prepare computes it from rows and entries"""
    return [4 if e / r <= 10.0 else 8 if e / r <= 24.0 else 16 for r, e in zip(rows[:-1], entries[:-1])]


# ---- the cases and the constants both tests share ---------------------------------------------------------------------------------------------------
# name -> (mesh of meshgen, order, operator, path, knobs, the k a solve stops at).  operator "reaction": -Lap + 2, "adr": -Lap + b.grad + 1 (b = ADVECTION);
# path "solve": fdapde_solve with the Dirichlet data dirichlet_data (the boundary DOFs belong to no aggregate), "handle": fdapde_lin_compute / fdapde_lin_solve
AMG_CASES = {
    "a": (("unit_square", 24), 1, "reaction", "solve", {}, (1, 2, 3, 5, 8)),          # >= 3 levels, 4-lane teams, agg == -1 on the Dirichlet DOFs
    "b": (("unit_square", 48), 1, "reaction", "handle", {}, (1, 2, 3, 5, 8)),         # >= 5 levels: flexible CG nested three deep
    "c": (("unit_square", 24), 1, "adr", "solve", {}, (1, 2, 3, 5, 8)),               # GCR steps, a non-symmetric Galerkin chain
    "d": (("unit_cube", 12), 1, "reaction", "handle", dict(amg_absorb=1), (1, 2, 3, 5, 8)),   # aggregates of more than four rows, 8-lane teams
    "e": (("unit_square", 20), 2, "reaction", "solve", {}, (1, 2, 3, 5, 8)),          # rows longer than one team pass, long and short rows on one level
    "f": (("unit_square", 7), 1, "reaction", "solve", {}, (1,)),                     # below amg_coarse_rows: the dense level alone, with its boundary mask
    "h": (("unit_cube", 6), 2, "reaction", "handle", {}, (1, 2, 3, 5, 8)),            # 3-D P2: 16-lane teams
}
COLS_CASES = {"b": (1, 3), "d": (1, 3)}   # case g: these systems at amg_cols = 8, every column against its own reference at these k
AMG_COARSE_ROWS = 64
ADVECTION = [3.0, -1.5]
# c(k) = 4 r_cpu(k) rounded up to a power of two, r_cpu the worst ratio of the float64 checker above against the reference over the cases and both units (the
# iterate's and relres'): tests/test_amg_iter_cpu.py measures it on the oracle's matrices and fails if a constant no longer fits or exceeds 2^12
C_AMG = {1: 512.0, 2: 256.0, 3: 256.0, 5: 256.0, 8: 256.0}
# the damping: 4 times the worst relative difference of the float64 estimator from the np.longdouble one over the levels of the cases, rounded up to a power of
# two (measured by the same test, which fails if it no longer fits or exceeds 1e-9)
OMEGA_RTOL = 2.0 ** -49
OMEGA_RTOL_MAX = 1e-9


def dirichlet_data(coords):
    return 0.3 * np.cos(2.0 * coords[:, 0]) + coords[:, -1]


def forcing(q):
    """the forcing of the "solve" cases at the quadrature nodes"""
    return 1.0 + np.sin(3.0 * q[:, 0]) * q[:, 1]


def columns(A_mv, coords, interior, n):
    """case g's eight columns: smooth, a unit vector at an interior DOF, zeros, one scaled by 1e-150, four random"""
    B = np.random.default_rng(11).standard_normal((n, 8))
    B[:, 0] = A_mv(np.prod(np.cos(np.pi * coords), axis=1))
    B[:, 1] = 0.0
    B[interior[len(interior) // 2], 1] = 1.0
    B[:, 2] = 0.0
    B[:, 3] *= 1e-150
    return B
