"""Extended-precision reference for the k-th iterate of Jacobi-scaled CG and BiCGStab, with the per-entry scale its error is measured in -- plain numpy,
nothing of the library.

In exact arithmetic iterate k of CG (or of BiCGStab with the shadow residual r0) on

    At x^ = bt,   At = S A S,   bt = S (f - A g~),   S = diag(1 / sqrt|a_ii|),   u = S x^ + g~

is ONE vector: the recurrence variant, the storage form, the partition into workgroups and their hand-offs do not change it.  `System` takes the float64 data
the kernels receive (pattern, values fetched BEFORE the first solve, force vector, boundary mask, Dirichlet data), does the Dirichlet reduction itself and
forms At and bt in np.longdouble (64-bit mantissa: within 0.01 u of 60-digit mpmath, tests/test_krylov_ref_cpu.py); `cg_iterates` / `bicgstab_iterates` run
the textbook recurrences on it.

The scale of entry i of iterate k is the magnitude of everything that was added up to make it,

    CG:        s_i = (1 / sqrt d_i) sum_{m<k} |alpha_m| (|At| |p_m|)_i
    BiCGStab:  s_i = (1 / sqrt d_i) sum_{m<k} |alpha_m| (|At| |p_m|)_i + |omega_m| (|At| |s_m|)_i

(At has a unit diagonal, so |p_m,i| is part of it).  Where s_i = 0 the Krylov front has not arrived and the entry is exactly 0 in x^, exactly g~_i in u.

The float64 checkers (`cg_float64`, `cg_fused_float64`, `bicgstab_float64`) are the same recurrences in float64 with the scale and the scaled matrix formed as
the kernels form them (1.0 / sqrt, (si * v) * sj).  They are the measuring stick for the tolerance of the GPU tests, never the thing tested."""
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble must carry a 64-bit mantissa (x87 extended or wider) on the machine that runs the reference"
U = 2.0 ** -53


@dataclass
class Iterate:
    k: int
    x: np.ndarray        # S x^_k on the interior DOFs (u without the lift)
    s: np.ndarray        # the per-entry scale of x, same units
    rho: float           # ||r_k|| / ||bt||  (the recurrence residual)
    alpha: float = 0.0   # of step k - 1
    beta: float = 0.0
    omega: float = 0.0
    Ap: np.ndarray = None    # At p_{k-1}
    pmax: float = 0.0        # max_i |p_{k-1,i}|
    rho_est: float = None    # fused-estimate checker only: sqrt of (alpha^2 Ap.Ap - r.r) / bt.bt


@dataclass
class System:
    """The Jacobi-scaled interior system of (rowptr, colidx, vals, f, bnd, g) in dtype `dt`; `like_kernels`: S and At rounded as k_jacobi_scale / k_scale_matrix do"""
    rowptr: np.ndarray
    colidx: np.ndarray
    vals: np.ndarray
    f: np.ndarray
    bnd: np.ndarray = None
    g: np.ndarray = None
    dt: type = LD
    like_kernels: bool = False
    interior: np.ndarray = field(init=False)

    def __post_init__(self):
        dt = self.dt
        n = self.rowptr.size - 1
        rp = np.asarray(self.rowptr, dtype=np.int64)
        ci = np.asarray(self.colidx, dtype=np.int64)
        rows = np.repeat(np.arange(n), np.diff(rp))
        bnd = np.zeros(n, dtype=bool) if self.bnd is None else np.asarray(self.bnd).astype(bool)
        self.n = n
        self.gt = np.where(bnd, 0.0 if self.g is None else np.asarray(self.g, dtype=float), 0.0)
        v = np.asarray(self.vals, dtype=float).astype(dt)
        b = np.asarray(self.f, dtype=float).astype(dt) - _rowsum(v * self.gt.astype(dt)[ci], rp, n, dt)   # f - A g~
        self.interior = np.nonzero(~bnd)[0]
        ni = self.interior.size
        new = np.full(n, -1, dtype=np.int64)
        new[self.interior] = np.arange(ni)
        keep = (~bnd[rows]) & (~bnd[ci])
        r2, c2, v2 = new[rows[keep]], new[ci[keep]], v[keep]
        self.indptr = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=ni))]).astype(np.int64)
        self.rows, self.cols = r2, c2
        self.row_len = np.diff(self.indptr)
        assert (self.row_len > 0).all(), "every interior row holds at least its diagonal"
        dmask = r2 == c2
        d = np.zeros(ni, dtype=dt)
        d[r2[dmask]] = v2[dmask]
        assert (d > 0).all(), "the reference is for positive diagonals (no tiny-diagonal rule)"
        self.d = d
        if self.like_kernels:
            self.S = 1.0 / np.sqrt(d)
            self.At = (self.S[r2] * v2) * self.S[c2]
        else:
            self.S = dt(1) / np.sqrt(d)
            self.At = v2 * self.S[r2] * self.S[c2]
        self.absAt = np.abs(self.At)
        self.bt = self.S * b[self.interior]
        self.ni = ni

    def mv(self, x):
        return np.add.reduceat(self.At * x[self.cols], self.indptr[:-1])

    def amv(self, x):
        return np.add.reduceat(self.absAt * np.abs(x)[self.cols], self.indptr[:-1])

    def lift(self, x_int):
        """full-length u = S x^ + g~ from an iterate's x"""
        u = self.gt.astype(np.result_type(x_int.dtype, float)).copy()
        u[self.interior] += x_int
        return u

    def spread(self, a_int):
        """a quantity of the interior DOFs on all DOFs (0 on Dirichlet DOFs)"""
        out = np.zeros(self.n, dtype=a_int.dtype)
        out[self.interior] = a_int
        return out


def _rowsum(prod, rp, n, dt):
    out = np.zeros(n, dtype=dt)
    nz = np.diff(rp) > 0
    out[nz] = np.add.reduceat(prod, rp[:-1][nz]) if prod.size else 0
    return out


def _cg(sy, K, fused):
    dt = sy.dt
    x = np.zeros(sy.ni, dtype=dt)
    r = sy.bt.copy()
    p = r.copy()
    bb = r @ r
    rr = bb
    acc = np.zeros(sy.ni, dtype=dt)
    out = []
    for k in range(1, K + 1):
        Ap = sy.mv(p)
        pAp = p @ Ap
        alpha = rr / pAp
        acc = acc + abs(alpha) * sy.amv(p)
        pmax = float(np.abs(p).max())
        x = x + alpha * p
        r = r - alpha * Ap
        rr_new = r @ r                       # the explicit r.r: alpha of the next step in both variants
        rr_est = alpha * alpha * (Ap @ Ap) - rr
        beta = (rr_est if fused else rr_new) / rr
        p = r + beta * p
        out.append(Iterate(k, sy.S * x, sy.S * acc, float(np.sqrt(rr_new / bb)), float(alpha), float(beta), 0.0, Ap, pmax,
                           float(np.sqrt(max(rr_est, 0) / bb)) if fused else None))
        rr = rr_new
    return out


def _bicgstab(sy, K):
    dt = sy.dt
    x = np.zeros(sy.ni, dtype=dt)
    r = sy.bt.copy()
    r0 = r.copy()
    p = r.copy()
    bb = r @ r
    rho = r0 @ r
    acc = np.zeros(sy.ni, dtype=dt)
    out = []
    for k in range(1, K + 1):
        v = sy.mv(p)
        alpha = rho / (r0 @ v)
        s = r - alpha * v
        t = sy.mv(s)
        omega = (t @ s) / (t @ t)
        acc = acc + abs(alpha) * sy.amv(p) + abs(omega) * sy.amv(s)
        pmax = float(np.abs(p).max())
        x = x + alpha * p + omega * s
        r = s - omega * t
        rho_new = r0 @ r
        beta = (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        rho = rho_new
        out.append(Iterate(k, sy.S * x, sy.S * acc, float(np.sqrt((r @ r) / bb)), float(alpha), float(beta), float(omega), v, pmax))
    return out


def _system(A, b, dt, like_kernels):
    """A: a System of another dtype or a tuple (rowptr, colidx, vals[, bnd, g]) with b the force vector"""
    if isinstance(A, System):
        if A.dt is dt and A.like_kernels == like_kernels and b is None:
            return A
        return System(A.rowptr, A.colidx, A.vals, A.f if b is None else b, A.bnd, A.g, dt=dt, like_kernels=like_kernels)
    return System(A[0], A[1], A[2], b, *A[3:], dt=dt, like_kernels=like_kernels)


def cg_iterates(A, b, K):
    """textbook CG on At x^ = bt in np.longdouble -> [Iterate k = 1 .. K]"""
    return _cg(_system(A, b, LD, False), K, False)


def bicgstab_iterates(A, b, K):
    """textbook BiCGStab (shadow residual r0) on At x^ = bt in np.longdouble -> [Iterate k = 1 .. K]"""
    return _bicgstab(_system(A, b, LD, False), K)


def cg_float64(A, b, K):
    return _cg(_system(A, b, np.float64, True), K, False)


def cg_fused_float64(A, b, K):
    return _cg(_system(A, b, np.float64, True), K, True)


def bicgstab_float64(A, b, K):
    return _bicgstab(_system(A, b, np.float64, True), K)


def ratio(x, ref):
    """max_i |x - ref.x|_i / (u s_i) over the entries with s_i > 0; entries with s_i = 0 must be exactly 0 (-> inf otherwise)"""
    err = np.abs(np.asarray(x).astype(LD) - ref.x)
    live = ref.s > 0
    if (err[~live] != 0).any():
        return float("inf")
    return float((err[live] / (U * ref.s[live])).max()) if live.any() else 0.0


def symmetric_storage_bound(sy, iterates, k, max_len):
    """F_i of iterate k for the symmetric storage of the single-launch CG (kernels_persist.h, fixed-point accumulators: the quantum of a block's accumulator
    is max_len max|at| max|p| 2^-56 or finer, and an entry collects at most len_i roundings to it per product):
    F_i = (1 / sqrt d_i) sum_{m<k} |alpha_m| len_i max_len max|at| max|p_m| 2^-56, with the GLOBAL max|p_m| standing in for the block's"""
    amax = float(sy.absAt.max())
    tot = sum(abs(it.alpha) * it.pmax for it in iterates[:k])
    return sy.S * (sy.row_len.astype(LD) * LD(max_len) * LD(amax) * LD(tot) * LD(2.0 ** -56))


def symmetric_storage_residual_slack(sy, iterates, k, max_len):
    """the same bound on the recurrence residual r_k = bt - sum_m alpha_m At p_m, as a share of ||bt||: what the fixed-point accumulators may move
    ||r_k|| / ||bt|| by (| ||a|| - ||b|| | <= ||a - b||)"""
    Fr = symmetric_storage_bound(sy, iterates, k, max_len) / sy.S
    return float(np.sqrt(Fr @ Fr) / np.sqrt(sy.bt @ sy.bt))


# ---- 60 digits (systems of at most 400 rows: tests/test_krylov_ref_cpu.py) -----------------------------------------------------------------------------
def _mp_system(rowptr, colidx, vals, f, bnd=None, g=None):
    import mpmath as mp

    sy = System(rowptr, colidx, vals, f, bnd, g)   # (for the index sets; the numbers are redone from the float64 inputs)
    assert sy.ni <= 400
    M = mp.mpf
    gt = [M(float(v)) for v in sy.gt]
    rp, ci = np.asarray(rowptr), np.asarray(colidx)
    b = []
    for i in sy.interior:
        acc = M(float(f[i]))
        for q in range(rp[i], rp[i + 1]):
            acc -= M(float(vals[q])) * gt[ci[q]]
        b.append(acc)
    new = {int(i): j for j, i in enumerate(sy.interior)}
    rowsA = []
    for i in sy.interior:
        rowsA.append([(new[int(ci[q])], M(float(vals[q]))) for q in range(rp[i], rp[i + 1]) if int(ci[q]) in new])
    d = [next(v for (j, v) in row if j == i) for i, row in enumerate(rowsA)]
    S = [1 / mp.sqrt(abs(v)) for v in d]
    At = [[(j, v * S[i] * S[j]) for (j, v) in row] for i, row in enumerate(rowsA)]
    bt = [S[i] * b[i] for i in range(sy.ni)]
    return At, bt, S


def _mp_mv(At, x, absolute=False):
    import mpmath as mp

    if absolute:
        return [mp.fsum(abs(v) * abs(x[j]) for (j, v) in row) for row in At]
    return [mp.fsum(v * x[j] for (j, v) in row) for row in At]


def mp_iterates(rowptr, colidx, vals, f, K, bnd=None, g=None, method="cg", digits=60):
    """the same two recurrences in mpmath -> [(x as list of mpf, s as list of mpf, rho as mpf)], k = 1 .. K"""
    import mpmath as mp

    with mp.workdps(digits):
        At, bt, S = _mp_system(rowptr, colidx, vals, f, bnd, g)
        n = len(bt)
        dot = lambda a, b: mp.fsum(a[i] * b[i] for i in range(n))
        x = [mp.mpf(0)] * n
        r = list(bt)
        p = list(r)
        r0 = list(r)
        bb = dot(r, r)
        rr = bb
        rho = bb
        acc = [mp.mpf(0)] * n
        out = []
        for _ in range(K):
            if method == "cg":
                Ap = _mp_mv(At, p)
                alpha = rr / dot(p, Ap)
                ap = _mp_mv(At, p, True)
                acc = [acc[i] + abs(alpha) * ap[i] for i in range(n)]
                x = [x[i] + alpha * p[i] for i in range(n)]
                r = [r[i] - alpha * Ap[i] for i in range(n)]
                rr_new = dot(r, r)
                beta = rr_new / rr
                p = [r[i] + beta * p[i] for i in range(n)]
                rr = rr_new
            else:
                v = _mp_mv(At, p)
                alpha = rho / dot(r0, v)
                s = [r[i] - alpha * v[i] for i in range(n)]
                t = _mp_mv(At, s)
                omega = dot(t, s) / dot(t, t)
                ap, asv = _mp_mv(At, p, True), _mp_mv(At, s, True)
                acc = [acc[i] + abs(alpha) * ap[i] + abs(omega) * asv[i] for i in range(n)]
                x = [x[i] + alpha * p[i] + omega * s[i] for i in range(n)]
                r = [s[i] - omega * t[i] for i in range(n)]
                rho_new = dot(r0, r)
                beta = (rho_new / rho) * (alpha / omega)
                p = [r[i] + beta * (p[i] - omega * v[i]) for i in range(n)]
                rho = rho_new
                rr = dot(r, r)
            out.append(([S[i] * x[i] for i in range(n)], [S[i] * acc[i] for i in range(n)], mp.sqrt(rr / bb)))
        return out
